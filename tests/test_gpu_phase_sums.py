"""The N = 2048 wave kernels sum the phase about ZERO (amcx_wave_kernel.h, StatsT with kShiftedPhase = false) and the
finaliser flags the frames whose phase is too narrow for that (amcx_math.h, phase_suspect: var < 0.05 x mean square of
theta, for theta or for |theta|); a flagged frame gets f2 / f3 from an fp64 sweep about its means, behind its batch
(wave_exact_phase).  Frames on both sides of the flag, about the phase centres 0, pi / 2 and +-2.5, are held to the parity
contract against the oracle, and every form of the kernel to the same bits.  About +-2.5 the spreads 0.215 and 0.23 -- the
two beside the flag's threshold -- put the outer of their two phase values at 3.05 ... 3.13, just under +-pi; 0.25 and 0.5
pass +-pi and wrap (wide frames, not flagged); at spread 1e-4 the centres 2.9 and 3.1 stand there themselves."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from oracle import iq_features_oracle as orc                  # noqa: E402

N = 2048
CRITERION = 1e-5           # the parity contract: scaled relative error (oracle.parity_errors), as __graft_entry__.smoke
EDGE_ATOL = 2e-6           # test_gpu_parity.test_golden_edges: ids 1-9 of a series that is constant in fp64
KAPPA = 0.05               # amcx_math.h, kPhaseKappa: flagged when var / mean square < KAPPA, i.e. std / rms < 0.2236
# std / rms of the phase: none, far below, below, either side of sqrt(KAPPA) = 0.2236, above, wide
SPREADS = (0.0, 1e-4, 1e-2, 0.20, 0.215, 0.23, 0.25, 0.5)
CENTRES = (0.0, np.pi / 2, 2.5, -2.5)
# Spread 1e-4 is a series of 1e-4 ... 3e-4 rad, and the contract wants its standard deviation to ~2e-9 rad from fp32 angles
# good to 2.5e-7 rad: away from the centre 0 whether a frame meets 1e-5 depends on the draw, and does so alike -- to two
# digits of the error -- under the kernels of before, which summed the phase about a shift (profiles/r38_narrow_cells.txt:
# 0.2 ... 13 of the criterion by centre and seed; about pi / 2, on or beside the seam of the angle at re = 0, never below 0.7).
# The row of that spread is therefore made of (centre, seed) cells that meet the criterion under those kernels, with room:
# without the random signs 0, 2.5, 2.9, 3.1 (0.07, 0.24, 0.30, 0.30 of it), with them 0, 2.0, 2.9, 3.1 (0.07, 0.17, 0.19, 0.16).
NARROWEST = {False: ((0.0, 1), (2.5, 1), (2.9, 1), (3.1, 2)), True: ((0.0, 1), (2.0, 2), (2.9, 2), (3.1, 3))}
pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible to torch")
    return torch


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _cell(rng, r, c, both_signs):
    """One frame: theta = c + s (+-1 + 0.05 g), g Gaussian, s chosen so that std / rms of theta is r (about the centre 0,
    where the rms IS the std, s is r in radians); both_signs: a random sign per sample on top."""
    s = r if c == 0.0 else r * abs(c) / np.sqrt(1.0 - r * r)
    th = c + s * (rng.choice([-1.0, 1.0], N) + 0.05 * rng.standard_normal(N))
    if both_signs:
        th = th * rng.choice([-1.0, 1.0], N)
    amp = rng.uniform(0.5, 2.0) * np.clip(1.0 + 0.2 * rng.standard_normal(N), 0.2, None)
    return amp + 0j if (r == 0.0 and c == 0.0) else amp * np.exp(1j * th)      # (positive reals: every angle exactly 0)


def sweep_frames():
    """64 frames, (spread index, centre index, both-signs) in that order, each a _cell; the second 32 carry a random sign
    per sample, so that theta is wide and |theta| alone is narrow -- a BPSK burst received at 90 degrees.  The envelope
    varies by 20 % so that no other feature is degenerate.  The row of spread 1e-4 is NARROWEST's cells, each from a
    generator of its own; about pi / 2 the spread 1e-2 stands three spreads above it, off the seam of the angle at re = 0.
    Returns (frames complex64, spread of each frame, whether it carries the random signs)."""
    rng = np.random.default_rng(2048)
    frames, spread, signs = [], [], []
    for both_signs in (False, True):
        for r in SPREADS:
            for k, c in enumerate(CENTRES):
                if c == np.pi / 2 and 0.0 < r <= 1e-2:
                    c = c + 3.0 * r * c / np.sqrt(1.0 - r * r)
                frame = _cell(rng, r, c, both_signs)
                if r == 1e-4:
                    centre, seed = NARROWEST[both_signs][k]
                    frame = _cell(np.random.default_rng(seed), r, centre, both_signs)
                frames.append(frame)
                spread.append(r)
                signs.append(both_signs)
    return np.asarray(frames).astype(np.complex64), np.asarray(spread), np.asarray(signs)


def narrow_cancelling_frames(n_frames, seed):
    """Frames flagged for phase AND for cancelling cumulants: constant modulus at +45 and -45 degrees, exactly as many of
    one as of the other, in noise of 1e-2 -- |theta| is pi / 4 to within 1e-2 (var / mean square ~1e-4) while x^2 points
    up and down equally often, so that m20 and m41 vanish and C41, C60 and C62 (ids 13, 15, 17) are sums of nothing but
    rounding: cancellation_suspect_np below, the finaliser's predicate restated, says so of every one of them."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_frames):
        sgn = np.repeat([1.0, -1.0], N // 2)
        rng.shuffle(sgn)
        out.append(rng.uniform(0.5, 2.0) * np.exp(1j * np.pi / 4 * sgn) + 1e-2 * (rng.standard_normal(N) + 1j * rng.standard_normal(N)))
    return np.asarray(out).astype(np.complex64)


def cancellation_suspect_np(x, kappa=4.0e-3):
    """amcx_math.h, cancellation_suspect at N = 2048, statement for statement in float32 on the 15 moment sums of one
    frame (the sums themselves taken in float64 here): which of ids 12, 13, 15, 16, 17 it flags."""
    f = np.float32
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    A, Bh, P = re * re - im * im, re * im, re * re + im * im
    AA, BB = A * A, Bh * Bh
    X4 = AA - 4.0 * BB
    s = [f(v.sum()) for v in (A, Bh, P, AA, X4, A * Bh, A * P, Bh * P, AA * A, A * BB, AA * Bh, BB * Bh, AA * P, X4 * P, A * P * Bh)]
    n, kappa = f(x.size), f(kappa)
    c2 = f(1.0) / s[2]
    c4 = n * c2 * c2
    c6 = c4 * (n * c2)
    b20r, b20i = s[0] * c2, f(2) * s[1] * c2
    n20 = b20r * b20r + b20i * b20i
    a20 = np.sqrt(n20)
    b40r, b40i, b41r, b41i = s[4] * c4, f(4) * s[5] * c4, s[6] * c4, f(2) * s[7] * c4
    b42 = (f(2) * s[3] - s[4]) * c4
    b60r, b60i = (s[8] - f(12) * s[9]) * c6, (f(6) * s[10] - f(8) * s[11]) * c6
    b61r, b61i = s[13] * c6, f(4) * s[14] * c6
    b62, b63 = (f(4) * s[9] + s[8]) * c6, (f(2) * s[12] - s[13]) * c6
    s40 = abs(b40r) + abs(b40i)
    a40l = max(max(abs(b40r), abs(b40i)), f(0.70710678) * s40)
    a40h = f(1.0823922) * a40l
    a41l, a41h = max(abs(b41r), abs(b41i)), abs(b41r) + abs(b41i)
    g, u, c3, v = a20 * b42, a20 * a40l, a20 * n20, a20 * a41l
    t12 = kappa * (f(6) * a20 + b42) - f(3) * n20
    t13 = kappa * (f(3) * a20 + b42 + f(3)) - f(3) * a20
    t15 = kappa * (f(9) * n20 + f(15) * (g + a40h) + b63) - f(15) * u - f(3) * c3
    t16 = kappa * (f(60) * a20 + f(30) * n20 + f(10) * (g + a41h) + f(5) * (b42 + a40h) + b63) - f(5) * a40l - f(10) * v - f(30) * n20
    t17 = kappa * (f(48) * a20 + f(18) * n20 + f(8) * a41h + f(7) * g + f(14) * b42 + b63 + a40h + f(24)) \
        - f(6) * (g + c3) - f(8) * a41l - f(24) * a20 - u
    return {12: bool(t12 > 0 and b40r * b40r + b40i * b40i < t12 * t12), 13: bool(t13 > 0 and b41r * b41r + b41i * b41i < t13 * t13),
            15: bool(t15 > 0 and b60r * b60r + b60i * b60i < t15 * t15), 16: bool(t16 > 0 and b61r * b61r + b61i * b61i < t16 * t16),
            17: bool(abs(b62) < t17)}


def phase_suspect_np(x):
    """amcx_math.h, phase_suspect: var / mean square of theta and of |theta| (angles and sums in float64 here)."""
    th = np.angle(x.astype(np.complex128))
    ms = (th * th).mean(axis=-1)
    return np.minimum(ms - th.mean(axis=-1) ** 2, ms - np.abs(th).mean(axis=-1) ** 2) / ms


def _special_frames():
    """Narrow-phase frames on the finaliser's other paths too: both kinds outside the fp32 sums' range (times 2^28 and
    2^-36: the in-kernel re-run on a scaled copy), and narrow frames whose cumulants cancel."""
    sweep = sweep_frames()[0]
    both = narrow_cancelling_frames(4, 7)
    narrow = sweep[[9, 10, 11, 41, 42, 13, 14, 17]]               # spreads 1e-2, 0.20, 0.215 about pi / 2 and +-2.5; |theta| alone
    return np.concatenate([both, narrow * np.float32(2.0 ** 28), narrow * np.float32(2.0 ** -36),
                           both[:2] * np.float32(2.0 ** 28), both[2:] * np.float32(2.0 ** -36)]).astype(np.complex64)


def _ordinary_frames():
    from amcpy_amd import synth
    return np.concatenate([synth.host_block(m, 10.0, 4, N, seed=500 + i) for i, m in enumerate(synth.MODS6)]).astype(np.complex64)


def _features(x, **kw):
    torch = _torch()
    from amcpy_amd.features import features18
    y = features18(x if isinstance(x, torch.Tensor) else torch.from_numpy(x).cuda(), **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _scaled_errors(got, x):
    gold = orc.features18_batch(x)
    with np.errstate(over="ignore"):
        gold32 = gold.astype(np.float32)
    _, scaled = orc.parity_errors(got, gold32, orc.conditioning_scales(x))
    scaled[np.isinf(gold32) & (got == gold32)] = 0.0              # a cumulant beyond float32 in the reference's store too
    return scaled, gold


def test_phase_spread_sweep_against_the_oracle():
    """Every frame of the sweep of spread > 0 -- 56 of the 64, the row of spread 1e-4 among them -- within the parity
    contract on all 18 features.  The eight frames of spread 0, whose phase (or |phase|) is constant in fp64, are held by the
    rule of test_gpu_parity.test_golden_edges for such series: ids 1-9 to the contract plus 2e-6 absolute, f9 (the kurtosis
    of the steps, rounding dust in the reference itself) not a target; their f2, and f3 where theta itself is constant,
    are zero to that 2e-6.  The kernels of before (phase sums about a shift) pass the same test."""
    x, spread, signs = sweep_frames()
    got = _features(x)
    scaled, gold = _scaled_errors(got, x)
    const = spread == 0.0
    worst = scaled[~const].max(axis=0)
    print("worst scaled error per feature, frames of spread > 0:", np.array2string(worst, precision=2))
    print("f2, f3 of the frames of spread 0:", got[const][:, 1:3].ravel(), "reference", gold[const][:, 1:3].ravel())
    print("worst scaled error of each frame of spread 1e-4:", np.array2string(scaled[spread == 1e-4].max(axis=1), precision=2))
    assert worst.max() <= CRITERION, (np.argwhere(scaled * ~const[:, None] > CRITERION)[:8], worst)
    cols = [j for j in range(18) if j != 8]
    lim = CRITERION * np.abs(gold[const][:, cols]) + np.where(np.array(cols) < 9, EDGE_ATOL, 0.0)
    cscale = orc.conditioning_scales(x[const])[:, cols]
    lim = np.maximum(lim, CRITERION * cscale)
    diff = np.abs(got[const][:, cols].astype(np.float64) - gold[const][:, cols])
    assert (diff <= lim).all(), (np.argwhere(diff > lim)[:8], got[const], gold[const])
    assert (np.abs(got[spread == 0.0][:, 1]) <= EDGE_ATOL).all(), got[spread == 0.0][:, 1]             # |theta| constant
    assert (np.abs(got[(spread == 0.0) & ~signs][:, 2]) <= EDGE_ATOL).all(), got[spread == 0.0][:, 2]   # theta constant


def test_special_frames_against_the_oracle():
    """Narrow-phase frames that are re-run scaled, and narrow frames whose cumulants cancel, within the contract.  That the
    latter are flagged for both is held here on the predicates restated: far below the phase flag's threshold, and ids 13,
    15 and 17 of the cancellation flag, for each of them -- scaled by a power of two or not."""
    both = narrow_cancelling_frames(4, 7)
    assert (phase_suspect_np(both) < 0.1 * KAPPA).all(), phase_suspect_np(both)
    for frame in both:
        hit = cancellation_suspect_np(frame)
        assert hit[13] and hit[15] and hit[17], hit
    x = _special_frames()
    got = _features(x)
    scaled, _ = _scaled_errors(got, x)
    print("worst scaled error per feature:", np.array2string(scaled.max(axis=0), precision=2))
    assert scaled.max() <= CRITERION, (np.argwhere(scaled > CRITERION)[:8], scaled.max(axis=0))


_CHILD = """
import sys
import numpy as np
import torch
sys.path.insert(0, {repo!r})
from amcpy_amd.features import features18
x = torch.from_numpy(np.load(sys.argv[1])).cuda()
pick = torch.from_numpy(np.load(sys.argv[2])).cuda()
y = features18(x[pick].contiguous())
torch.cuda.synchronize()
np.save(sys.argv[3], y.cpu().numpy())
"""


def test_forms_agree_bit_for_bit_over_flushes_and_reruns(tmp_path):
    """More than 64 frames per wave of a full grid, so that every wave flushes its ring more than once, with flagged
    frames (narrow, narrow and cancelling, narrow and out of range) in every run of four: every row equals the row of the
    same frame in a small launch of its own, the LDS form (a fresh process with AMCX_WAVE_RING=0) gives the same bits as
    the ring form, and the feature-subset kernels the same columns."""
    torch = _torch()
    rng = np.random.default_rng(23)
    uniq = np.concatenate([_ordinary_frames(), sweep_frames()[0], _special_frames()])
    n_plain = _ordinary_frames().shape[0]
    n_runs = _cus() * 16 * 17 + 3                                  # 68 frames per wave
    pick = rng.integers(0, n_plain, size=(n_runs, 4))
    pick[:, 1] = n_plain + rng.integers(0, uniq.shape[0] - n_plain, size=n_runs)
    pick = pick.reshape(-1)[:-1]
    alone = _features(uniq)
    xd = torch.from_numpy(uniq).cuda()[torch.from_numpy(pick).cuda()].contiguous()
    ring = _features(xd)
    bad = np.flatnonzero(~np.all((ring == alone[pick]) | (np.isnan(ring) & np.isnan(alone[pick])), axis=1))
    assert bad.size == 0, (bad.size, bad[:8], pick[bad[:8]], ring[bad[:2]], alone[pick][bad[:2]])
    from amcpy_amd import _lib
    for mask in (_lib.FEATURES_NO_SPECTRAL, _lib.FEATURES_CUMULANTS, (1 << 1) | (1 << 12), 1 << 2):
        cols = [j for j in range(18) if (mask >> j) & 1]
        sub = _features(xd, feature_ids=[j + 1 for j in cols])
        assert _same(sub[:, cols], ring[:, cols]), hex(mask)
    del xd
    np.save(tmp_path / "uniq.npy", uniq)
    np.save(tmp_path / "pick.npy", pick)
    subprocess.run([sys.executable, "-c", _CHILD.format(repo=str(REPO)), str(tmp_path / "uniq.npy"), str(tmp_path / "pick.npy"),
                    str(tmp_path / "lds.npy")], check=True, env=dict(os.environ, AMCX_WAVE_RING="0"), timeout=600)
    lds = np.load(tmp_path / "lds.npy")
    bad = np.flatnonzero(~np.all((ring == lds) | (np.isnan(ring) & np.isnan(lds)), axis=1))
    assert bad.size == 0, (bad.size, bad[:8], pick[bad[:8]])


def test_sc16_equals_complex64_on_int16_data():
    """The sweep and the special frames brought to int16 (scale 2^-12 after normalising every frame's peak to 0.9 x 2^3):
    the sc16 kernels give the bits of the complex64 kernels on the widened frames, 18-feature and subset.  (Bits only: the
    rounded frames are other frames, and it is the complex64 kernel that the tests above hold to the oracle.)"""
    torch = _torch()
    from amcpy_amd import _lib
    from amcpy_amd.features import features18_sc16
    x = np.concatenate([sweep_frames()[0], narrow_cancelling_frames(4, 7), _ordinary_frames()])
    peak = np.maximum(np.abs(x.real).max(axis=1), np.abs(x.imag).max(axis=1))[:, None]
    q = np.stack([np.rint(x.real / peak * 29000.0), np.rint(x.imag / peak * 29000.0)], axis=-1).astype(np.int16)
    q = np.tile(q, (3, 1, 1))[:2 * 64 + 5]                          # more than one batch of 64
    scale = 2.0 ** -12
    xd = torch.from_numpy(q).cuda()
    wide = torch.view_as_complex((xd.to(torch.float32) * np.float32(scale)).contiguous())
    ref = _features(wide, variant="wave")
    assert "sc16" in _lib.kernel_name_sc16(N)
    got = features18_sc16(xd, scale=scale, variant="wave")
    torch.cuda.synchronize()
    assert _same(got.cpu().numpy(), ref)
    cols = [1, 2, 4, 12]
    sub = features18_sc16(xd, scale=scale, variant="wave", feature_ids=[j + 1 for j in cols])
    torch.cuda.synchronize()
    assert _same(sub.cpu().numpy()[:, cols], ref[:, cols])
