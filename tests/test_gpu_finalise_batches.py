"""The N = 2048 wave kernel finalises 64 frames per wave at a time from a ring of stash rows in global memory
(amcx_wave_kernel.h, wave_body RING; amcx.hip, pool_ring); a launch without a ring runs batches of four from the LDS stash.
Per-frame arithmetic is the same whichever batch a frame lands in, so everything here is compared bit for bit."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
N = 2048
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


def _base_frames():
    """96 ordinary frames: the six modulations at two SNRs."""
    from amcpy_amd import synth
    return np.concatenate([synth.host_block(m, snr, 8, N, seed=300 + 7 * i + j)
                           for i, m in enumerate(synth.MODS6) for j, snr in enumerate((0.0, 12.0))]).astype(np.complex64)


def _near_pi_tie_frames(n_frames, seed):
    """Noisy frames with 40 planted steps antiparallel to within one or two fp32 ulps of one component (the fixture of
    test_gpu_parity.test_phase_steps_within_an_ulp_of_pi): the sweep flags them, the finaliser takes f5 / f9 again."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n_frames, N)) + 1j * rng.standard_normal((n_frames, N))).astype(np.complex64)
    for f in range(n_frames):
        for n in rng.choice(np.arange(2, N - 2, 3), size=40, replace=False):
            re, im = np.float32(x[f, n].real), np.float32(x[f, n].imag)
            k = int(rng.choice([-2, -1, 1, 2]))
            scale = np.float32(2.0 ** int(rng.integers(-1, 2)))
            re2, im2 = np.float32(-re * scale), np.float32(-im * scale)
            for _ in range(abs(k)):
                im2 = np.nextafter(im2, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
            x[f, n + 1] = re2 + 1j * im2
    return x


def _cancelling_frames(n_frames, seed):
    """Noiseless QPSK at 8 samples per symbol with exactly balanced squares (the fixture of
    test_gpu_parity.test_cancelling_cumulants_take_the_fp64_path): C41 and C60 cancel, the finaliser takes ids 10-18 from fp64 sums."""
    rng = np.random.default_rng(seed)
    sps, n_sym = 8, N // 8
    pts = np.exp(1j * (np.pi / 4 + np.pi / 2 * np.arange(4)))
    x = np.empty((n_frames, N), np.complex128)
    for f in range(n_frames):
        sym = np.concatenate([rng.choice([0, 2], n_sym // 2), rng.choice([1, 3], n_sym - n_sym // 2)])
        rng.shuffle(sym)
        x[f] = np.repeat(pts[sym], sps) * np.exp(1j * rng.uniform(0, 2 * np.pi))
        x[f] += (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * 1e-4
    return x.astype(np.complex64)


def _special_frames():
    """Frames that take one of the finaliser's slow paths: near-pi ties, cancelling cumulants, and both kinds as well as
    ordinary frames outside the fp32 sums' range (times 2^28 and 2^-36: the in-kernel re-run on a scaled copy)."""
    ties, canc, plain = _near_pi_tie_frames(4, 11), _cancelling_frames(4, 12), _base_frames()[:4]
    out_of_range = np.concatenate([ties[:2] * np.float32(2.0 ** 28), canc[:2] * np.float32(2.0 ** -36),
                                   plain[:2] * np.float32(2.0 ** 28), plain[2:] * np.float32(2.0 ** -36)])
    return np.concatenate([ties, canc, out_of_range]).astype(np.complex64)


def _features(x):
    torch = _torch()
    from amcpy_amd.features import features18
    y = features18(x)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("n_frames", [1, 63, 64, 65, 256 * 16 * 64 + 3])
def test_every_kind_of_partial_batch(n_frames):
    """1, 63, 64 and 65 frames, and 64 per wave of a 256-CU grid plus 3 (whole batches, and whatever the dynamic work
    distribution leaves each wave at the end): every row equals the row of the same frames fed 64 at a time."""
    torch = _torch()
    rng = np.random.default_rng(n_frames)
    base = torch.from_numpy(_base_frames()).cuda()
    x = base[torch.from_numpy(rng.integers(0, base.shape[0], size=n_frames)).cuda()].contiguous()
    got = _features(x).cpu().numpy()
    from amcpy_amd.features import features18
    want = torch.empty((n_frames, 18), dtype=torch.float32, device="cuda")
    for lo in range(0, n_frames, 64):
        features18(x[lo:lo + 64], out=want[lo:lo + 64])
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    bad = np.flatnonzero(~np.all((got == want) | (np.isnan(got) & np.isnan(want)), axis=1))
    assert bad.size == 0, (n_frames, bad[:8], got[bad[:2]], want[bad[:2]])


def test_flagged_frames_in_the_first_middle_and_last_lane_of_a_batch():
    """A wave takes its frames in aligned runs of four and a full batch is sixteen of them, so with every run laid out
    (special, ordinary, ordinary, special) lanes 0, 31 and 63 of every full batch -- and the first and last lane of most
    partial ones -- hold a frame that is out of range, cancelling, within an ulp of a +-pi step, or two of these at once.
    Two batches' worth of frames per wave.  Every row equals the row of the same frame in a small launch of its own."""
    torch = _torch()
    rng = np.random.default_rng(5)
    uniq = np.concatenate([_base_frames(), _special_frames()])
    n_plain = _base_frames().shape[0]
    n_runs = 2 * _cus() * 16 * 16 + 5
    pick = rng.integers(0, n_plain, size=(n_runs, 4))
    pick[:, 0] = n_plain + rng.integers(0, uniq.shape[0] - n_plain, size=n_runs)
    pick[:, 3] = n_plain + rng.integers(0, uniq.shape[0] - n_plain, size=n_runs)
    pick = pick.reshape(-1)[:-1]                                   # the last run is short
    alone = _features(torch.from_numpy(uniq).cuda()).cpu().numpy()
    assert not np.isneginf(alone[:, 4]).any() and ((alone[:, 4] >= 0) | np.isnan(alone[:, 4])).all()
    x = torch.from_numpy(uniq).cuda()[torch.from_numpy(pick).cuda()].contiguous()
    got = _features(x).cpu().numpy()
    want = alone[pick]
    bad = np.flatnonzero(~np.all((got == want) | (np.isnan(got) & np.isnan(want)), axis=1))
    assert bad.size == 0, (bad.size, bad[:8], pick[bad[:8]], got[bad[:2]], want[bad[:2]])


def test_two_streams_at_once_each_equal_to_its_serial_result():
    """Launches that overlap never share a ring: two streams, full grids, different inputs, three rounds."""
    torch = _torch()
    from amcpy_amd.features import features18
    rng = np.random.default_rng(9)
    base = torch.from_numpy(np.concatenate([_base_frames(), _special_frames()])).cuda()
    n = _cus() * 16 * 24 + 7
    a = base[torch.from_numpy(rng.integers(0, base.shape[0], size=n)).cuda()].contiguous()
    b = base[torch.from_numpy(rng.integers(0, base.shape[0], size=n + 130)).cuda()].contiguous()
    ya, yb = features18(a), features18(b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            oa = features18(a)
        with torch.cuda.stream(s2):
            ob = features18(b)
        outs.append((oa, ob))
    torch.cuda.synchronize()
    for oa, ob in outs:
        assert _same(oa.cpu().numpy(), ya.cpu().numpy()) and _same(ob.cpu().numpy(), yb.cpu().numpy())


def test_graph_capture_and_two_replays_equal_the_eager_call():
    torch = _torch()
    from amcpy_amd.features import features18
    rng = np.random.default_rng(13)
    base = torch.from_numpy(np.concatenate([_base_frames(), _special_frames()])).cuda()
    x = base[torch.from_numpy(rng.integers(0, base.shape[0], size=_cus() * 16 * 20 + 1)).cuda()].contiguous()
    eager = _features(x).cpu().numpy()
    out = torch.zeros((x.shape[0], 18), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        features18(x, out=out)                                     # the stream's first call is outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            features18(x, out=out)
    for _ in range(2):
        out.fill_(-1.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy(), eager)
    # a stream whose FIRST call arrives inside a capture
    s2, g2 = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    s2.wait_stream(torch.cuda.current_stream())
    out2 = torch.zeros_like(out)
    with torch.cuda.graph(g2, stream=s2):
        features18(x, out=out2)
    g2.replay()
    torch.cuda.synchronize()
    assert _same(out2.cpu().numpy(), eager)


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


def test_ring_form_equals_the_lds_form(tmp_path):
    """The same launch in a fresh process that was told to use no ring (AMCX_WAVE_RING=0: batches of four from the LDS
    stash, the form a launch without a ring falls back to) and in this one; also the feature-subset kernels, which share
    the body, against the 18-feature kernel's columns."""
    torch = _torch()
    rng = np.random.default_rng(17)
    uniq = np.concatenate([_base_frames(), _special_frames()])
    pick = rng.integers(0, uniq.shape[0], size=_cus() * 16 * 70 + 9)
    np.save(tmp_path / "uniq.npy", uniq)
    np.save(tmp_path / "pick.npy", pick)
    env = dict(os.environ, AMCX_WAVE_RING="0")
    subprocess.run([sys.executable, "-c", _CHILD.format(repo=str(REPO)), str(tmp_path / "uniq.npy"), str(tmp_path / "pick.npy"),
                    str(tmp_path / "lds.npy")], check=True, env=env, timeout=600)
    lds = np.load(tmp_path / "lds.npy")
    x = torch.from_numpy(uniq).cuda()[torch.from_numpy(pick).cuda()].contiguous()
    ring = _features(x).cpu().numpy()
    bad = np.flatnonzero(~np.all((ring == lds) | (np.isnan(ring) & np.isnan(lds)), axis=1))
    assert bad.size == 0, (bad.size, bad[:8], pick[bad[:8]])
    from amcpy_amd import _lib
    from amcpy_amd.features import features18
    for mask in (_lib.FEATURES_NO_SPECTRAL, _lib.FEATURES_CUMULANTS):
        cols = [j for j in range(18) if (mask >> j) & 1]
        sub = features18(x, feature_ids=[j + 1 for j in cols])
        torch.cuda.synchronize()
        assert _same(sub.cpu().numpy()[:, cols], ring[:, cols]), hex(mask)
