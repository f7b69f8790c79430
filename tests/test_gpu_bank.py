"""The polyphase filter bank (include/amcx.h, amcx_filter_bank; ABI 12) on the GPU.

THE REFERENCE is tests/bank_ref.py: channel c is the float64 down-converter of tests/ddc_ref.py with phase_step - c 2^64 / C.
THE CRITERION is |y - y64| <= (P + 8 + 7 log2 C) 2^-24 S for EVERY output of every channel (derived there); each test prints
the worst ratio it saw.  Taps come from +-[0.5, 1] so that every tap counts, phase_step is an odd 64-bit constant,
sample_index0 is no multiple of any C.  Everything that the contract calls bit-identical is compared as bytes."""
from fractions import Fraction

import numpy as np
import pytest

from amcpy_amd import _formats, _lib, bank, ddc
from tests import bank_ref, ddc_ref, stream_inputs

pytestmark = pytest.mark.gpu

FORMATS = list(ddc.FORMATS)
STEP = Fraction(ddc_ref.ODD_STEP, 1 << 64)
INDEX0 = (1 << 33) + 12345                  # odd, 57 mod 256: no multiple of any C
SHAPES = [(2, 1, 1), (2, 5, 2), (4, 4, 4), (8, 19, 5), (8, 64, 8), (64, 200, 32), (64, 1024, 64), (256, 513, 256), (256, 4096, 128),
          (16, 37, 16), (16, 256, 11), (32, 100, 32), (32, 1024, 24), (128, 300, 128), (128, 2048, 96)]
ALL_FORMATS_AT = [(8, 19, 5), (64, 200, 32), (256, 513, 256), (32, 100, 32), (128, 300, 128)]
POOL = 40_000                               # samples: the longest stream of these tests and some


_torch, _taps_dev = stream_inputs.torch, stream_inputs.taps_dev
_host, _dev, _wide = stream_inputs.bind(47, POOL)


def _run(x, T, Cn, D, **kw):
    y = bank.filter_bank(x, _taps_dev(T), Cn, D, **kw)
    _torch().cuda.synchronize()
    return y.cpu().numpy()


def _phase0(index0=INDEX0):
    return (index0 * ddc_ref.ODD_STEP) & ddc_ref.MASK64


@pytest.mark.parametrize("Cn,T,D,fmt", [(c, t, d, f) for c, t, d in SHAPES
                                        for f in (FORMATS if (c, t, d) in ALL_FORMATS_AT else ["cf32"])])
def test_criterion_against_float64(Cn, T, D, fmt):
    """M = 2 tile + 3: two tile seams and a ragged last tile, every channel, every output."""
    tile, _, lds = _lib.filter_bank_plan(T, Cn, D)
    M = 2 * tile + 3
    S = (M - 1) * D + T + (D - 1)                       # not the shortest stream that gives M
    assert bank.out_samples(S, T, Cn, D) == M and S <= POOL
    y = _run(_dev(fmt)[:S], T, Cn, D, shift=STEP, sample_index0=INDEX0)
    assert y.shape == (Cn, M) and y.dtype == np.complex64
    y64, s = bank_ref.reference(_wide(fmt)[:S], ddc_ref.make_taps(T), Cn, D, _phase0(), ddc_ref.ODD_STEP, INDEX0)
    r = bank_ref.worst_ratio(y, y64, s, T, Cn)
    print(f"bank criterion {fmt} C={Cn} T={T} D={D} tile={tile} lds={lds} M={M}: worst |err| / bound = {r:.4f} "
          f"(bound factor {bank_ref.bound_factor(T, Cn)})")
    assert r <= 1.0, (fmt, Cn, T, D, r)


@pytest.mark.parametrize("Cn,T,channels", [(4, 8, None), (256, 512, (0, 1, 86, 255))])
def test_criterion_against_float64_over_three_trips_of_the_grid(Cn, T, channels):
    """M = tile (2 grid + 1) + 3 at D = 1, the pre-mixer at an ODD step (the exact-arithmetic tests of this size,
    tests/test_gpu_chain_exact.py, stand at quarter turns, which a phase taken from another tile of the same workgroup would
    pass: grid tile D is a multiple of 4): every output of the channels against float64 (all four at C = 4; four of the 256,
    the reference being what takes the time)."""
    torch = _torch()
    D = 1
    tile, grid, _ = _lib.filter_bank_plan(T, Cn, D)
    M = tile * (2 * grid + 1) + 3
    tiles = -(-M // tile)
    S = (M - 1) * D + T
    print(f"bank criterion C={Cn} T={T} D={D}: {M} outputs = {tiles} tiles of {tile} over {grid} workgroups")
    assert tiles >= 2 * grid + 1 and bank.out_samples(S, T, Cn, D) == M
    host = stream_inputs.stream("cf32", S, np.random.default_rng(4700 + Cn))
    y = _run(torch.from_numpy(host).cuda(), T, Cn, D, shift=STEP, sample_index0=INDEX0)
    assert y.shape == (Cn, M)
    y64, s = bank_ref.reference(host.astype(np.complex128), ddc_ref.make_taps(T), Cn, D, _phase0(), ddc_ref.ODD_STEP, INDEX0,
                                channels=channels)
    r = bank_ref.worst_ratio(y if channels is None else y[list(channels)], y64, s, T, Cn)
    print(f"bank criterion C={Cn} T={T} D={D} over three trips: worst |err| / bound = {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("Cn", [2, 4, 8, 16, 32, 64, 128, 256])
def test_every_channel_every_branch(Cn):
    """One non-zero sample at each position of a window in turn (T = 2 C: both taps of every branch), batched as one stream
    with gaps of 2 T >= T between them.  Impulse j sits where the windows that hold it hold it at taps k = j mod D and beyond
    in steps of D; an output is h[k] x exp(-2 pi j c a / C) for the ONE impulse its window holds, within the criterion
    (S = |h[k]| |x|), and exactly 0 where the window holds none.  Independent of the reference; a wrong circular shift, bit
    reversal or tap index is off by O(1)."""
    torch = _torch()
    T, D, L = 2 * Cn, Cn, 4 * Cn
    h = ddc_ref.make_taps(T).astype(np.float64)
    rng = np.random.default_rng(Cn)
    amp = (rng.uniform(0.5, 1.0, T) * np.exp(2j * np.pi * rng.uniform(0, 1, T))).astype(np.complex64)
    S = T * L + T
    x = np.zeros(S, np.complex64)
    pos = np.arange(T) * L + T - 1 - np.arange(T)                       # impulse j: a multiple of D minus j, plus T - 1
    x[pos] = amp
    M = bank.out_samples(S, T, Cn, D)
    y = _run(torch.from_numpy(x).cuda(), T, Cn, D, sample_index0=INDEX0).astype(np.complex128)
    want = np.zeros((Cn, M), np.complex128)
    s = np.zeros(M)
    k = np.arange(M)[None, :] * D + T - 1 - pos[:, None]                # (T, M): the tap that meets impulse j in output m
    held = (0 <= k) & (k < T)
    assert held.sum(axis=0).max() == 1                                  # one impulse per window
    hit = int(held.sum())
    j, m = np.nonzero(held)
    a = (INDEX0 + pos[j]) % Cn
    amp128 = amp.astype(np.complex128)
    want[:, m] = (h[k[j, m]] * amp128[j])[None, :] * np.exp(-2j * np.pi * ((np.arange(Cn)[:, None] * a[None, :]) % Cn) / Cn)
    s[m] = np.abs(h[k[j, m]]) * np.abs(amp128[j])
    assert hit == 2 * T and len({(int(pos[j]) + INDEX0) % Cn for j in range(T)}) == Cn        # every tap, every rotation
    assert (y[:, s == 0.0] == 0).all(), "an output whose window holds no sample is not exactly 0"
    r = bank_ref.worst_ratio(y, want, s, T, Cn)
    print(f"bank impulses C={Cn} T={T}: {hit} (tap, instant) pairs x {Cn} channels: worst |err| / bound = {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("Cn,T,D", [(8, 64, 8), (8, 2048, 4), (64, 200, 32), (64, 1024, 64), (16, 256, 16), (128, 512, 128)])
def test_against_the_down_converter(Cn, T, D):
    """Every channel against amcx_tune_decimate with the equivalent phases (shift - c / C, the same sample_index0): both are
    within their criteria of the same exact value, so they differ by at most the sum of the two bounds."""
    fmt = "sc16"
    tile, _, _ = _lib.filter_bank_plan(T, Cn, D)
    M = tile + 3
    S = (M - 1) * D + T
    x = _dev(fmt)[:S]
    y = _run(x, T, Cn, D, shift=STEP, sample_index0=INDEX0).astype(np.complex128)
    sabs = np.abs(_wide(fmt)[:S])
    idx = np.arange(M)[:, None] * D + (T - 1 - np.arange(T))[None, :]
    s = sabs[idx] @ np.abs(ddc_ref.make_taps(T).astype(np.float64))
    bound = (T + 8 + bank_ref.bound_factor(T, Cn)) * ddc_ref.U * s
    worst = 0.0
    for c in range(Cn):
        one = ddc.tune_decimate(x, _taps_dev(T), D, shift=STEP - Fraction(c, Cn), sample_index0=INDEX0)
        err = np.abs(one.cpu().numpy().astype(np.complex128) - y[c])
        worst = max(worst, float(np.max(err / bound)))
    print(f"bank against the down-converter C={Cn} T={T} D={D}: worst |difference| / (sum of the bounds) = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("Cn,T,D", [(8, 19, 5), (64, 200, 32), (4, 1, 4), (16, 37, 11), (128, 300, 96)])
@pytest.mark.parametrize("fmt", ["cf32", "cu8"])
def test_chunk_invariance(fmt, Cn, T, D):
    torch = _torch()
    rng = np.random.default_rng(T + D)
    tile, _, _ = _lib.filter_bank_plan(T, Cn, D)
    S = (2 * tile + 40) * D + T + 3
    x = _dev(fmt)[:S]
    whole = _run(x, T, Cn, D, shift=STEP, sample_index0=INDEX0)
    M = whole.shape[1]
    # calls cut at random multiples of D, each told where in the stream it starts
    cuts = sorted({0, M} | set(rng.integers(0, M, 9).tolist()))
    parts = [_run(x[a * D:(b - 1) * D + T], T, Cn, D, shift=STEP, sample_index0=INDEX0 + a * D) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.concatenate(parts, axis=1).tobytes() == whole.tobytes(), (fmt, Cn, T, D, cuts)
    # the streaming form, cut anywhere: empty chunks, single samples, chunks below T (its stream begins at index 0)
    whole0 = _run(x, T, Cn, D, shift=STEP)
    fb = bank.FilterBank(ddc_ref.make_taps(T), Cn, D, STEP, fmt)
    got, pos = [], 0
    for n in [0, 1, max(T - 1, 1), 0] + rng.integers(1, S // 4, 30).tolist():
        got.append(fb.push(x[pos:pos + n]))
        pos = min(S, pos + n)
    assert pos == S
    torch.cuda.synchronize()
    assert torch.cat(got, dim=1).cpu().numpy().tobytes() == whole0.tobytes(), (fmt, Cn, T, D)
    assert whole0.tobytes() != whole.tobytes()


@pytest.mark.parametrize("Cn,T,D", [(8, 19, 5), (256, 513, 256), (32, 100, 32), (128, 300, 96)])
@pytest.mark.parametrize("fmt", ["sc16", "ci8", "cu8"])
def test_the_four_formats_give_the_same_bits(fmt, Cn, T, D):
    torch = _torch()
    tile, _, _ = _lib.filter_bank_plan(T, Cn, D)
    S = (tile + 5) * D + T
    widened = torch.from_numpy(_wide(fmt)[:S].astype(np.complex64)).cuda()          # exact: the values are float32
    a = _run(_dev(fmt)[:S], T, Cn, D, shift=STEP, sample_index0=INDEX0)
    b = _run(widened, T, Cn, D, shift=STEP, sample_index0=INDEX0)
    assert a.tobytes() == b.tobytes(), (fmt, Cn, T, D)


@pytest.mark.parametrize("fmt,offsets", [("cf32", (8,)), ("sc16", (4, 8, 12)), ("ci8", (2, 6, 14)), ("cu8", (2, 6, 14))])
def test_every_legal_misalignment_reads_the_same_samples(fmt, offsets):
    torch = _torch()
    Cn, T, D, S = 8, 19, 5, 6_011
    host = np.array(_host(fmt)[:S])
    nbytes = host.nbytes
    aligned = _run(_dev(fmt)[:S], T, Cn, D, shift=STEP, sample_index0=INDEX0)
    assert _dev(fmt).data_ptr() % 16 == 0
    arena = torch.zeros(nbytes + 32, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    raw = torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()
    for off in offsets:
        arena.fill_(0x5A)
        arena[off:off + nbytes] = raw
        x = arena[off:off + nbytes].view(_dev(fmt).dtype)
        x = x if fmt == "cf32" else x.view(S, 2)
        assert x.data_ptr() % 16 == off
        assert _run(x, T, Cn, D, shift=STEP, sample_index0=INDEX0).tobytes() == aligned.tobytes(), (fmt, off)


@pytest.mark.parametrize("Cn,T,D", [(8, 19, 5), (64, 200, 32)])
def test_a_wider_stride_leaves_the_gaps_untouched(Cn, T, D):
    torch = _torch()
    lib = _lib.load()
    fmt, G = "ci8", 7
    tile, _, _ = _lib.filter_bank_plan(T, Cn, D)
    M = tile + 1
    S = (M - 1) * D + T
    x = _dev(fmt)[:S]
    packed = _run(x, T, Cn, D, shift=STEP, sample_index0=INDEX0)
    stride = M + G
    buf = torch.full((G + Cn * stride,), -7.0 + 3.0j, dtype=torch.complex64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(cap, st=stride):
        return lib.amcx_filter_bank(x.data_ptr(), _formats.get(fmt).kind, S, _formats.get(fmt).scale, _phase0(), ddc_ref.ODD_STEP, INDEX0,
                                    _taps_dev(T).data_ptr(), T, Cn, D, buf.data_ptr() + 8 * G, st, cap, stream)
    need = (Cn - 1) * stride + M
    assert call(need - 1) == _lib.EINVAL and call(need, M - 1) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((buf == complex(-7.0, 3.0)).all()), "a refused call wrote"
    assert call(need) == _lib.OK
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    rows = got[G:].reshape(Cn, stride)
    assert (got[:G] == complex(-7.0, 3.0)).all() and (rows[:, M:] == complex(-7.0, 3.0)).all()
    assert np.ascontiguousarray(rows[:, :M]).tobytes() == packed.tobytes()
    # the Python entry with a wider `out`
    out = torch.full((Cn, stride), -7.0 + 3.0j, dtype=torch.complex64, device="cuda")
    view = bank.filter_bank(x, _taps_dev(T), Cn, D, shift=STEP, sample_index0=INDEX0, out=out)
    torch.cuda.synchronize()
    assert view.shape == (Cn, M) and view.cpu().numpy().tobytes() == packed.tobytes()
    assert bool((out[:, M:] == complex(-7.0, 3.0)).all())


@pytest.mark.parametrize("Cn", [2, 4])
@pytest.mark.parametrize("fmt", ["cf32", "ci8"])
def test_one_tap_is_the_input_times_an_exact_power_of_j(fmt, Cn):
    """phase0 = phase_step = 0, T = 1, h = {1}, D = 1: y[c, n] = x[n] (-j)^(c a(n) 4 / C), a(n) = (sample_index0 + n) mod C --
    swaps and sign changes of the components, compared with ==."""
    torch = _torch()
    S, index0 = 5_003, 3
    x = _dev(fmt)[:S]
    w = _wide(fmt)[:S].astype(np.complex64)
    y = bank.filter_bank(x, torch.ones(1, device="cuda"), Cn, 1, sample_index0=index0).cpu().numpy()
    assert y.shape == (Cn, S)
    a = (index0 + np.arange(S)) % Cn
    for c in range(Cn):
        q = (c * a * (4 // Cn)) % 4                                  # quarter turns clockwise
        re = np.select([q == 0, q == 1, q == 2, q == 3], [w.real, w.imag, -w.real, -w.imag])
        im = np.select([q == 0, q == 1, q == 2, q == 3], [w.imag, -w.real, -w.imag, w.real])
        assert (y[c].real == re).all() and (y[c].imag == im).all(), (fmt, Cn, c)


def test_graph_capture():
    torch = _torch()
    lib = _lib.load()
    Cn, T, D, S, fmt = 64, 200, 32, 9_000, "sc16"
    M = bank.out_samples(S, T, Cn, D)
    first, second = _dev(fmt)[:S], _dev(fmt)[S:2 * S]
    eager = [_run(first, T, Cn, D, shift=STEP, sample_index0=INDEX0), _run(second, T, Cn, D, shift=STEP, sample_index0=INDEX0)]
    assert eager[0].tobytes() != eager[1].tobytes()
    xin = first.clone()
    out = torch.zeros((Cn, M), dtype=torch.complex64, device="cuda")
    taps = _taps_dev(T)

    def launch():
        _lib.check(lib.amcx_filter_bank(xin.data_ptr(), _lib.SRC_SC16, S, _lib.SC16_SCALE, _phase0(), ddc_ref.ODD_STEP, INDEX0,
                                        taps.data_ptr(), T, Cn, D, out.data_ptr(), M, Cn * M, torch.cuda.current_stream().cuda_stream))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        launch()                                               # the stream's first call is outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            launch()
    for src, want in ((second, eager[1]), (first, eager[0])):
        xin.copy_(src)
        out.fill_(-1.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes()


# ---- end to end: the bank's rows as frames for the feature kernels ----------------------------------------------------
def _kurtosis_change(v, eta):
    """How far m4 / m2^2 of d = v - mean(v) can move when every d moves by at most eta: |dm2| <= 2 eta mean|d| + eta^2 and
    |dm4| <= 4 eta mean|d|^3 + 6 eta^2 m2 + 4 eta^3 mean|d| + eta^4, with mean|d| <= sqrt(m2) and mean|d|^3 <= m4^(3/4)."""
    d = v - v.mean()
    m2, m4 = float((d ** 2).mean()), float((d ** 4).mean())
    dm2 = 2 * eta * np.sqrt(m2) + eta ** 2
    dm4 = 4 * eta * m4 ** 0.75 + 6 * eta ** 2 * m2 + 4 * eta ** 3 * np.sqrt(m2) + eta ** 4
    assert m2 > dm2, "the frame's spread is no larger than the perturbation: kurtosis says nothing"
    k = m4 / m2 ** 2
    return max((m4 + dm4) / (m2 - dm2) ** 2 - k, k - (m4 - dm4) / (m2 + dm2) ** 2)


def _feature_moves(z, eps):
    """(18,) how far each of the oracle's features of the frame z (complex128, the exact stream) can move when every sample
    moves by at most eps.  With a = |z|, mu = mean(a), theta = angle(z), c = sqrt(N / (N - 1)) (std1 of a vector whose entries
    move by at most delta moves by at most c delta):
      1  max |Z_k|^2 / N: every |Z_k| moves by at most N eps                     -> 2 eps sqrt(N gamma) + N eps^2
      2, 3  std1(|theta|), std1(theta): an angle moves by asin(eps / a) <= (pi / 2) eps / min(a) =: dth (no sample near
            +-pi: asserted)                                                      -> c dth
      4  std1(|a / mu - 1|): a and mu move by eps                                -> c dcna, dcna = (1 + max(a) / mu) eps / (mu - eps)
      5  std1(phi), phi = the wrapped difference of theta over 2 pi (no wrap: asserted)   -> c dth / pi
      6  mu -> eps;   7  sqrt(sum a) / N -> eps / (2 sqrt(N (mu - eps)))
      8, 9  the kurtosis of a / mu - 1 and of phi: every centred value moves by twice its own move (the mean moves too)
      10 ... 18  |sum of terms|, a term = coefficient x product of moments, in all a mean of products of deg factors z or
            conj(z) (deg = 2, 4, 6): each factor's modulus is at most max(a) and moves by eps, so a term moves by at most
            |coefficient| ((max(a) + eps)^deg - max(a)^deg); the coefficients are the oracle's own (its terms at moments 1)."""
    from oracle import iq_features_oracle as orc
    N = z.shape[0]
    a, th = np.abs(z), np.angle(z)
    mu, amin, amax = float(a.mean()), float(a.min()) - eps, float(a.max())
    assert amin > eps
    c = np.sqrt(N / (N - 1))
    dth = np.pi / 2 * eps / amin
    dd = np.diff(th)
    assert np.abs(th).max() + dth < np.pi and np.abs(dd).max() + 2 * dth < np.pi
    gamma = float((np.abs(np.fft.fft(z)) ** 2).max()) / N
    dcna = (1 + amax / mu) * eps / (mu - eps)
    k = np.zeros(18)
    k[0] = 2 * eps * np.sqrt(N * gamma) + N * eps ** 2
    k[1] = k[2] = c * dth
    k[3] = c * dcna
    k[4] = c * dth / np.pi
    k[5] = eps
    k[6] = eps / (2 * np.sqrt(N * (mu - eps)))
    k[7] = _kurtosis_change(a / mu - 1, 2 * dcna)
    k[8] = _kurtosis_change(dd / (2 * np.pi), 2 * dth / np.pi)
    ones = orc.cumulant_terms({name: 1.0 for name in ("m20", "m21", "m22", "m40", "m41", "m42", "m43", "m60", "m61", "m62", "m63")})
    for fid in range(10, 19):
        deg = 2 if fid <= 11 else 4 if fid <= 14 else 6
        k[fid - 1] = sum(abs(t) for t in ones[fid]) * ((amax + eps) ** deg - amax ** deg)
    return k


def test_two_tones_end_to_end():
    """Two tones on raster channels 1 and 6 of 8, in noise, through filter_bank -> features18: each of the two channels' rows
    against features18 of the same channel taken with tune_decimate (shift -c / C, the same taps).

    THE BOUND.  Both routes' frames are fp32 approximations of the same exact stream y64: the bank's within
    eb = (P + 8 + 7 log2 C) 2^-24 S of it, the down-converter's within ed = (T + 8) 2^-24 S (the two criteria).  The feature
    kernel is within TOL = 1e-5 of the float64 oracle F on ITS OWN input, relative to max(|F|, S_j) (tests/test_gpu_parity.py:
    the feature parity bound).  So, with k_j(eps) how far F_j can move when every sample moves by eps (_feature_moves, from
    the exact stream alone),
        |f_j(bank) - f_j(ddc)| <= TOL (max(|F_j|, S_j) + k_j(eb)) + TOL (max(|F_j|, S_j) + k_j(ed)) + k_j(eb) + k_j(ed)
                               <= 2 TOL (max(|F_j|, S_j) + k_j(eb + ed)) + k_j(eb + ed)
    (every k_j is convex in eps and 0 at 0, so k_j(eb) + k_j(ed) <= k_j(eb + ed); the conditioning scale S_j is taken at y64,
    its own move being of second order, TOL k_j).  A row of the wrong channel is noise alone: off by O(1)."""
    torch = _torch()
    from amcpy_amd.features import features18
    from oracle import iq_features_oracle as orc
    Cn, P, N, K = 8, 16, 128, 4
    T, D = Cn * P, Cn
    taps = bank.design_bank_lowpass(Cn, P)
    M = N * K
    S = (M - 1) * D + T
    rng = np.random.default_rng(77)
    n = np.arange(S)
    tones = {1: (1.0, 0.5), 6: (0.7, -1.0)}                                    # channel: (amplitude, phase)
    x = sum(amp * np.exp(1j * (2 * np.pi * c / Cn * n + ph)) for c, (amp, ph) in tones.items())
    x = (x + 0.25 * (rng.standard_normal(S) + 1j * rng.standard_normal(S))).astype(np.complex64)
    xd = torch.from_numpy(x).cuda()
    y = bank.filter_bank(xd, taps, Cn, D)
    assert y.shape == (Cn, M)
    chans = sorted(tones)
    y64, s = bank_ref.reference(x.astype(np.complex128), taps, Cn, D, channels=chans)
    eps = ((bank_ref.bound_factor(T, Cn) + T + 8) * ddc_ref.U * s).reshape(K, N).max(axis=1)          # per frame
    worst = 0.0
    for row, c in enumerate(chans):
        amp, ph = tones[c]
        assert abs(np.abs(y64[row]).mean() - amp) < 0.1 and abs(np.angle(y64[row].mean()) - ph) < 0.1      # the tone, at 0 Hz
        fa = features18(y[c].view(K, N).contiguous()).cpu().numpy().astype(np.float64)
        one = ddc.tune_decimate(xd, taps, D, shift=Fraction(-c, Cn))
        fb = features18(one.view(K, N).contiguous()).cpu().numpy().astype(np.float64)
        frames = y64[row].reshape(K, N)
        F, scales = orc.features18_batch(frames), orc.conditioning_scales(frames)
        assert np.isfinite(fa).all() and np.isfinite(fb).all() and np.isfinite(F).all()
        for f in range(K):
            k = _feature_moves(frames[f], float(eps[f]))
            tol = 2 * 1e-5 * (np.maximum(np.abs(F[f]), scales[f]) + k) + k
            ratio = np.abs(fa[f] - fb[f]) / tol
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1.0).all(), (c, f, np.argmax(ratio) + 1, fa[f], fb[f], tol)
        # a neighbouring channel holds no tone: its rows are nowhere near
        other = features18(y[c + 1].view(K, N).contiguous()).cpu().numpy()
        assert abs(other[0, 5] - fa[0, 5]) > 0.3                                      # the mean magnitude
    print(f"bank end to end: two tones, {K} frames of {N} per channel: worst |f(bank) - f(ddc)| / bound = {worst:.4f}")
