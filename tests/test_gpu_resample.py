"""The rational resampler (include/amcx.h, amcx_resample; ABI 13) on the GPU.

THE REFERENCE is tests/resample_ref.py: the phase in Python integers, the mixer and the sum in float64, and beside every
output S = sum_q |h[p + q L]| |x[.]|.  THE CRITERION is |y - y64| <= (P + 8) 2^-24 S for EVERY output, P = ceil(T / L) (derived
there); each test prints the worst ratio it saw.  Taps come from +-[0.5, 1] so that every tap counts, phase_step is an odd
64-bit constant.  Everything that the contract calls bit-identical is compared as bytes."""
import json
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _formats, _lib, ddc, resample as rs
from tests import resample_ref as ref, stream_inputs

pytestmark = pytest.mark.gpu

FORMATS = list(ddc.FORMATS)
SHAPES = [(1, 1, 1), (1, 3, 2), (2, 2, 1), (7, 3, 2), (23, 5, 3), (64, 64, 1), (33, 2, 3), (129, 7, 4096), (2561, 160, 147),
          (4096, 256, 255), (4096, 1, 1), (4095, 7, 4096)]
M_EDGES = (1, 63, 64, 65, 255, 256, 257)
STEP = Fraction(ref.ODD_STEP, 1 << 64)
POOL = 160_000                           # samples: the longest parity stream (257 outputs at D / L = 4096 / 7) and some


_torch, _taps_dev = stream_inputs.torch, stream_inputs.taps_dev
_host, _dev, _wide = stream_inputs.bind(57, POOL)


def _run(x, T, L, D, **kw):
    y = rs.resample(x, _taps_dev(T), L, D, **kw)
    _torch().cuda.synchronize()
    return y.cpu().numpy()


def _span(M, T, L, D, tau0):
    """(S, M'): a stream length that gives M outputs, not always the shortest -- or, where interp > decim lets several outputs
    end on one sample and no length gives exactly M, the shortest that gives more -- and the M' >= M it gives"""
    P = ref.phase_taps(T, L)
    shortest, longest = P + ((M - 1) * D + tau0) // L, P + (M * D + tau0) // L - 1
    S = max(shortest, min(shortest + M % 3, longest))
    got = rs.out_samples(S, T, L, D, tau0)
    assert got >= M and (got == M or longest < shortest)
    return S, got


@pytest.mark.parametrize("T,L,D", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_parity(fmt, T, L, D):
    tile, max_span, _, _ = _lib.resample_plan(T, L, D)
    P = ref.phase_taps(T, L)
    Ms = sorted(set(M_EDGES) | {tile, tile + 1})
    worst = 0.0
    for tau0 in sorted({0, L - 1}):
        spans = [_span(M, T, L, D, tau0) for M in Ms]
        y64, s = ref.reference(_wide(fmt), ref.make_taps(T), L, D, tau0, 0, ref.ODD_STEP, M=spans[-1][1])
        longest = None
        for S, M in reversed(spans):
            assert S <= POOL
            y = _run(_dev(fmt)[:S], T, L, D, shift=STEP, phase_index0=tau0)
            assert y.shape == (M,) and y.dtype == np.complex64
            r = ref.worst_ratio(y, y64[:M], s[:M], P)
            worst = max(worst, r)
            assert r <= 1.0, (fmt, T, L, D, tau0, M, r)
            if longest is None:
                longest = y
            assert y.tobytes() == longest[:M].tobytes(), (fmt, T, L, D, tau0, M)   # an output does not depend on the call's length
    print(f"resample parity {fmt} T={T} L={L} D={D} P={P} tile={tile} M={Ms}: worst |err| / bound = {worst:.4f}")


@pytest.mark.parametrize("T,D", [(1, 1), (63, 4), (5, 17), (2048, 1)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_interp_1_is_the_down_converter_bit_for_bit(fmt, T, D):
    S = 40_000 + T
    x = _dev(fmt)[:S]
    want = ddc.tune_decimate(x, _taps_dev(T), D, shift=STEP, sample_index0=77)
    got = rs.resample(x, _taps_dev(T), 1, D, shift=STEP, sample_index0=77)
    _torch().cuda.synchronize()
    assert got.shape == want.shape == (ddc.out_samples(S, T, D),)
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (fmt, T, D)


@pytest.mark.parametrize("T", [23, 3])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_phase_and_tap_pair(fmt, T):
    """phi = 0 and one non-zero sample at a time: every output is exactly fl(h[k] x) for the k the definition gives and exactly
    0 elsewhere -- phases with fewer taps, and (T = 3 < L) phases with none, included."""
    torch = _torch()
    L, D, S = 5, 3, 14
    P = ref.phase_taps(T, L)
    h = ref.make_taps(T)
    M = rs.out_samples(S, T, L, D)
    t = np.arange(M) * D
    p, top = t % L, (P - 1) + t // L
    seen = set()
    for j in range(S):
        if fmt == "cf32":
            x = np.zeros(S, np.complex64)
            x[j] = np.complex64(1.3125 - 0.71875j)
            value = x[j]
        else:
            x = np.full((S, 2), _formats.get(fmt).zero, _formats.get(fmt).plain)
            x[j] = (x[j].astype(np.int64) + np.array([3, -5])).astype(x.dtype)
            value = ref.widen(x, fmt, _formats.get(fmt).scale)[j].astype(np.complex64)
        y = rs.resample(torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda(), L, D).cpu().numpy()
        assert y.shape == (M,)
        k = p + (top - j) * L                                  # the tap that meets sample j in output m, where there is one
        hit = (top - j >= 0) & (k < T)
        hk = np.where(hit, h[np.where(hit, k, 0)], np.float32(0))
        want = (hk * np.float32(value.real)).astype(np.float32) + 1j * (hk * np.float32(value.imag)).astype(np.float32)
        assert np.array_equal(y, want.astype(np.complex64)), (fmt, T, j)
        assert np.all(y[~hit] == 0)
        empty = y[p >= T]                                      # phases with no tap at all: +0 + 0j to the bit, not -0
        assert empty.tobytes() == np.zeros(empty.shape[0], np.complex64).tobytes(), (fmt, T, j)
        seen |= {(int(a), int(b)) for a, b in zip(p[hit], k[hit])}
    # every tap was met, in its own phase, and (T = 3) phases 3 and 4 never gave anything
    assert seen == {(k % L, k) for k in range(T)}
    assert bool((p >= T).any()) == (T < L)                      # (the empty phases were among the outputs where there are any)


@pytest.mark.parametrize("T,L,D", [(23, 5, 3), (2561, 160, 147), (2, 3, 50)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_chunk_invariance(fmt, T, L, D):
    torch = _torch()
    rng = np.random.default_rng(T + L + D)
    S = 12_001
    x = _dev(fmt)[:S]
    whole = _run(x, T, L, D, shift=STEP)
    M = whole.shape[0]
    assert M == rs.out_samples(S, T, L, D) > 0
    # calls cut after random whole numbers of outputs, each told where in the stream it starts and at which phase
    cuts = sorted({0, M} | set(rng.integers(0, M, 9).tolist()))
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        drop, tau0 = divmod(a * D, L)
        part = _run(x[drop:ref.phase_taps(T, L) + ((b - 1) * D) // L], T, L, D, shift=STEP, sample_index0=drop, phase_index0=tau0)
        assert part.shape[0] >= b - a                           # (interp > decim: the last sample may complete further outputs)
        parts.append(part[:b - a])
    assert np.concatenate(parts).tobytes() == whole.tobytes(), (fmt, T, L, D, cuts)
    # the streaming form: single samples, sevens, one long chunk, a random mix with empty chunks
    sizes = [0] + [1] * 300 + [7] * 200 + [4097] + [0]
    r = rs.Resampler(ref.make_taps(T), L, D, STEP, fmt)
    got, pos = [], 0
    while pos < S:
        n = sizes.pop(0) if sizes else int(rng.integers(0, 900))
        got.append(r.push(x[pos:pos + n]))
        pos = min(S, pos + n)
    torch.cuda.synchronize()
    assert torch.cat(got).cpu().numpy().tobytes() == whole.tobytes(), (fmt, T, L, D)
    assert (r.index, r.phase_index) == divmod(M * D, L)


def test_parity_beyond_one_pass_of_the_grid():
    """More tiles than the persistent grid has workgroups: (129, 7, 4096) has tiles of ten outputs."""
    T, L, D, fmt = 129, 7, 4096, "ci8"
    tile, _, grid, _ = _lib.resample_plan(T, L, D)
    S, M = _span(tile * grid + 1, T, L, D, 3)
    assert 2 * S <= 64 << 20 and M > tile * grid
    y = _run(_dev(fmt, S, 1), T, L, D, shift=STEP, phase_index0=3)
    y64, s = ref.reference(_wide(fmt, S, 1), ref.make_taps(T), L, D, 3, 0, ref.ODD_STEP)
    r = ref.worst_ratio(y, y64, s, ref.phase_taps(T, L))
    print(f"resample parity beyond one pass: {M} outputs, {(M + tile - 1) // tile} tiles over {grid} workgroups: worst ratio {r:.4f}")
    assert y.shape == (M,) and r <= 1.0


@pytest.mark.parametrize("fmt", ["cf32", "sc16", "ci8"])
def test_parity_over_three_trips_of_the_grid(fmt):
    """2 grid + 1 tiles and one output more, per loader (each is a kernel with its own copy of the tile loop): (4095, 7, 4096)
    has tiles of nine outputs and the smallest grid.  The criterion for EVERY output."""
    torch = _torch()
    T, L, D, tau0 = 4095, 7, 4096, 3
    tile, _, grid, _ = _lib.resample_plan(T, L, D)
    S, M = _span(tile * (2 * grid + 1) + 1, T, L, D, tau0)
    tiles = -(-M // tile)
    assert tiles >= 2 * grid + 1
    host = stream_inputs.stream(fmt, S, np.random.default_rng(3300 + FORMATS.index(fmt)))
    y = _run(torch.from_numpy(host).cuda(), T, L, D, shift=STEP, phase_index0=tau0)
    y64, s = ref.reference(ref.widen(host, fmt, _formats.get(fmt).scale), ref.make_taps(T), L, D, tau0, 0, ref.ODD_STEP)
    r = ref.worst_ratio(y, y64, s, ref.phase_taps(T, L))
    print(f"resample {fmt} over three trips: {M} outputs, {tiles} tiles of {tile} over {grid} workgroups: worst ratio {r:.4f}")
    assert y.shape == (M,) and r <= 1.0


def test_output_index_times_decim_beyond_32_bits():
    """m D passes 2^32 inside one call: the tiles' first inputs are 64-bit.  The reference of the last outputs is the
    definition's own continuation -- floor(m1 D / L) inputs dropped, tau0' = m1 D mod L, the phase advanced."""
    T, L, D, fmt = 512, 256, 4096, "ci8"
    P = ref.phase_taps(T, L)
    S, M = _span((1 << 32) // D + 700, T, L, D, 0)
    assert (M - 1) * D > 1 << 32 and 2 * S <= 64 << 20
    y = _run(_dev(fmt, S, 2), T, L, D, shift=STEP)
    assert y.shape == (M,)
    host = _host(fmt, S, 2)
    worst = 0.0
    for m1 in (0, (1 << 32) // D - 300, M - 600):
        drop, tau0 = divmod(m1 * D, L)
        xw = ref.widen(host[drop:drop + P + (600 * D + tau0) // L], fmt, _formats.get(fmt).scale)     # all that 600 outputs read
        y64, s = ref.reference(xw, ref.make_taps(T), L, D, tau0, (drop * ref.ODD_STEP) & ref.MASK64, ref.ODD_STEP, M=600)
        worst = max(worst, ref.worst_ratio(y[m1:m1 + 600], y64, s, P))
    print(f"resample beyond 2^32: {M} outputs, m D up to {(M - 1) * D}: worst ratio {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("fmt", FORMATS)
def test_long_streams(fmt):
    T, L, D, S = 23, 5, 3, 5000
    index0 = (1 << 40) + 12345
    phase0 = (index0 * ref.ODD_STEP) & ref.MASK64
    y = _run(_dev(fmt)[:S], T, L, D, shift=STEP, sample_index0=index0, phase_index0=2)
    y64, s = ref.reference(_wide(fmt)[:S], ref.make_taps(T), L, D, 2, phase0, ref.ODD_STEP)
    r = ref.worst_ratio(y, y64, s, ref.phase_taps(T, L))
    print(f"resample long stream {fmt}: sample_index0 = 2^40 + 12345: worst ratio {r:.4f}")
    assert r <= 1.0
    assert y.tobytes() != _run(_dev(fmt)[:S], T, L, D, shift=STEP, phase_index0=2).tobytes()


@pytest.mark.parametrize("fmt,offsets", [("cf32", (8,)), ("sc16", (4, 8, 12)), ("ci8", (2, 6, 14)), ("cu8", (2, 6, 14))])
def test_every_legal_misalignment_reads_the_same_samples(fmt, offsets):
    torch = _torch()
    T, L, D, S = 7, 3, 2, 20_011
    host = np.array(_host(fmt)[:S])
    nbytes = host.nbytes
    aligned = _run(_dev(fmt)[:S], T, L, D, shift=STEP, phase_index0=1)
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
        assert _run(x, T, L, D, shift=STEP, phase_index0=1).tobytes() == aligned.tobytes(), (fmt, off)


@pytest.mark.parametrize("L,D,f", [(3, 2, 0.05), (2, 5, -0.02), (160, 147, 0.11), (1, 4, 0.03)])
def test_rate_sign_and_gain_convention_with_a_tone(L, D, f):
    """Independent of the reference.  A unit tone at f cycles per INPUT sample, through the designer's taps (DC gain L), comes
    out as a tone at f D / L cycles per OUTPUT sample with the input's amplitude within 1 %: consecutive outputs turn by
    exp(2 pi j f D / L) -- the wrong sign, the wrong rate or a missing gain of L is nowhere near -- and mixing by -f leaves
    the constant."""
    torch = _torch()
    h = rs.design_resample_lowpass(L, D)
    S = 6000
    x = torch.from_numpy(np.exp(2j * np.pi * f * np.arange(S)).astype(np.complex64)).cuda()
    y = rs.resample(x, h, L, D).cpu().numpy().astype(np.complex128)
    assert y.shape == (rs.out_samples(S, h.shape[0], L, D),) and y.shape[0] > 1000
    amp = np.abs(y)
    turn = y[1:] / y[:-1]
    want = np.exp(2j * np.pi * f * D / L)
    print(f"resample tone L={L} D={D} f={f}: amplitude {amp.min():.5f} ... {amp.max():.5f}, "
          f"worst |turn - exp(2 pi j f D / L)| = {np.abs(turn - want).max():.2e}")
    assert np.all(np.abs(amp - 1.0) <= 0.01)
    assert np.abs(turn - want).max() <= 0.01 and np.abs(turn - np.conj(want)).min() > 0.05
    dc = rs.resample(x, h, L, D, shift=-f).cpu().numpy().astype(np.complex128)
    assert np.abs(dc - dc[0]).max() <= 0.01 and abs(abs(dc[0]) - 1.0) <= 0.01


@pytest.mark.parametrize("fmt", FORMATS)
def test_bounds(fmt):
    torch = _torch()
    lib = _lib.load()
    T, L, D, G, tau0 = 7, 3, 2, 64, 2
    tile, _, _, _ = _lib.resample_plan(T, L, D)
    for want_m in (1, 257, tile + 1):
        S, M = _span(want_m, T, L, D, tau0)
        x = _dev(fmt)[:S]
        buf = torch.full((G + M + G,), -7.0 + 3.0j, dtype=torch.complex64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def call(cap):
            return lib.amcx_resample(x.data_ptr(), _formats.get(fmt).kind, S, _formats.get(fmt).scale, 0, ref.ODD_STEP,
                                     _taps_dev(T).data_ptr(), T, L, D, tau0, buf.data_ptr() + 8 * G, cap, stream)
        assert call(M - 1) == _lib.EINVAL
        torch.cuda.synchronize()
        assert bool((buf == complex(-7.0, 3.0)).all()), "a refused call wrote"
        assert call(M) == _lib.OK
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:G] == complex(-7.0, 3.0)).all() and (got[G + M:] == complex(-7.0, 3.0)).all(), (fmt, M)
        assert got[G:G + M].tobytes() == _run(x, T, L, D, shift=STEP, phase_index0=tau0).tobytes()
    with pytest.raises(ValueError):
        rs.resample(_dev(fmt)[:100], _taps_dev(T), L, D, out=torch.empty(3, dtype=torch.complex64, device="cuda"))
    out = torch.full((80,), 9.0 + 0j, dtype=torch.complex64, device="cuda")
    y = rs.resample(_dev(fmt)[:30], _taps_dev(T), L, D, out=out)
    assert y.data_ptr() == out.data_ptr() and y.shape == (rs.out_samples(30, T, L, D),) and bool((out[y.shape[0]:] == 9.0).all())


def test_graph_capture():
    torch = _torch()
    lib = _lib.load()
    T, L, D, S, fmt = 23, 5, 3, 30_000, "sc16"
    M = rs.out_samples(S, T, L, D, 4)
    first, second = _dev(fmt)[:S], _dev(fmt)[S:2 * S]
    eager = [_run(first, T, L, D, shift=STEP, phase_index0=4), _run(second, T, L, D, shift=STEP, phase_index0=4)]
    assert eager[0].tobytes() != eager[1].tobytes()
    xin = first.clone()
    out = torch.zeros(M, dtype=torch.complex64, device="cuda")
    taps = _taps_dev(T)

    def launch():
        _lib.check(lib.amcx_resample(xin.data_ptr(), _lib.SRC_SC16, S, _lib.SC16_SCALE, 0, ref.ODD_STEP, taps.data_ptr(),
                                     T, L, D, 4, out.data_ptr(), M, torch.cuda.current_stream().cuda_stream))
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


def test_recording_end_to_end(tmp_path):
    """A ci8 SigMF recording of two captures, each an off-centre QPSK burst whose band is fs / 3.9 wide: the integer path would
    deliver it 3.9 times oversampled (D = 1); extract_sigmf(tune=dict(annotation=0, oversample=2, rational=True)) resamples by
    20 / 39 and equals features18 on resample's materialised output bit for bit, also from the command line."""
    torch = _torch()
    from scipy.io import loadmat
    from amcpy_amd import main as cli
    from amcpy_amd import sigmf
    from amcpy_amd.features import features18
    from amcpy_amd.synth import host_block
    N, R, fs, f_off = 128, 4, 1.0e6, 125_000.0
    rng = np.random.default_rng(6)
    segs = []
    for j, n_sym_samples in enumerate((5 * N + 40, 3 * N + 77)):
        base = np.repeat(host_block("QPSK", 20.0, 1, n_sym_samples, 50 + j)[0].astype(np.complex128), R)
        n = np.arange(base.shape[0])
        wide = 0.5 * base * np.exp(2j * np.pi * f_off / fs * n) + 0.01 * (rng.standard_normal(n.shape) + 1j * rng.standard_normal(n.shape))
        segs.append(np.clip(np.round(np.stack([wide.real, wide.imag], axis=1) * 100.0), -128, 127).astype(np.int8))
    stem = tmp_path / "burst"
    Path(str(stem) + ".sigmf-data").write_bytes(segs[0].tobytes() + b"\xee" * 6 + segs[1].tobytes())
    bw = fs / 3.9
    meta = {"global": {"core:datatype": "ci8", "core:version": "1.0.0", "core:sample_rate": fs},
            "captures": [{"core:sample_start": 0, "core:frequency": 100.0e6},
                         {"core:sample_start": len(segs[0]), "core:header_bytes": 6, "core:frequency": 100.0e6}],
            "annotations": [{"core:sample_start": 10, "core:sample_count": 100, "core:freq_lower_edge": 100.0e6 + f_off - bw / 2,
                             "core:freq_upper_edge": 100.0e6 + f_off + bw / 2}]}
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps(meta))
    assert sigmf.tune_from_annotation(meta, 0, oversample=2)[1] == 1
    shift_hz, (L, D) = sigmf.tune_from_annotation(meta, 0, oversample=2, rational=True)
    assert shift_hz == -f_off and abs(L / D - 2 / 3.9) <= 0.005 * 2 / 3.9
    taps = rs.design_resample_lowpass(L, D)
    want, starts = [], []
    for seg, start in zip(segs, (0, len(segs[0]))):
        y = rs.resample(torch.from_numpy(seg).cuda(), taps, L, D, shift=Fraction(-f_off) / Fraction(fs))
        n = y.shape[0] // N
        want.append(features18(y[:n * N].view(n, N).contiguous()).cpu().numpy())
        starts += [start + k * N * D // L for k in range(n)]
    want = np.concatenate(want)
    assert want.shape[0] == len(starts) >= 6 and np.isfinite(want).all()
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    for tune in ({"annotation": 0, "oversample": 2, "rational": True}, {"shift_hz": -f_off, "resample": (L, D)},
                 {"shift_hz": -f_off, "resample": (L, D), "taps": taps}):
        for chunk in (1 << 24, 1000):
            feats, frame_start = sigmf.extract_sigmf(stem, N, tune=tune, chunk_samples=chunk)
            assert frame_start.tolist() == starts and same(feats, want), (tune.keys(), chunk)
    # the integer path's frames are another oversampling: not the same features
    coarse, _ = sigmf.extract_sigmf(stem, N, tune={"annotation": 0, "oversample": 2})
    assert not same(coarse[:4], want[:4])
    out = tmp_path / "o.mat"
    args = cli.build_parser().parse_args(["recording", str(stem), "--frame-size", str(N), "--annotation", "0", "--rational",
                                          "--out", str(out)])
    got = loadmat(cli.run_recording(args))
    assert got["frame_start"].ravel().tolist() == starts and same(got["features"], want)
    assert int(got["interp"].ravel()[0]) == L and int(got["decim"].ravel()[0]) == D
    args = cli.build_parser().parse_args(["recording", str(stem), "--frame-size", str(N), "--shift-hz", str(-f_off), "--resample",
                                          f"{L}/{D}", "--out", str(out)])
    got = loadmat(cli.run_recording(args))
    assert got["frame_start"].ravel().tolist() == starts and same(got["features"], want)
