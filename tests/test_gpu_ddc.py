"""The digital down-converter (include/amcx.h, amcx_tune_decimate; ABI 11) on the GPU.

THE REFERENCE is tests/ddc_ref.py: the phase in Python integers, the mixer and the sum in float64, and beside every output
S = sum_k |h[k]| |x[.]|.  THE CRITERION is |y - y64| <= (T + 8) 2^-24 S for EVERY output (derived there); each test prints the
worst ratio it saw.  Taps come from +-[0.5, 1] so that every tap counts, phase_step is an odd 64-bit constant.  Everything
that the contract calls bit-identical is compared as bytes."""
import json
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _formats, _lib, ddc
from tests import ddc_ref, stream_inputs

pytestmark = pytest.mark.gpu

FORMATS = list(ddc.FORMATS)
SHAPES = [(1, 1), (2, 1), (7, 3), (5, 17), (63, 4), (64, 64), (129, 4096), (2048, 1), (2048, 4096)]
M_EDGES = (1, 63, 64, 65, 255, 256, 257)
STEP = Fraction(ddc_ref.ODD_STEP, 1 << 64)
POOL = 257 * 4096 + 2048 + 4096          # samples: the longest parity stream and some


_torch, _taps_dev = stream_inputs.torch, stream_inputs.taps_dev
_host, _dev, _wide = stream_inputs.bind(31, POOL)


def _run(x, T, D, **kw):
    y = ddc.tune_decimate(x, _taps_dev(T), D, **kw)
    _torch().cuda.synchronize()
    return y.cpu().numpy()


def _span(M, T, D):
    """a stream length that gives M outputs, not always the shortest"""
    return (M - 1) * D + T + (M % D)


@pytest.mark.parametrize("T,D", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_parity(fmt, T, D):
    tile, _ = _lib.tune_decimate_plan(T, D)
    Ms = sorted({m for m in M_EDGES + (tile - 1, tile, tile + 1) if m >= 1})
    y64, s = ddc_ref.reference(_wide(fmt), ddc_ref.make_taps(T), D, 0, ddc_ref.ODD_STEP, M=Ms[-1])
    worst, longest = 0.0, None
    for M in reversed(Ms):
        S = _span(M, T, D)
        assert ddc.out_samples(S, T, D) == M and S <= POOL
        y = _run(_dev(fmt)[:S], T, D, shift=STEP)
        assert y.shape == (M,) and y.dtype == np.complex64
        r = ddc_ref.worst_ratio(y, y64[:M], s[:M], T)
        worst = max(worst, r)
        assert r <= 1.0, (fmt, T, D, M, r)
        if longest is None:
            longest = y
        assert y.tobytes() == longest[:M].tobytes(), (fmt, T, D, M)           # an output does not depend on the call's length
    print(f"ddc parity {fmt} T={T} D={D} tile={tile} M={Ms}: worst |err| / bound = {worst:.4f}")


def test_parity_beyond_one_pass_of_the_grid():
    """More tiles than the persistent grid has workgroups: (129, 4096) has tiles of two outputs."""
    T, D, fmt = 129, 4096, "ci8"
    tile, grid = _lib.tune_decimate_plan(T, D)
    M = tile * grid + 1
    S = (M - 1) * D + T
    assert 2 * S <= 32 << 20 and M > tile * grid
    y = _run(_dev(fmt, S, 1), T, D, shift=STEP)
    y64, s = ddc_ref.reference(_wide(fmt, S, 1), ddc_ref.make_taps(T), D, 0, ddc_ref.ODD_STEP)
    r = ddc_ref.worst_ratio(y, y64, s, T)
    print(f"ddc parity beyond one pass: {M} outputs, {(M + tile - 1) // tile} tiles over {grid} workgroups: worst ratio {r:.4f}")
    assert y.shape == (M,) and r <= 1.0


@pytest.mark.parametrize("fmt", ["cf32", "sc16", "ci8"])
def test_parity_over_three_trips_of_the_grid(fmt):
    """2 grid + 1 tiles and one output more, per loader (each is a kernel with its own copy of the tile loop): (2048, 4096)
    has tiles of two outputs and the smallest grid.  The criterion for EVERY output, and the bytes of the same outputs made in
    calls of at most one trip (the stream from output m0 on, its first sample's index m0 D)."""
    torch = _torch()
    T, D = 2048, 4096
    tile, grid = _lib.tune_decimate_plan(T, D)
    M = tile * (2 * grid + 1) + 1
    tiles = -(-M // tile)
    S = (M - 1) * D + T
    assert tiles >= 2 * grid + 1 and ddc.out_samples(S, T, D) == M
    host = stream_inputs.stream(fmt, S, np.random.default_rng(3100 + FORMATS.index(fmt)))
    x = torch.from_numpy(host).cuda()
    y = _run(x, T, D, shift=STEP)
    y64, s = ddc_ref.reference(ddc_ref.widen(host, fmt, _formats.get(fmt).scale), ddc_ref.make_taps(T), D, 0, ddc_ref.ODD_STEP)
    r = ddc_ref.worst_ratio(y, y64, s, T)
    print(f"ddc {fmt} over three trips: {M} outputs, {tiles} tiles of {tile} over {grid} workgroups: worst ratio {r:.4f}")
    assert y.shape == (M,) and r <= 1.0
    per = tile * grid
    parts = [ddc.tune_decimate(x[m0 * D:(min(m0 + per, M) - 1) * D + T], _taps_dev(T), D, shift=STEP, sample_index0=m0 * D)
             for m0 in range(0, M, per)]
    torch.cuda.synchronize()
    assert all(p.shape[0] <= per for p in parts) and torch.cat(parts).cpu().numpy().tobytes() == y.tobytes()


@pytest.mark.parametrize("fmt", FORMATS)
def test_zero_phase_one_tap_is_the_widened_input(fmt):
    torch = _torch()
    S = 70_001
    x = np.array(_host(fmt)[:S])
    if fmt == "cf32":
        x[:6] = np.array([complex(-0.0, 1.0), complex(1.0, -0.0), complex(-0.0, -0.0), complex(0.0, -3.0), 1e-42 - 1e-40j,
                          complex(np.inf, -1.0)], dtype=np.complex64)
        want = x
    else:
        x[:4] = np.array([[0, 0], [np.iinfo(x.dtype).min, np.iinfo(x.dtype).max], [0, 1], [1, 0]], dtype=np.int64).astype(x.dtype)
        want = ddc_ref.widen(x, fmt, _formats.get(fmt).scale).astype(np.complex64)
    for off in (0, 1):                                       # 16-byte aligned and not (for 8-bit samples: 2 mod 16)
        y = ddc.tune_decimate(torch.from_numpy(x).cuda()[off:], torch.ones(1, device="cuda"), 1)
        torch.cuda.synchronize()
        assert y.cpu().numpy().tobytes() == want[off:].tobytes(), (fmt, off)
    # ... and for every phi below 2^32, whose top 32 bits are 0: the mixer is exactly 1 + 0j there
    y = ddc.tune_decimate(torch.from_numpy(x).cuda(), torch.ones(1, device="cuda"), 1, shift=Fraction(3, 1 << 64), sample_index0=5)
    assert y.cpu().numpy().tobytes() == want.tobytes()


def test_the_mixer_on_its_own():
    """x = 1 + 0j, one tap of 1.0, D = 1: y[n] is ddc_mixer(p) itself (fma(1, w, -+0) is exact), and with shift = s / 2^32 the
    angle is p = ((sample_index0 + n) s) mod 2^32.  Walked: every octant boundary k 2^29 +- 2^16, where the quarter turn q and
    the remainder r of the reduction change (k = 0 wraps the phase accumulator through 0); 2^20 angles at the odd stride 4099;
    the angle 0xDD9F6111 and its seven images under the octant symmetries.

    THE BOUND is the mixer's own share of tests/ddc_ref.py's derivation: |w - exp(2 pi j p / 2^32)| <= 2.5 x 2^-24 (the angle's
    fp32 rounding and the two polynomials).  The same operation sequence in C on the CPU (fmaf, no contraction) over all 2^32
    angles: worst 2.458 x 2^-24, at p = 0xDD9F6111 (w = 0x3F2A2797, 0xBF3F4492) and its images -- inside, by 1.7 %.
    Exactly (1, 0), (0, 1), (-1, 0), (0, -1) at the multiples of 2^30; w(p + 2^30) = (-w.y, w.x) bit for bit (the quarter turns
    are swaps and sign changes); p = 0 returns x untouched."""
    torch = _torch()
    one = torch.ones(1, device="cuda")

    def walk(first, n, stride=1):
        """(p (n,) uint64, y (n,) complex64): the mixer at p = (first + i stride) mod 2^32"""
        index0 = (first * pow(stride, -1, 1 << 32)) % (1 << 32)
        y = ddc.tune_decimate(torch.ones(n, dtype=torch.complex64, device="cuda"), one, 1, shift=Fraction(stride, 1 << 32),
                              sample_index0=index0)
        torch.cuda.synchronize()
        return (first + np.arange(n, dtype=np.uint64) * np.uint64(stride)) % np.uint64(1 << 32), y.cpu().numpy()

    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    corner = 0xDD9F6111
    images = sorted({(sign * corner + k * (1 << 30)) % (1 << 32) for sign in (1, -1) for k in range(4)})
    assert len(images) == 8 and len({p >> 29 for p in images}) == 8                  # one in every octant
    runs = [((k << 29) - (1 << 16), (1 << 17) + 1, 1) for k in range(8)] + [(0, 1 << 20, 4099)] + [(p, 1, 1) for p in images]
    worst, worst_at, worst_bits, turns = 0.0, None, None, 0
    for first, n, stride in runs:
        p, y = walk(first % (1 << 32), n, stride)
        assert y.shape == (n,) and y.dtype == np.complex64
        err = np.abs(y.astype(np.complex128) - np.exp(2j * np.pi * (p.astype(np.float64) / 4294967296.0))) / ddc_ref.U
        i = int(np.argmax(err))
        if err[i] > worst:
            worst, worst_at, worst_bits = float(err[i]), int(p[i]), (int(bits(y.real)[i]), int(bits(y.imag)[i]))
        assert err[i] <= 2.5, (hex(int(p[i])), float(err[i]), hex(int(bits(y.real)[i])), hex(int(bits(y.imag)[i])))
        for q, (re, im) in enumerate(((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))):
            at = p == np.uint64(q << 30)
            turns += int(at.sum())
            assert (y.real[at] == re).all() and (y.imag[at] == im).all(), (q, y[at])
        assert y[p == 0].tobytes() == np.ones(int((p == 0).sum()), np.complex64).tobytes()     # x untouched, +0 included
        p4, y4 = walk((first + (1 << 30)) % (1 << 32), n, stride)
        assert np.array_equal(p4, (p + np.uint64(1 << 30)) % np.uint64(1 << 32))
        assert np.array_equal(bits(y4.real), bits(-y.imag)) and np.array_equal(bits(y4.imag), bits(y.real)), (hex(first), stride)
    assert turns >= 4 and worst_at is not None
    print(f"ddc mixer alone: {sum(n for _, n, _ in runs)} angles: worst |w - exp| = {worst:.4f} x 2^-24 at p = {worst_at:#010x} "
          f"(w = {worst_bits[0]:#010x}, {worst_bits[1]:#010x}); {turns} exact quarter turns")


@pytest.mark.parametrize("T,D", [(63, 4), (5, 17), (2048, 1)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_chunk_invariance(fmt, T, D):
    torch = _torch()
    rng = np.random.default_rng(T + D)
    S = 2500 * D + T + 3
    x = _dev(fmt)[:S]
    whole = _run(x, T, D, shift=STEP)
    M = whole.shape[0]
    # calls cut at random multiples of D, each told where in the stream it starts
    cuts = sorted({0, M} | set(rng.integers(0, M, 9).tolist()))
    parts = [_run(x[a * D:(b - 1) * D + T], T, D, shift=STEP, sample_index0=a * D) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.concatenate(parts).tobytes() == whole.tobytes(), (fmt, T, D, cuts)
    # the streaming form, cut anywhere: empty chunks, single samples, chunks below T
    chan = ddc.Channelizer(ddc_ref.make_taps(T), D, STEP, fmt)
    got, pos = [], 0
    for n in [0, 1, max(T - 1, 1), 0] + rng.integers(1, S // 4, 30).tolist():
        got.append(chan.push(x[pos:pos + n]))
        pos = min(S, pos + n)
    assert pos == S
    torch.cuda.synchronize()
    assert torch.cat(got).cpu().numpy().tobytes() == whole.tobytes(), (fmt, T, D)


@pytest.mark.parametrize("fmt,offsets", [("cf32", (8,)), ("sc16", (4, 8, 12)), ("ci8", (2, 6, 14)), ("cu8", (2, 6, 14))])
def test_every_legal_misalignment_reads_the_same_samples(fmt, offsets):
    torch = _torch()
    T, D, S = 7, 3, 20_011
    host = np.array(_host(fmt)[:S])
    nbytes = host.nbytes
    aligned = _run(_dev(fmt)[:S], T, D, shift=STEP)
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
        assert _run(x, T, D, shift=STEP).tobytes() == aligned.tobytes(), (fmt, off)


def test_sign_and_index_convention_with_a_pure_tone():
    """Independent of the reference.  A tone at +1/4 cycle per sample is 1, j, -1, -j: exact in complex64, and the mixer's
    quarter turns are exact, so shift = -1/4 gives v = 1 exactly and every output is the taps' own fp32 sum -- the DC gain, 1
    within the criterion (S = sum |h|).  shift = +1/4 leaves a tone at the half rate, which the low-pass removes.  A second
    tone at 3/32 is not exact in complex64: each sample is off by at most sqrt(2) 2^-25 < 2^-24 of its magnitude 1, which
    adds 2^-24 sum |h| to the bound."""
    torch = _torch()
    D = 4
    h = ddc.design_lowpass(D)
    T, S = h.shape[0], 4096 + h.shape[0]
    sabs = float(np.abs(h.astype(np.float64)).sum())
    dc = float(h.astype(np.float64).sum())
    n = np.arange(S)
    for f, extra in ((Fraction(1, 4), 0.0), (Fraction(3, 32), 1.0)):
        tone = np.exp(2j * np.pi * float(f) * n)
        if f == Fraction(1, 4):
            tone = np.array([1, 1j, -1, -1j], dtype=np.complex128)[n % 4]
        x = torch.from_numpy(tone.astype(np.complex64)).cuda()
        down = ddc.tune_decimate(x, h, D, shift=-f).cpu().numpy().astype(np.complex128)
        bound = (T + 8 + extra) * ddc_ref.U * sabs
        worst = float(np.abs(down - dc).max())
        print(f"ddc tone f={f}: worst |y - DC gain| / bound = {worst / bound:.4f}")
        assert down.shape == ((S - T) // D + 1,) and worst <= bound, (f, worst, bound)
        up = ddc.tune_decimate(x, h, D, shift=f).cpu().numpy().astype(np.complex128)
        assert float(np.abs(up - dc).min()) > 0.9, f                      # the wrong sign is nowhere near
        # one sample late or early is a different phase of the tone, not the constant
        late = ddc.tune_decimate(x, h, D, shift=-f, sample_index0=1).cpu().numpy().astype(np.complex128)
        assert float(np.abs(late - dc * np.exp(-2j * np.pi * float(f))).max()) <= bound and float(np.abs(late - dc).min()) > 0.5


@pytest.mark.parametrize("fmt", FORMATS)
def test_long_streams(fmt):
    T, D, S = 63, 4, 5000
    index0 = (1 << 40) + 12345
    phase0 = (index0 * ddc_ref.ODD_STEP) & ddc_ref.MASK64
    y = _run(_dev(fmt)[:S], T, D, shift=STEP, sample_index0=index0)
    y64, s = ddc_ref.reference(_wide(fmt)[:S], ddc_ref.make_taps(T), D, phase0, ddc_ref.ODD_STEP)
    r = ddc_ref.worst_ratio(y, y64, s, T)
    print(f"ddc long stream {fmt}: sample_index0 = 2^40 + 12345: worst ratio {r:.4f}")
    assert r <= 1.0
    assert y.tobytes() != _run(_dev(fmt)[:S], T, D, shift=STEP).tobytes()


@pytest.mark.parametrize("fmt", FORMATS)
def test_bounds(fmt):
    torch = _torch()
    lib = _lib.load()
    T, D, G = 7, 3, 64
    tile, _ = _lib.tune_decimate_plan(T, D)
    for M in (1, 257, tile + 1):
        S = _span(M, T, D)
        x = _dev(fmt)[:S]
        buf = torch.full((G + M + G,), -7.0 + 3.0j, dtype=torch.complex64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def call(cap):
            return lib.amcx_tune_decimate(x.data_ptr(), _formats.get(fmt).kind, S, _formats.get(fmt).scale, 0, ddc_ref.ODD_STEP,
                                          _taps_dev(T).data_ptr(), T, D, buf.data_ptr() + 8 * G, cap, stream)
        assert call(M - 1) == _lib.EINVAL
        torch.cuda.synchronize()
        assert bool((buf == complex(-7.0, 3.0)).all()), "a refused call wrote"
        assert call(M) == _lib.OK
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:G] == complex(-7.0, 3.0)).all() and (got[G + M:] == complex(-7.0, 3.0)).all(), (fmt, M)
        assert got[G:G + M].tobytes() == _run(x, T, D, shift=STEP).tobytes()


def test_graph_capture():
    torch = _torch()
    lib = _lib.load()
    T, D, S, fmt = 63, 4, 30_000, "sc16"
    M = ddc.out_samples(S, T, D)
    first, second = _dev(fmt)[:S], _dev(fmt)[S:2 * S]
    eager = [_run(first, T, D, shift=STEP), _run(second, T, D, shift=STEP)]
    assert eager[0].tobytes() != eager[1].tobytes()
    xin = first.clone()
    out = torch.zeros(M, dtype=torch.complex64, device="cuda")
    taps = _taps_dev(T)

    def launch():
        _lib.check(lib.amcx_tune_decimate(xin.data_ptr(), _lib.SRC_SC16, S, _lib.SC16_SCALE, 0, ddc_ref.ODD_STEP, taps.data_ptr(),
                                          T, D, out.data_ptr(), M, torch.cuda.current_stream().cuda_stream))
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
    """A ci8 SigMF recording of two captures, each an off-centre QPSK burst four times oversampled: extract_sigmf(tune=)
    equals features18 on tune_decimate's materialised output bit for bit, by either form of `tune` and from the command
    line."""
    torch = _torch()
    from scipy.io import loadmat
    from amcpy_amd import main as cli
    from amcpy_amd import sigmf
    from amcpy_amd.features import features18
    from amcpy_amd.synth import host_block
    N, R, fs, f_off = 128, 4, 1.0e6, 125_000.0
    rng = np.random.default_rng(5)
    segs = []
    for j, n_sym_samples in enumerate((5 * N + 40, 3 * N + 77)):
        base = np.repeat(host_block("QPSK", 20.0, 1, n_sym_samples, 40 + j)[0].astype(np.complex128), R)
        n = np.arange(base.shape[0])
        wide = 0.5 * base * np.exp(2j * np.pi * f_off / fs * n) + 0.01 * (rng.standard_normal(n.shape) + 1j * rng.standard_normal(n.shape))
        q = np.clip(np.round(np.stack([wide.real, wide.imag], axis=1) * 100.0), -128, 127).astype(np.int8)
        segs.append(q)
    stem = tmp_path / "burst"
    Path(str(stem) + ".sigmf-data").write_bytes(segs[0].tobytes() + b"\xee" * 6 + segs[1].tobytes())
    bw = fs / R
    meta = {"global": {"core:datatype": "ci8", "core:version": "1.0.0", "core:sample_rate": fs},
            "captures": [{"core:sample_start": 0, "core:frequency": 100.0e6},
                         {"core:sample_start": len(segs[0]), "core:header_bytes": 6, "core:frequency": 100.0e6}],
            "annotations": [{"core:sample_start": 10, "core:sample_count": 100, "core:freq_lower_edge": 100.0e6 + f_off - bw / 2,
                             "core:freq_upper_edge": 100.0e6 + f_off + bw / 2}]}
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps(meta))
    assert sigmf.tune_from_annotation(meta, 0, oversample=2) == (-f_off, 2)
    D = 2
    taps = ddc.design_lowpass(D)
    want, starts = [], []
    for seg, start in zip(segs, (0, len(segs[0]))):
        y = ddc.tune_decimate(torch.from_numpy(seg).cuda(), taps, D, shift=Fraction(-f_off) / Fraction(fs))
        n = y.shape[0] // N
        want.append(features18(y[:n * N].view(n, N).contiguous()).cpu().numpy())
        starts += [start + k * N * D for k in range(n)]
    want = np.concatenate(want)
    assert want.shape[0] == len(starts) >= 6 and np.isfinite(want).all()
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    for tune in ({"shift_hz": -f_off, "decimate": D}, {"annotation": 0, "oversample": 2}, {"shift_hz": -f_off, "decimate": D, "taps": taps}):
        for chunk in (1 << 24, 1000):
            feats, frame_start = sigmf.extract_sigmf(stem, N, tune=tune, chunk_samples=chunk)
            assert frame_start.tolist() == starts and same(feats, want), (tune.keys(), chunk)
    feats, frame_start = sigmf.extract_sigmf(stem, N, tune={"annotation": 0}, feature_ids=[3, 13], max_frames=4)
    assert frame_start.tolist() == starts[:4] and same(feats[:, [2, 12]], want[:4][:, [2, 12]]) and np.isnan(feats[:, 0]).all()
    # the tuned burst is a usable frame: the untuned one is not the same thing
    untuned, _ = sigmf.extract_sigmf(stem, N)
    assert not same(untuned[:len(starts)], want)
    out = tmp_path / "o.mat"
    args = cli.build_parser().parse_args(["recording", str(stem), "--frame-size", str(N), "--shift-hz", str(-f_off), "--decimate",
                                          str(D), "--out", str(out)])
    got = loadmat(cli.run_recording(args))
    assert got["frame_start"].ravel().tolist() == starts and same(got["features"], want)
    args = cli.build_parser().parse_args(["recording", str(stem), "--frame-size", str(N), "--annotation", "0", "--out", str(out)])
    got = loadmat(cli.run_recording(args))
    assert got["frame_start"].ravel().tolist() == starts and same(got["features"], want)
