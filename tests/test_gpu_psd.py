"""The Welch spectrogram and its detection (include/amcx.h, ABI 15) on the GPU.

THE ERROR CRITERION is |P - P64| <= bound for EVERY cell (tests/psd_ref.py derives the bound from the kernel's operation
sequence); the test prints the worst fraction of the bound it saw per nfft.  Everything the contract calls bit-identical --
the float32 restatement, positions, strides, chunking, formats, the detection -- is compared with `==`."""
import numpy as np
import pytest

from amcpy_amd import _lib, occupancy, psd
from tests import ddc_ref, psd_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [64, 128, 256, 512, 1024, 2048, 4096]
SENTINEL = -7.0
INT_FORMATS = ("sc16", "ci8", "cu8")


def _torch():
    import torch
    return torch


def _hops(nfft):
    return (1, nfft // 2, nfft, nfft + 3)


def _samples_for(R, nfft, hop, A, ragged=True):
    """S such that exactly R rows fit, plus a tail that fills neither a segment nor a row."""
    S = (R * A - 1) * hop + nfft
    if ragged:
        S += min(hop, nfft) - 1 if A == 1 else hop + min(hop, nfft) // 2     # A > 1: one more segment, not a row
    assert ref.out_rows(S, nfft, hop, A) == R
    return S


def _noise(S, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(S) + 1j * rng.standard_normal(S)).astype(np.complex64)


def _raw(S, fmt, seed):
    """Stored samples of an integer format, (S, 2), over the format's whole range."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(ref.FORMATS[fmt])
    return rng.integers(info.min, info.max + 1, (S, 2)).astype(ref.FORMATS[fmt])


def _run(x, nfft, **kw):
    t = _torch()
    P = psd.spectrogram(t.from_numpy(np.ascontiguousarray(x)).cuda(), nfft, **kw)
    t.cuda.synchronize()
    return P.cpu().numpy()


@pytest.mark.parametrize("nfft", SIZES)
def test_error_bound_on_bins_three_decades_apart(nfft):
    worst = 0.0
    for kind in ("hann", "rect"):
        w = psd.window(nfft, kind)
        for hop in _hops(nfft):
            for A in (1, 3):
                S = _samples_for(3, nfft, hop, A)
                x = ref.spread_signal(S, nfft, 7 * nfft + hop + A)
                P = _run(x, nfft, hop=hop, averages=A, window=w)
                assert P.shape == (3, nfft) and P.dtype == np.float32
                frac = ref.worst_fraction(P, x, w, nfft, hop, A)
                worst = max(worst, frac)
                assert frac <= 1.0, (nfft, kind, hop, A, frac)
    print(f"spectrogram nfft={nfft}: worst |err| / bound = {worst:.5f}")


@pytest.mark.parametrize("nfft", [64, 256, 4096])
def test_rows_equal_the_float32_restatement(nfft):
    w = psd.window(nfft, "hann")
    for hop, A in ((nfft // 2, 3), (nfft + 3, 1), (1, 3)):
        S = _samples_for(3, nfft, hop, A)
        x = ref.spread_signal(S, nfft, nfft + hop)
        assert np.array_equal(_run(x, nfft, hop=hop, averages=A, window=w), ref.float32_rows(x, w, nfft, hop, A)), (nfft, hop, A)


def test_more_and_fewer_rows_than_segments_per_pass():
    """nfft = 64 holds 64 rows' segments per pass: one row leaves 63 slots idle, 130 rows need three passes; 4096 holds one."""
    for nfft, R in ((64, 1), (64, 130), (1024, 2), (1024, 9), (4096, 3)):
        assert _lib.spectrogram_plan(nfft, nfft // 2, 2)[0] == 4096 // nfft
        w = psd.window(nfft, "hann")
        x = _noise(_samples_for(R, nfft, nfft // 2, 2), nfft + R)
        P = _run(x, nfft, averages=2, window=w)
        assert P.shape == (R, nfft)
        if nfft == 64:
            assert np.array_equal(P, ref.float32_rows(x, w, nfft, nfft // 2, 2))
        assert ref.worst_fraction(P, x, w, nfft, nfft // 2, 2) <= 1.0


@pytest.mark.parametrize("nfft", SIZES)
def test_exact_cases(nfft):
    rect = psd.window(nfft, "rect")
    for A in (1, 3):
        S = _samples_for(3, nfft, nfft, A)
        # an impulse at n = 0 of every segment: every bin of every transform is 1
        x = np.zeros(S, np.complex64)
        x[::nfft] = 1.0
        assert np.array_equal(_run(x, nfft, hop=nfft, averages=A, window=rect), np.full((3, nfft), float(A), np.float32))
        # a constant integer: A (nfft c)^2 in bin 0, exactly 0 elsewhere
        c = max(1, int(np.sqrt((1 << 24) / A)) // nfft)
        want = np.zeros((3, nfft), np.float64)
        want[:, 0] = A * (nfft * c) ** 2
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)          # float32 holds it exactly
        for hop in _hops(nfft):
            x = np.full(_samples_for(3, nfft, hop, A), c, np.complex64)
            assert np.array_equal(_run(x, nfft, hop=hop, averages=A, window=rect).astype(np.float64), want), (nfft, A, hop)
        # a tone at a quarter of the sample rate, sampled at quarter turns: bin nfft / 4 and only there
        x = np.array([1, 1j, -1, -1j], np.complex64)[np.arange(S) % 4]
        want = np.zeros((3, nfft), np.float64)
        want[:, nfft // 4] = A * nfft ** 2
        assert np.array_equal(_run(x, nfft, hop=nfft, averages=A, window=rect).astype(np.float64), want), (nfft, A)


@pytest.mark.parametrize("nfft", [64, 512, 4096])
def test_formats_are_the_complex64_bits_at_every_16_byte_phase(nfft):
    """The same span at sample offsets 0, 1, 2, 3 and 5 of its buffer (every 16-byte phase of 8-, 4- and 2-byte samples), in
    every format: all rows `==`, and the integer formats' rows `==` the complex64 rows of the widened samples."""
    t = _torch()
    w = psd.window(nfft, "hann")
    for hop, A in ((nfft // 2, 3), (nfft + 3, 1)):
        S = _samples_for(3, nfft, hop, A)
        for fmt in ("cf32",) + INT_FORMATS:
            raw = _noise(S, nfft + hop) if fmt == "cf32" else _raw(S, fmt, nfft + hop)
            scale = None if fmt == "cf32" else ref.DEFAULT_SCALE[fmt] * 1.25
            wide = ddc_ref.widen(raw, fmt, scale).astype(np.complex64)
            base = _run(wide, nfft, hop=hop, averages=A, window=w)
            assert ref.worst_fraction(base, wide, w, nfft, hop, A) <= 1.0
            for off in (0, 1, 2, 3, 5):
                buf = t.zeros((S + 8,) + raw.shape[1:], dtype=t.from_numpy(raw[:1]).dtype, device="cuda")
                buf[off:off + S].copy_(t.from_numpy(raw).cuda())
                got = psd.spectrogram(buf[off:off + S], nfft, hop=hop, averages=A, window=w, scale=scale)
                t.cuda.synchronize()
                assert np.array_equal(got.cpu().numpy(), base), (nfft, hop, A, fmt, off)


@pytest.mark.parametrize("nfft", [64, 1024, 4096])
def test_row_index_stride_and_padding(nfft):
    t = _torch()
    w = psd.window(nfft, "hann")
    hop, A = nfft // 2, 3
    x = _noise(_samples_for(5, nfft, hop, A), nfft)
    base = _run(x, nfft, hop=hop, averages=A, window=w)
    xd = t.from_numpy(x).cuda()
    for pad, first in ((5, 0), (1, 2), (64, 1)):
        out = t.full((5 + first + 1, nfft + pad), SENTINEL, dtype=t.float32, device="cuda")
        got = psd.spectrogram(xd, nfft, hop=hop, averages=A, window=w, out=out[first:])
        t.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(got.cpu().numpy(), base) and np.array_equal(o[first:first + 5, :nfft], base)
        assert np.all(o[:, nfft:] == SENTINEL) and np.all(o[:first] == SENTINEL) and np.all(o[first + 5:] == SENTINEL)
    # a row's bits do not depend on its index: the stream from row 2 on gives the rows 2 ...
    step = A * hop
    assert np.array_equal(_run(x[2 * step:], nfft, hop=hop, averages=A, window=w), base[2:])


@pytest.mark.parametrize("nfft", [64, 256, 4096])
def test_chunking_is_bit_identical(nfft):
    t = _torch()
    w = psd.window(nfft, "hann")
    for hop, A in ((nfft // 2, 3), (nfft + 3, 2)):
        R = 4
        x = _noise(_samples_for(R, nfft, hop, A), nfft + hop)
        base = _run(x, nfft, hop=hop, averages=A, window=w)
        step, span = A * hop, psd.row_samples(nfft, hop, A)
        for r in range(R):                                                   # the call cut after every whole row
            assert np.array_equal(_run(x[r * step:r * step + span], nfft, hop=hop, averages=A, window=w), base[r:r + 1])
        assert np.array_equal(_run(x[step:3 * step + span - step], nfft, hop=hop, averages=A, window=w), base[1:3])
        xd = t.from_numpy(x).cuda()
        for cut in ((1, 7, span - 1) if nfft == 64 else (span - 1, 997)):
            sp = psd.Spectrogram(nfft, hop, A, w)
            rows = [sp.push(xd[i:i + cut]) for i in range(0, len(x), cut)]
            t.cuda.synchronize()
            assert np.array_equal(t.cat(rows).cpu().numpy(), base), (nfft, hop, A, cut)
            assert sp.rows_done == R and sp.index == R * step and sp.held == max(0, len(x) - R * step)


def _detect_rows(R, bins, seed):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((R, bins)) ** 2).astype(np.float32)
    p[1] = rng.integers(0, 3, bins)                                         # ties
    p[2] = 5.0                                                              # all equal
    p[3, rng.integers(0, bins, max(1, bins // 8))] = np.nan
    p[4, rng.integers(0, bins, max(1, bins // 8))] = np.inf
    p[5] = np.nan
    p[6, 0] = np.nan
    p[6, -1] = np.inf
    return p


@pytest.mark.parametrize("bins", [2, 3, 63, 64, 65, 1000, 4096])
def test_detect_equals_numpy(bins):
    t = _torch()
    lib = _lib.load()
    R = 9
    p = _detect_rows(R, bins, bins)
    for stride in (bins, bins + 3):
        pd = t.full((R, stride), SENTINEL, dtype=t.float32, device="cuda")
        pd[:, :bins].copy_(t.from_numpy(p).cuda())
        for rank in sorted({0, bins // 2, bins - 1}):
            for thr in (np.float32(1.0), occupancy.threshold_of(6.0)):
                floor = t.full((R + 1,), SENTINEL, dtype=t.float32, device="cuda")
                mask = t.full((R * bins + 1,), 9, dtype=t.uint8, device="cuda")
                _lib.check(lib.amcx_psd_detect_f32(pd.data_ptr(), R, bins, stride, rank, float(thr), floor.data_ptr(),
                                                   mask.data_ptr(), t.cuda.current_stream().cuda_stream))
                t.cuda.synchronize()
                f, m = ref.numpy_psd_detect(p, rank, thr)
                assert np.array_equal(floor.cpu().numpy()[:R], f, equal_nan=True), (bins, stride, rank, thr)
                assert np.array_equal(mask.cpu().numpy()[:R * bins].reshape(R, bins).astype(bool), m), (bins, stride, rank, thr)
                assert floor.cpu().numpy()[R] == SENTINEL and mask.cpu().numpy()[R * bins] == 9
    # the Python layer: quantile and decibels through occupancy's rank and threshold
    det = psd.detect(pd[:, :bins], floor_quantile=0.25, threshold_db=6.0)
    f, m = ref.numpy_psd_detect(p, occupancy.floor_rank_of(bins, 0.25), occupancy.threshold_of(6.0))
    assert np.array_equal(det.floor.cpu().numpy(), f, equal_nan=True) and np.array_equal(det.mask.cpu().numpy(), m)
    assert det.snr_db.shape == (R, bins)


@pytest.mark.parametrize("datatype", ["cf32_le", "ci8"])
def test_scan_end_to_end(datatype, tmp_path):
    """The synthetic recording of tests/psd_ref.py (checked against the float64 reference alone in tests/test_psd_host.py)
    through scan_sigmf on the device, the `scan` command's annotations, and extract_sigmf tuned to every one of them."""
    import json
    from pathlib import Path
    from amcpy_amd import main as cli, sigmf
    nfft, A, S = 256, 16, 1 << 18
    hop, half = nfft // 2, S // 2
    stem, held = ref.write_recording(tmp_path, ref.synthetic_recording(S, 0), datatype)
    want = sigmf.scan_sigmf(stem, nfft=nfft, averages=A, detect={}, psd_compute=ref.numpy_psd, detect_compute=ref.numpy_psd_detect)
    got = sigmf.scan_sigmf(stem, nfft=nfft, averages=A, detect={}, chunk_samples=50000)
    assert set(got) == set(want) and np.array_equal(got["row_start"], want["row_start"]) and got["psd"].shape == want["psd"].shape
    w = psd.window(nfft)
    rank, thr = occupancy.floor_rank_of(nfft, 0.25), occupancy.threshold_of(6.0)
    per = ref.out_rows(half, nfft, hop, A)
    near = 0
    for cap in (0, 1):
        x, rows = held[cap * half:(cap + 1) * half], slice(cap * per, (cap + 1) * per)
        frac = ref.worst_fraction(got["psd"][rows], x, w, nfft, hop, A)
        print(f"scan {datatype} capture {cap}: worst |err| / bound = {frac:.5f}")
        assert frac <= 1.0
        P64 = ref.reference(x, w, nfft, hop, A)
        margin = P64 / (float(thr) * np.sort(P64, axis=1)[:, rank][:, None])
        close = np.abs(margin - 1.0) < 1e-4
        near += int(close.sum())
        assert np.array_equal(got["occupied"][rows][~close], (margin > 1.0)[~close])
    assert near <= 0.001 * got["occupied"].size
    assert len(got["emitters"]) == len(want["emitters"]) == 5
    for e, t in zip(got["emitters"], want["emitters"]):
        assert {k: e[k] for k in e if k != "snr_db"} == {k: t[k] for k in t if k != "snr_db"}
        assert abs(e["snr_db"] - t["snr_db"]) < 0.01
    # the command on the device, its annotations, and the tuned extraction of every one of them
    noted = tmp_path / "noted.sigmf-meta"
    cli.run_scan(cli.build_parser().parse_args(["scan", str(stem), "--nfft", str(nfft), "--averages", str(A), "--annotate", str(noted),
                                                "--out", str(tmp_path / "s.mat")]))
    Path(str(tmp_path / "noted") + ".sigmf-data").write_bytes(Path(str(stem) + ".sigmf-data").read_bytes())
    anns = json.loads(noted.read_text())["annotations"]
    assert len(anns) == 6
    for k, ann in enumerate(anns):
        if ann == ref.OWN_ANNOTATION:
            continue
        feats, frame_start = sigmf.extract_sigmf(noted, 1024, tune=dict(annotation=k, oversample=2, rational=True))
        assert feats.shape[0] >= 2 and feats.shape[1] == 18 and np.all(np.isfinite(feats)), (k, ann)


def test_spectrogram_and_detect_replay_in_a_graph():
    t = _torch()
    nfft, hop, A, R = 1024, 512, 4, 6
    w = t.from_numpy(psd.window(nfft, "hann")).cuda()
    S = _samples_for(R, nfft, hop, A)
    xd = t.from_numpy(_noise(S, 1)).cuda()
    out = t.empty((R, nfft), dtype=t.float32, device="cuda")
    eager = {}
    for seed in (2, 3):
        xd.copy_(t.from_numpy(_noise(S, seed)).cuda())
        P = psd.spectrogram(xd, nfft, hop=hop, averages=A, window=w, out=out)
        det = psd.detect(P)
        t.cuda.synchronize()
        eager[seed] = (P.cpu().numpy().copy(), det.floor.cpu().numpy(), det.mask.cpu().numpy())
    g = t.cuda.CUDAGraph()
    with t.cuda.graph(g):
        P = psd.spectrogram(xd, nfft, hop=hop, averages=A, window=w, out=out)
        det = psd.detect(P)
    for seed in (2, 3):
        xd.copy_(t.from_numpy(_noise(S, seed)).cuda())
        out.fill_(SENTINEL)
        g.replay()
        t.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), eager[seed][0])
        assert np.array_equal(det.floor.cpu().numpy(), eager[seed][1]) and np.array_equal(det.mask.cpu().numpy(), eager[seed][2])


# ---- the persistent loops' second and third trips ----------------------------------------------------------------------------
# Every case below gives its launch at least 2 * grid + 1 units of work, the grid read from the library, so that some workgroup
# goes round its grid-stride loop three times and the last trip is ragged: the loop's tail barrier, the state re-derived per
# trip (live, acc[], row words) and `unit * stride` at large indices all run.

def _float32_rows_blocked(x, w, nfft, hop, A, R, block=8192):
    """ref.float32_rows over R rows in blocks of rows, to bound memory."""
    out = np.empty((R, nfft), np.float32)
    step, span = A * hop, (A - 1) * hop + nfft
    for r in range(0, R, block):
        n = min(block, R - r)
        out[r:r + n] = ref.float32_rows(x[r * step:(r + n - 1) * step + span], w, nfft, hop, A)
    return out


def _passes(R, nfft, hop, A, what):
    """(passes, grid) of a spectrogram of R rows, asserted to be three trips for some workgroup, and printed."""
    G, _, grid = _lib.spectrogram_plan(nfft, hop, A)
    passes = -(-R // G)
    print(f"spectrogram {what}: {R} rows = {passes} passes of {G} over {grid} workgroups")
    assert passes >= 2 * grid + 1
    return passes, grid


@pytest.mark.parametrize("nfft,A", [(64, 1), (64, 2), (4096, 1)])
def test_rows_equal_the_float32_restatement_over_three_trips_of_the_grid(nfft, A):
    """hop = 1: a row costs A samples.  nfft = 64: 2 g + 1 passes of 64 slots, the last with 3 live (A = 1) or 5 (A = 2, the
    accumulators re-seeded between trips); nfft = 4096: one row per pass, 2 g + 1 rows."""
    G, _, g = _lib.spectrogram_plan(nfft, 1, A)
    R = G * (2 * g + 1) + 3 if (nfft, A) == (64, 1) else G * 2 * g + (5 if G > 1 else 1)
    _passes(R, nfft, 1, A, f"nfft={nfft} A={A}")
    w = psd.window(nfft, "hann")
    x = ref.spread_signal(_samples_for(R, nfft, 1, A), nfft, 33 * nfft + A)
    P = _run(x, nfft, hop=1, averages=A, window=w)
    assert P.shape == (R, nfft)
    assert np.array_equal(P, _float32_rows_blocked(x, w, nfft, 1, A, R))


@pytest.mark.parametrize("fmt", ["sc16", "ci8"])
def test_integer_formats_are_the_complex64_bits_over_three_trips_of_the_grid(fmt):
    """Each loader is a kernel of its own with its own copy of the pass loop."""
    nfft = 64
    G, _, g = _lib.spectrogram_plan(nfft, 1, 1)
    R = G * (2 * g + 1) + 3
    _passes(R, nfft, 1, 1, f"{fmt} nfft={nfft}")
    w = psd.window(nfft, "hann")
    raw = _raw(_samples_for(R, nfft, 1, 1), fmt, 33)
    scale = ref.DEFAULT_SCALE[fmt] * 1.25
    wide = ddc_ref.widen(raw, fmt, scale).astype(np.complex64)
    got = _run(raw, nfft, hop=1, averages=1, window=w, scale=scale)
    assert got.shape == (R, nfft) and np.array_equal(got, _run(wide, nfft, hop=1, averages=1, window=w))


def test_padding_is_untouched_over_three_trips_of_the_grid():
    """r * stride at large r: rows of nfft + 5 floats, the 5 a sentinel before and after."""
    t = _torch()
    nfft = 64
    G, _, g = _lib.spectrogram_plan(nfft, 1, 1)
    R = G * (2 * g + 1) + 3
    _passes(R, nfft, 1, 1, f"padded nfft={nfft}")
    w = psd.window(nfft, "hann")
    xd = t.from_numpy(ref.spread_signal(_samples_for(R, nfft, 1, 1), nfft, 34)).cuda()
    base = psd.spectrogram(xd, nfft, hop=1, averages=1, window=w)
    out = t.full((R + 1, nfft + 5), SENTINEL, dtype=t.float32, device="cuda")
    got = psd.spectrogram(xd, nfft, hop=1, averages=1, window=w, out=out[:R])
    t.cuda.synchronize()
    assert t.equal(got, base) and t.equal(out[:R, :nfft], base)
    assert bool((out[:, nfft:] == SENTINEL).all()) and bool((out[R] == SENTINEL).all())


@pytest.mark.parametrize("bins", [2, 65, 1000])
def test_detect_equals_numpy_over_three_trips_of_the_grid(bins):
    """One row per trip.  The grid restates the call site of amcx_psd_detect_f32 in amcx.hip (8 workgroups per CU): there is
    no plan entry for it.  The rows tile _detect_rows' nine kinds (random, ties, all equal, NaN and inf rows), the tiling
    shifted after every `grid` rows so that a workgroup's consecutive trips see different kinds."""
    t = _torch()
    lib = _lib.load()
    grid = 8 * t.cuda.get_device_properties(0).multi_processor_count
    R = 2 * grid + 5
    print(f"psd detect bins={bins}: {R} rows over {grid} workgroups")
    assert R >= 2 * grid + 1
    nine = _detect_rows(9, bins, bins + 1)
    shift = 1 if (grid + 1) % 9 else 2
    kind = (np.arange(R) + shift * (np.arange(R) // grid)) % 9            # row r + grid is another kind than row r
    assert np.all(kind[grid:] != kind[:-grid])
    rng = np.random.default_rng(bins)
    p = nine[kind]
    plain = np.isin(kind, (0, 7, 8))                                      # the random rows: fresh values per row
    p[plain] = (rng.standard_normal((int(plain.sum()), bins)) ** 2).astype(np.float32)
    stride = bins + 3
    pd = t.full((R, stride), SENTINEL, dtype=t.float32, device="cuda")
    pd[:, :bins].copy_(t.from_numpy(p).cuda())
    thr = occupancy.threshold_of(6.0)
    for rank in sorted({0, bins // 2, bins - 1}):
        floor = t.full((R + 1,), SENTINEL, dtype=t.float32, device="cuda")
        mask = t.full((R * bins + 1,), 9, dtype=t.uint8, device="cuda")
        _lib.check(lib.amcx_psd_detect_f32(pd.data_ptr(), R, bins, stride, rank, float(thr), floor.data_ptr(), mask.data_ptr(),
                                           t.cuda.current_stream().cuda_stream))
        t.cuda.synchronize()
        f, m = ref.numpy_psd_detect(p, rank, thr)
        fl, mk = floor.cpu().numpy(), mask.cpu().numpy()
        assert np.array_equal(fl[:R], f, equal_nan=True), (bins, rank)
        assert np.array_equal(mk[:R * bins].reshape(R, bins).astype(bool), m), (bins, rank)
        assert fl[R] == SENTINEL and mk[R * bins] == 9
    assert bool((pd[:, bins:] == SENTINEL).all())
