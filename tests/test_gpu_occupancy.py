"""Occupancy detection (include/amcx.h, ABI 14) on the GPU: the row power, the detection, the row gather and the survey of a
synthetic recording end to end.

THE POWER CRITERION is |p - p64| <= B 2^-24 p64 for EVERY row, B = 4 ceil(N / 128) + 8 (tests/occupancy_ref.py derives it);
each test prints the worst ratio it saw.  The detection is compared with `==` against exact numpy float32
(occupancy_ref.numpy_detect); everything the contract calls bit-identical is compared as bytes."""
import ctypes as C

import numpy as np
import pytest

from amcpy_amd import _lib, occupancy
from tests import bank_ref, occupancy_ref as ref

pytestmark = pytest.mark.gpu

POWER_N = [2, 3, 127, 128, 129, 130, 256, 1000, 2048, 32768]
CANARY = -7


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _frames(R, N, seed, decades=True):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((R, N)) + 1j * rng.standard_normal((R, N))).astype(np.complex64)
    if decades:
        x = (x * (10.0 ** rng.uniform(-3.0, 3.0, (R, 1))).astype(np.float32)).astype(np.complex64)
    return x


def _power(x):
    t = _torch()
    p = occupancy.row_power(t.from_numpy(np.ascontiguousarray(x)).cuda())
    t.cuda.synchronize()
    return p.cpu().numpy()


@pytest.mark.parametrize("N", POWER_N)
def test_power_criterion(N):
    worst = 0.0
    for R in (1, 3, 65):
        x = _frames(R, N, 100 * N + R)
        p = _power(x)
        assert p.shape == (R,) and p.dtype == np.float32
        r = ref.worst_ratio(p, ref.power64(x), N)
        worst = max(worst, r)
        assert r <= 1.0, (N, R, r)
    print(f"row power N={N} B={ref.bound_factor(N)}: worst |err| / bound = {worst:.4f}")


def test_power_criterion_beyond_one_pass_of_the_grid():
    x = _frames(5000, 128, 9)
    p = _power(x)
    r = ref.worst_ratio(p, ref.power64(x), 128)
    print(f"row power 5000 x 128: worst |err| / bound = {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("N", POWER_N)
def test_power_exact_on_integers(N):
    """|re|, |im| <= 64 (16 at N = 32768): every partial sum is an integer <= 2^24, so float32 is exact in ANY order."""
    amp = 16 if N == 32768 else 64
    assert 2 * N * amp * amp <= 1 << 24
    rng = np.random.default_rng(N)
    re, im = rng.integers(-amp, amp + 1, (7, N)), rng.integers(-amp, amp + 1, (7, N))
    re[0], im[0] = amp, -amp                                                # the largest sum
    re[1], im[1] = 0, 0
    p = _power((re + 1j * im).astype(np.complex64))
    want = (re.astype(np.int64) ** 2 + im.astype(np.int64) ** 2).sum(axis=1)
    assert np.array_equal(p.astype(np.int64), want) and np.array_equal(p, want.astype(np.float32))


@pytest.mark.parametrize("N", [2, 3, 127, 128, 129, 130, 1000, 2048])
def test_power_position_independence(N):
    """A row's bits depend on its samples alone: alone, inside a larger call, reversed, at strides N, N + 1 (rows that begin
    on 8 bytes only) and N + 2, from a base offset by one sample; and nothing behind power is written."""
    t = _torch()
    R = 11
    x = _frames(R, N, 31 * N)
    want = _power(x)
    assert np.isfinite(want).all()
    for r in (0, 4, R - 1):
        assert _power(x[r:r + 1]).tobytes() == want[r:r + 1].tobytes(), (N, r)
    big = np.concatenate([_frames(700, N, 5), x, _frames(300, N, 6)])
    assert _power(big)[700:700 + R].tobytes() == want.tobytes()
    assert _power(x[::-1])[::-1].tobytes() == want.tobytes()
    for stride in (N, N + 1, N + 2):
        for offset in (0, 1):
            flat = t.full((offset + R * stride + 3,), complex(np.nan, np.nan), dtype=t.complex64, device="cuda")
            view = flat[offset:].as_strided((R, N), (stride, 1))
            view.copy_(t.from_numpy(x).cuda())
            assert (view.data_ptr() % 16 == 0) == (offset == 0)
            got = occupancy.row_power(view)
            t.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == want.tobytes(), (N, stride, offset)
    # the raw entry, a canary behind the R results
    xd = t.from_numpy(x).cuda()
    out = t.full((R + 5,), 123.0, dtype=t.float32, device="cuda")
    _lib.check(_lib.load().amcx_row_power_c64(xd.data_ptr(), R, N, N, out.data_ptr(), _stream()))
    t.cuda.synchronize()
    out = out.cpu().numpy()
    assert out[:R].tobytes() == want.tobytes() and np.all(out[R:] == 123.0)


def test_power_nan_and_inf_propagate():
    x = _frames(6, 130, 3, decades=False)
    x[1, 129] = complex(np.nan, 0.0)
    x[2, 0] = complex(0.0, np.inf)
    x[3, 64] = complex(-np.inf, 1.0)
    x[4, 5] = complex(3.0e19, 3.0e19)                                       # overflows to +inf as IEEE says
    p = _power(x)
    assert np.isnan(p[1]) and p[2] == np.inf and p[3] == np.inf and p[4] == np.inf and np.isfinite(p[[0, 5]]).all()


# ---- detection -----------------------------------------------------------------------------------------------------------------
def _detect_raw(power, rank, thr, want_mask=True, want_rows=True, want_count=True):
    """amcx_occupancy_detect_f32 itself: -> (floor, mask | None, the WHOLE rows buffer | None, count | None)."""
    t = _torch()
    lib = _lib.load()
    Cn, K = power.shape
    pd = t.from_numpy(np.ascontiguousarray(power, dtype=np.float32)).cuda()
    floor = t.full((K + 3,), -5.0, dtype=t.float32, device="cuda")
    mask = t.full((Cn * K + 3,), 9, dtype=t.uint8, device="cuda") if want_mask else None
    rows = t.full((Cn * K + 3,), CANARY, dtype=t.int32, device="cuda") if want_rows else None
    count = t.full((2,), CANARY, dtype=t.int32, device="cuda") if want_count else None
    need = lib.amcx_occupancy_workspace_bytes(Cn, K)
    ws = t.empty((need + 4,), dtype=t.uint8, device="cuda")
    ptr = lambda v: None if v is None else v.data_ptr()     # noqa: E731
    _lib.check(lib.amcx_occupancy_detect_f32(pd.data_ptr(), Cn, K, int(rank), float(np.float32(thr)), floor.data_ptr(), ptr(mask),
                                             ptr(rows), ptr(count), ws.data_ptr(), need, _stream()))
    t.cuda.synchronize()
    host = lambda v: None if v is None else v.cpu().numpy()  # noqa: E731
    floor, mask, rows, count = host(floor), host(mask), host(rows), host(count)
    assert np.all(floor[K:] == -5.0)
    if mask is not None:
        assert np.all(mask[Cn * K:] == 9)
        mask = mask[:Cn * K].reshape(Cn, K)
    if count is not None:
        assert count[1] == CANARY
    return floor[:K], mask, rows, None if count is None else int(count[0])


def _check_detect(power, rank, thr, tag):
    floor, mask, rows = ref.numpy_detect(power, rank, np.float32(thr))
    gf, gm, gr, n = _detect_raw(power, rank, thr)
    assert np.array_equal(gf, floor, equal_nan=True), tag
    assert gm.dtype == np.uint8 and np.array_equal(gm, mask.astype(np.uint8)), tag
    assert n == rows.size, tag
    assert np.array_equal(gr[:n], rows) and np.all(gr[n:] == CANARY), tag
    return n


def _tied(Cn, K, seed):
    return np.random.default_rng(seed).integers(0, 4, (Cn, K)).astype(np.float32)


def _special(Cn, K, seed):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((Cn, K)) ** 2 * 10.0 ** rng.uniform(-2, 2, (Cn, K))).astype(np.float32)
    n = max(1, Cn * K // 50)
    p[rng.integers(0, Cn, n), rng.integers(0, K, n)] = np.nan
    p[rng.integers(0, Cn, n), rng.integers(0, K, n)] = np.inf
    p[:, K // 2] = 0.0                                                       # a frame of zeros: floor 0
    if K > 3:
        p[:, 1] = np.nan                                                     # a frame of NaN
        p[0, 3] = 0.0
    return p


@pytest.mark.parametrize("Cn", [2, 256])
def test_detect_exact_over_three_trips_of_the_floor_grid(Cn):
    """The floor launch walks tiles of 64 frames with 4 workgroups per CU at C = 2 and 2 at C = 256 (67 584 bytes of LDS: this
    restates amcx_occupancy_detect_f32 in amcx.hip, wgs_per_cu(lds, 4) of 160 KiB); 2 grid + 1 tiles and one frame more.  At
    C = 256 the count and scatter launches (4 per CU, blocks of 256 cells) pass 2 grid + 1 blocks as well."""
    per_cu = 4 if Cn == 2 else 2
    grid = per_cu * _torch().cuda.get_device_properties(0).multi_processor_count
    K = 64 * (2 * grid + 1) + 1
    tiles = -(-K // 64)
    print(f"occupancy floor C={Cn}: {K} frames = {tiles} tiles of 64 over {grid} workgroups; {-(-Cn * K // 256)} blocks of 256 cells")
    assert tiles >= 2 * grid + 1
    thr = occupancy.threshold_of(6.0)
    n = _check_detect(_special(Cn, K, 5 + Cn), occupancy.floor_rank_of(Cn, 0.25), thr, ("special, three trips", Cn, K))
    assert 0 < n < Cn * K


@pytest.mark.parametrize("Cn", [2, 3, 8, 64, 255, 256])
def test_detect_exact(Cn):
    thr = occupancy.threshold_of(6.0)
    for K in (1, 63, 64, 65, 1000):
        for rank in sorted({0, occupancy.floor_rank_of(Cn, 0.25), Cn - 1}):
            _check_detect(_tied(Cn, K, 7 * Cn + K), rank, thr, ("tied", Cn, K, rank))
            _check_detect(_special(Cn, K, 11 * Cn + K), rank, thr, ("special", Cn, K, rank))
        _check_detect(_tied(Cn, K, K), 0, np.float32(1.0), ("tied, threshold 1", Cn, K))


def test_detect_exact_beyond_one_pass_of_the_grid():
    """C = 8, K = 70 000: 2188 blocks of 256 rows -- more than the persistent grid holds, and many chunks of the scan."""
    Cn, K = 8, 70_000
    thr = occupancy.threshold_of(6.0)
    n = _check_detect(_tied(Cn, K, 1), 1, thr, "tied 70000")
    assert 0 < n < Cn * K
    _check_detect(_special(Cn, K, 2), 1, thr, "special 70000")
    # the Python layer on the same grid
    t = _torch()
    p = _special(Cn, K, 2)
    occ = occupancy.detect(t.from_numpy(p).cuda(), floor_quantile=0.25, threshold_db=6.0)
    floor, mask, rows = ref.numpy_detect(p, 1, thr)
    assert occ.mask.dtype == t.bool and np.array_equal(occ.mask.cpu().numpy(), mask)
    assert np.array_equal(occ.floor.cpu().numpy(), floor, equal_nan=True)
    assert occ.rows.dtype == t.int32 and np.array_equal(occ.rows.cpu().numpy(), rows)
    snr = occ.snr_db.cpu().numpy()
    assert snr.shape == (Cn, K) and snr.dtype == np.float32
    with np.errstate(all="ignore"):
        want = 10.0 * np.log10(np.maximum(p.astype(np.float64) / floor[None, :] - 1.0, np.finfo(np.float32).tiny))
    ok = np.isfinite(want) & np.isfinite(snr) & (want > -100.0)
    assert ok.sum() > Cn * K // 2 and np.allclose(snr[ok], want[ok], rtol=1e-3, atol=1e-3)


def test_detect_none_all_and_unwanted_outputs():
    rng = np.random.default_rng(4)
    Cn, K = 8, 300
    p = rng.uniform(1.0, 2.0, (Cn, K)).astype(np.float32)
    assert _check_detect(p, 1, np.float32(3.0e38), "none") == 0                # threshold * floor overflows: nothing is above inf
    assert _check_detect(p, 1, np.float32(100.0), "none, finite") == 0
    assert _check_detect(p, Cn - 1, np.float32(0.25), "all") == Cn * K          # even the largest is above a quarter of itself
    floor, mask, rows = ref.numpy_detect(p, 2, np.float32(1.2))
    gf, gm, gr, n = _detect_raw(p, 2, 1.2, want_mask=False)
    assert gm is None and np.array_equal(gf, floor) and n == rows.size and np.array_equal(gr[:n], rows) and np.all(gr[n:] == CANARY)
    gf, gm, gr, n = _detect_raw(p, 2, 1.2, want_rows=False)
    assert gr is None and np.array_equal(gf, floor) and np.array_equal(gm, mask) and n == rows.size
    gf, gm, gr, n = _detect_raw(p, 2, 1.2, want_rows=False, want_count=False)
    assert gr is None and n is None and np.array_equal(gf, floor) and np.array_equal(gm, mask)
    gf, gm, gr, n = _detect_raw(p, 2, 1.2, want_mask=False, want_rows=False, want_count=False)
    assert np.array_equal(gf, floor)


def test_detect_replays_in_a_graph():
    t = _torch()
    lib = _lib.load()
    Cn, K = 64, 1000
    thr = occupancy.threshold_of(6.0)
    pd = t.from_numpy(_special(Cn, K, 1)).cuda()
    floor = t.empty((K,), dtype=t.float32, device="cuda")
    mask = t.empty((Cn * K,), dtype=t.uint8, device="cuda")
    rows = t.empty((Cn * K,), dtype=t.int32, device="cuda")
    count = t.empty((1,), dtype=t.int32, device="cuda")
    need = lib.amcx_occupancy_workspace_bytes(Cn, K)
    ws = t.empty((need,), dtype=t.uint8, device="cuda")
    t.cuda.synchronize()
    g = t.cuda.CUDAGraph()
    with t.cuda.graph(g):
        _lib.check(lib.amcx_occupancy_detect_f32(pd.data_ptr(), Cn, K, 15, float(thr), floor.data_ptr(), mask.data_ptr(),
                                                 rows.data_ptr(), count.data_ptr(), ws.data_ptr(), need, _stream()))
    for seed in (2, 3):
        p = _special(Cn, K, seed) if seed == 2 else _tied(Cn, K, seed)
        pd.copy_(t.from_numpy(p).cuda())
        rows.fill_(CANARY)
        g.replay()
        t.cuda.synchronize()
        f, m, r = ref.numpy_detect(p, 15, thr)
        n = int(count.item())
        assert n == r.size and np.array_equal(rows.cpu().numpy()[:n], r) and np.all(rows.cpu().numpy()[n:] == CANARY)
        assert np.array_equal(floor.cpu().numpy(), f, equal_nan=True) and np.array_equal(mask.cpu().numpy().reshape(Cn, K), m)


# ---- the gather ---------------------------------------------------------------------------------------------------------------
def _gather_raw(x, src_stride, index, dst_stride):
    t = _torch()
    R, N = x.shape
    src = t.full((R * src_stride + 2,), complex(7.0, 7.0), dtype=t.complex64, device="cuda")
    src.as_strided((R, N), (src_stride, 1)).copy_(t.from_numpy(x).cuda())
    idx = t.from_numpy(np.asarray(index, dtype=np.int32)).cuda()
    n = int(idx.shape[0])
    dst = t.full((n * dst_stride + 2,), complex(-3.0, 5.0), dtype=t.complex64, device="cuda")
    _lib.check(_lib.load().amcx_gather_rows_c64(src.data_ptr(), R, N, src_stride, idx.data_ptr() if n else None, n,
                                                dst.data_ptr() if n else None, dst_stride, _stream()))
    t.cuda.synchronize()
    return dst.cpu().numpy()


@pytest.mark.parametrize("N", [2, 127, 128, 2048])
def test_gather(N):
    t = _torch()
    rng = np.random.default_rng(N)
    R = 37
    x = _frames(R, N, N + 1)
    perm = rng.permutation(R)
    index = np.concatenate([perm, [3, 3, 3, 0, R - 1], [-1, R, R + 100, -2 ** 31], perm[:5]])
    bad = (index < 0) | (index >= R)
    for src_stride, dst_stride in ((N, N), (N + 1, N + 2), (N + 2, N + 1), (N + 1, N)):
        got = _gather_raw(x, src_stride, index, dst_stride)
        body = got[:index.size * dst_stride].reshape(index.size, dst_stride)
        assert body[~bad, :N].tobytes() == x[index[~bad]].tobytes(), (N, src_stride, dst_stride)
        assert np.all(np.isnan(body[bad, :N].real)) and np.all(np.isnan(body[bad, :N].imag))
        assert np.all(body[:, N:] == complex(-3.0, 5.0)) and np.all(got[index.size * dst_stride:] == complex(-3.0, 5.0))   # the gaps
    # the Python layer: packed rows; none; many
    xd = t.from_numpy(x).cuda()
    got = occupancy.gather_rows(xd, t.from_numpy(index.astype(np.int32)).cuda())
    assert got.shape == (index.size, N) and got.is_contiguous()
    assert got.cpu().numpy()[~bad].tobytes() == x[index[~bad]].tobytes()
    assert occupancy.gather_rows(xd, t.empty((0,), dtype=t.int32, device="cuda")).shape == (0, N)
    many = rng.integers(0, R, 5000).astype(np.int32)
    got = occupancy.gather_rows(xd, t.from_numpy(many).cuda())
    t.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == x[many].tobytes()
    assert _gather_raw(x, N, np.empty((0,), np.int32), N).size == 2


OCC_WAVES = 4                                     # kOccWaves of amcx_occupancy_kernels.h: rows (indices) a workgroup takes per trip


def _occ_grid():
    """Workgroups of the row-power and gather launches: this restates their call sites in amcx.hip (8 per CU, OCC_WAVES rows
    per workgroup and trip); there is no plan entry for them."""
    return 8 * _torch().cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("N", [2, 127])
def test_gather_over_three_trips_of_the_grid(N):
    """2 grid + 2 workgroups' worth of indices (the last with one of its four): every wave goes round its loop three times.
    Out-of-range indices stand in the second and the third trip, between rows that are copied."""
    grid = _occ_grid()
    per_trip = grid * OCC_WAVES
    n = 2 * per_trip + 5
    units = -(-n // OCC_WAVES)
    print(f"gather N={N}: {n} indices = {units} workgroups' worth over {grid} workgroups")
    assert units >= 2 * grid + 1
    rng = np.random.default_rng(N)
    R = 37
    x = _frames(R, N, N + 2)
    index = rng.integers(0, R, n).astype(np.int64)
    planted = {per_trip + 1: -1, per_trip + 6: R, 2 * per_trip - 3: -2 ** 31, 2 * per_trip + 1: R, 2 * per_trip + 4: -1}
    for at, v in planted.items():
        index[at] = v
    bad = (index < 0) | (index >= R)
    assert int(bad.sum()) == len(planted)
    for src_stride, dst_stride in ((N + 1, N + 2), (N, N + 1)):
        got = _gather_raw(x, src_stride, index, dst_stride)
        body = got[:n * dst_stride].reshape(n, dst_stride)
        assert body[~bad, :N].tobytes() == x[index[~bad]].tobytes(), (N, src_stride, dst_stride)
        assert np.all(np.isnan(body[bad, :N].real)) and np.all(np.isnan(body[bad, :N].imag))
        assert np.all(body[:, N:] == complex(-3.0, 5.0)) and np.all(got[n * dst_stride:] == complex(-3.0, 5.0))           # the gaps


def test_power_criterion_over_three_trips_of_the_grid():
    """Every wave of the row-power grid takes three rows, of N = 129 (the odd sample's lane) at a stride that puts every
    other row on 8 bytes: the criterion for EVERY row, and the bytes of the same rows in calls of one trip."""
    t = _torch()
    grid = _occ_grid()
    R, N = 2 * grid * OCC_WAVES + 5, 129
    units = -(-R // OCC_WAVES)
    print(f"row power N={N}: {R} rows = {units} workgroups' worth over {grid} workgroups")
    assert units >= 2 * grid + 1
    x = _frames(R, N, 12)
    p = _power(x)
    r = ref.worst_ratio(p, ref.power64(x), N)
    print(f"row power {R} x {N}: worst |err| / bound = {r:.4f}")
    assert p.shape == (R,) and r <= 1.0
    xd = t.from_numpy(x).cuda()
    parts = [occupancy.row_power(xd[a:a + 4096]) for a in range(0, R, 4096)]
    t.cuda.synchronize()
    assert t.cat(parts).cpu().numpy().tobytes() == p.tobytes()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
E2E = dict(C=8, N=128, frames=24, seed=1)
_rasters = {}


def _raster(oversample):
    if oversample not in _rasters:
        _rasters[oversample] = ref.raster(E2E["C"], E2E["N"], E2E["frames"], oversample, E2E["seed"])
    return _rasters[oversample]


@pytest.mark.parametrize("oversample", [1, 2])
@pytest.mark.parametrize("datatype", ["cf32_le", "ci16_le"])
def test_survey_end_to_end(tmp_path, datatype, oversample):
    from amcpy_amd import sigmf
    from amcpy_amd.classifier import MlpModel, classify, params_floats
    t = _torch()
    Cn, N, F = E2E["C"], E2E["N"], E2E["frames"]
    x, burst = _raster(oversample)
    stem, held = ref.write_sigmf(tmp_path, x, datatype)
    ch = {"channels": Cn, "oversample": oversample}
    D = Cn // oversample
    # the truth: the float64 route -- and, first, that no cell lies within 3 dB of the threshold
    y = bank_ref.numpy_bank(held, sigmf.resolve_channelize({"global": {}}, ch)[3], Cn, D)
    p64 = ref.power64(y[:, :F * N].reshape(Cn * F, N)).reshape(Cn, F)
    rank = occupancy.floor_rank_of(Cn, 0.25)
    db = 10.0 * np.log10(p64 / np.sort(p64, axis=0)[rank][None, :])
    print(f"survey {datatype} oversample {oversample}: occupied >= {db[db > 6.0].min():.1f} dB, empty <= {db[db <= 6.0].max():.1f} dB over the floor")
    assert not np.any(np.abs(db - 6.0) < 3.0)
    truth = db > 6.0
    assert truth[2].all() and np.flatnonzero(truth[5]).tolist() == list(range(burst[0], burst[1] + 1))

    rng = np.random.default_rng(8)
    widths = (6, 9, 4)
    model = MlpModel(widths, "tanh", rng.standard_normal(params_floats(widths)).astype(np.float32))
    cols = [2, 4, 6, 8, 12, 14]
    kw = dict(cols=cols, mean=np.zeros(6), scale=np.full(6, 3.0))
    got = sigmf.survey_sigmf(stem, N, channelize=ch, detect={"threshold_db": 6.0, "floor_quantile": 0.25}, model=model, **kw)
    full, frame_start = sigmf.extract_sigmf(stem, N, channelize=ch)
    occ = got["occupied"]
    assert np.array_equal(occ, truth)
    assert np.array_equal(got["frame_start"], frame_start) and full.shape == (Cn, F, 18)
    assert got["features"][occ].tobytes() == full[occ].tobytes()               # the same bank, the same kernel, a copy between
    assert np.all(np.isnan(got["features"][~occ]))
    assert got["segments"] == [(2, 0, F - 1), (5, burst[0], burst[1])]
    labels = classify(t.from_numpy(full).cuda(), model, **kw).cpu().numpy()
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"][occ], labels[occ]) and np.all(got["labels"][~occ] == -2)
    assert np.all(got["snr_db"][occ] > 15.0)
    # without detect: every cell
    plain = sigmf.survey_sigmf(stem, N, channelize=ch, model=model, **kw)
    assert plain["features"].tobytes() == full.tobytes() and np.array_equal(plain["labels"], labels)
    assert np.array_equal(plain["power"], got["power"]) and "occupied" not in plain
    # the Python layer's occupied_features on the same cells
    yd = t.from_numpy(np.ascontiguousarray(y[:, :F * N]).reshape(Cn, F, N)).cuda()
    o = occupancy.detect(occupancy.row_power(yd.view(Cn * F, N)).view(Cn, F))
    feats = occupancy.occupied_features(yd, o).cpu().numpy()
    assert np.array_equal(o.mask.cpu().numpy(), truth) and feats.shape == (Cn, F, 18)
    assert np.all(np.isfinite(feats[truth])) and np.all(np.isnan(feats[~truth]))
