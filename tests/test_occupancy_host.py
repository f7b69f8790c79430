"""Occupancy detection (include/amcx.h, ABI 14) on the host: the new symbols and their argument checks in the order the header
states, the workspace size, the exact numpy detection (tests/occupancy_ref.py) against a brute-force sort, the segments, the
survey of a synthetic SigMF recording over injected numpy computes, the command line's flags and the annotation round trip.
Needs no GPU."""
import json
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib, occupancy
from tests import bank_ref, occupancy_ref as ref
from tests.stream_inputs import aligned as _aligned

REPO = Path(__file__).resolve().parents[1]
NEW = ["amcx_row_power_c64", "amcx_occupancy_workspace_bytes", "amcx_occupancy_detect_f32", "amcx_gather_rows_c64",
       "amcx_kernel_name_occupancy"]
KERNELS = ["amcx_row_power_kernel", "amcx_occupancy_detect_kernel", "amcx_gather_rows_kernel", "amcx_occupancy_count_kernel",
           "amcx_occupancy_scan_kernel", "amcx_occupancy_scatter_kernel"]


def test_abi_14_symbols_exist_and_bind():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 14 and lib.amcx_abi_version() >= 14
    header = (REPO / "include" / "amcx.h").read_text()
    assert "#define AMCX_ABI_VERSION 14" in header
    for older in (13, 12, 11, 10):                                           # the live one first, the older lines kept
        assert header.index("#define AMCX_ABI_VERSION 14") < header.index(f"#define AMCX_ABI_VERSION {older}")
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    flat = " ".join(header.split())
    assert ("int amcx_row_power_c64(const void* rows_dev, int64_t n_rows, int32_t row_samples, int64_t row_stride_samples, "
            "float* power_dev, void* hip_stream);") in flat
    assert "int64_t amcx_occupancy_workspace_bytes(int32_t channels, int64_t n_frames);" in flat
    assert ("int amcx_occupancy_detect_f32(const float* power_dev, int32_t channels, int64_t n_frames, int32_t floor_rank, "
            "float threshold, float* floor_dev, uint8_t* mask_dev, int32_t* rows_dev, int32_t* count_dev, void* workspace_dev, "
            "int64_t workspace_bytes, void* hip_stream);") in flat
    assert ("int amcx_gather_rows_c64(const void* src_dev, int64_t n_src_rows, int32_t row_samples, int64_t row_stride_samples, "
            "const int32_t* index_dev, int64_t n_index, void* dst_dev, int64_t dst_stride_samples, void* hip_stream);") in flat
    assert "const char* amcx_kernel_name_occupancy(int32_t which);" in flat
    assert [_lib.kernel_name_occupancy(i) for i in range(6)] == KERNELS
    for which in (-1, 6, 100):
        with pytest.raises(ValueError):
            _lib.kernel_name_occupancy(which)
    # the committed resource table knows the kernels by the names the query gives: nothing spilled
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    for name in KERNELS:
        assert table[name]["spill"] == 0 and table[name]["scratch"] == 0, name
    # the per-kernel listing against the parent: every kernel that existed kept its bytes, the six are new
    listing = (REPO / "profiles" / "r21_occupancy_codeobj_kernels.txt").read_text()
    assert "identical" in listing.splitlines()[0] and "DIFFER" not in listing.upper().replace("IDENTICAL", "")
    assert sorted(l.split("::")[-1] for l in listing.splitlines() if l.startswith("ONLY IN B")) == sorted(KERNELS)
    assert "ONLY IN A" not in listing


def test_row_power_refusals_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_row_power_c64
    keep, p = _aligned()
    nul = dict(rows=None, power=None)

    def call(**kw):
        a = {**dict(rows=p, R=4, N=8, stride=8, power=p), **kw}
        return f(a["rows"], a["R"], a["N"], a["stride"], a["power"], None)
    # 1. ranges, also where the call would otherwise be the no-op
    for kw in (dict(R=-1), dict(N=1), dict(N=0), dict(N=32769), dict(N=-5)):
        assert call(**kw) == _lib.EINVAL and call(**{"R": 0, **kw}, **nul) == _lib.EINVAL, kw
    # 2. the stride
    for kw in (dict(stride=7), dict(stride=0), dict(stride=-8), dict(R=1 << 40, stride=1 << 40), dict(R=1 << 2, stride=(1 << 56) + 1)):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(R=0, stride=7, **nul) == _lib.EINVAL and call(R=0, stride=-8, **nul) == _lib.EINVAL
    # 3. nothing to do
    assert call(R=0, **nul) == _lib.OK and call(R=0, N=32768, stride=1 << 50, **nul) == _lib.OK
    # 4. null pointers and alignment
    assert call(rows=None) == _lib.EINVAL and call(power=None) == _lib.EINVAL
    assert call(rows=p + 4) == _lib.EINVAL and call(power=p + 2) == _lib.EINVAL
    del keep


def test_detect_refusals_in_the_documented_order_without_a_device():
    lib = _lib.load()
    f = lib.amcx_occupancy_detect_f32
    keep, p = _aligned()
    need = lib.amcx_occupancy_workspace_bytes(8, 100)
    nul = dict(power=None, floor=None, mask=None, rows=None, count=None, ws=None)

    def call(**kw):
        a = {**dict(power=p, C=8, K=100, rank=1, thr=4.0, floor=p, mask=p, rows=p, count=p, ws=p, wsb=need), **kw}
        return f(a["power"], a["C"], a["K"], a["rank"], a["thr"], a["floor"], a["mask"], a["rows"], a["count"], a["ws"], a["wsb"], None)
    # 1. the limits, in front of the no-op
    for kw in (dict(C=1), dict(C=257), dict(C=0), dict(K=-1), dict(C=256, K=1 << 23), dict(C=2, K=1 << 30), dict(rank=-1),
               dict(rank=8), dict(thr=0.0), dict(thr=-1.0), dict(thr=float("inf")), dict(thr=float("nan"))):
        assert call(**kw) == _lib.EINVAL, kw
        assert call(**{"K": 0, **kw}, **nul) == _lib.EINVAL, kw
    # 2. the workspace's size, where rows or the count are wanted
    assert call(wsb=need - 1) == _lib.EINVAL and call(wsb=0, rows=None) == _lib.EINVAL and call(wsb=-1) == _lib.EINVAL
    # 3. nothing to do: no pointer is looked at
    assert call(K=0, wsb=0, **nul) == _lib.OK and call(K=0, C=256, rank=255, wsb=0, **nul) == _lib.OK
    # 4. null pointers and alignment
    for kw in (dict(power=None), dict(floor=None), dict(count=None), dict(ws=None), dict(ws=None, rows=None),
               dict(power=p + 2), dict(floor=p + 1), dict(rows=p + 2), dict(count=p + 3), dict(ws=p + 2)):
        assert call(**kw) == _lib.EINVAL, kw
    del keep


def test_gather_refusals_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_gather_rows_c64
    keep, p = _aligned()
    nul = dict(src=None, index=None, dst=None)

    def call(**kw):
        a = {**dict(src=p, R=4, N=8, stride=8, index=p, n=3, dst=p, dstride=8), **kw}
        return f(a["src"], a["R"], a["N"], a["stride"], a["index"], a["n"], a["dst"], a["dstride"], None)
    for kw in (dict(R=-1), dict(n=-1), dict(N=1), dict(N=32769)):
        assert call(**kw) == _lib.EINVAL and call(**{"n": 0, **kw}, **nul) == _lib.EINVAL, kw
    for kw in (dict(stride=7), dict(dstride=7), dict(dstride=0)):
        assert call(**kw) == _lib.EINVAL and call(n=0, **kw, **nul) == _lib.EINVAL, kw
    # the row gate on either side: a stride of 0, a negative one, and one whose product with the row count passes 2^58
    for kw in (dict(stride=0), dict(stride=-8), dict(dstride=-8), dict(R=1 << 40, stride=1 << 40), dict(n=1 << 40, dstride=1 << 40),
               dict(R=1 << 2, stride=(1 << 56) + 1), dict(n=1 << 2, dstride=(1 << 56) + 1)):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(n=0, stride=0, **nul) == _lib.EINVAL and call(n=0, R=1 << 40, stride=1 << 40, **nul) == _lib.EINVAL
    assert call(n=0, dstride=1 << 60, **nul) == _lib.OK                      # no destination row, no product
    assert call(n=0, **nul) == _lib.OK and call(n=0, R=0, **nul) == _lib.OK
    for kw in (dict(src=None), dict(index=None), dict(dst=None), dict(src=p + 4), dict(index=p + 2), dict(dst=p + 4)):
        assert call(**kw) == _lib.EINVAL, kw
    del keep


def test_workspace_bytes_is_monotone_and_refuses():
    w = _lib.load().amcx_occupancy_workspace_bytes
    assert w(2, 0) == 0 and w(256, 0) == 0
    for Cn in (2, 3, 8, 64, 255, 256):
        last = 0
        for K in (0, 1, 2, 63, 64, 65, 1000, 70000, (1 << 31) // Cn - 1):
            if Cn * K >= 1 << 31:
                continue
            got = w(Cn, K)
            assert got >= last and got >= 4 * (-(-(Cn * K) // 256)) and got % 256 == 0, (Cn, K)
            last = got
    for K in (1, 1000, 70000):                                               # ... and in the channels
        sizes = [w(Cn, K) for Cn in range(2, 257)]
        assert sizes == sorted(sizes)
    for Cn, K in ((1, 10), (257, 10), (0, 0), (-2, 5), (8, -1), (256, 1 << 23), (2, 1 << 30), (8, 1 << 62)):
        assert w(Cn, K) == -1, (Cn, K)


def _detect_cases():
    rng = np.random.default_rng(5)
    yield "ties", rng.integers(0, 4, (7, 40)).astype(np.float32)
    p = rng.standard_normal((9, 50)).astype(np.float32) ** 2
    p[rng.integers(0, 9, 30), rng.integers(0, 50, 30)] = np.nan
    p[rng.integers(0, 9, 10), rng.integers(0, 50, 10)] = np.inf
    p[:, 7] = np.nan                                                          # a frame of NaN: the floor is NaN, nothing occupied
    p[:, 8] = 0.0                                                             # a frame of zeros: floor 0, nothing > 0
    p[3, 9] = 0.0
    yield "special", p
    yield "two", np.array([[1.0, 5.0, np.nan], [2.0, 1.0, 3.0]], np.float32)


def test_numpy_detect_against_a_brute_force_sort():
    for name, p in _detect_cases():
        Cn = p.shape[0]
        for rank in sorted({0, 1, Cn // 2, Cn - 1}):
            for thr in (1.0, 3.98, 0.5):
                floor, mask, rows = ref.numpy_detect(p, rank, np.float32(thr))
                bf, bm, br = ref.brute_detect(p, rank, np.float32(thr))
                assert floor.dtype == np.float32 and np.array_equal(floor, bf, equal_nan=True), (name, rank, thr)
                assert np.array_equal(mask, bm) and np.array_equal(rows, br) and rows.dtype == np.int32, (name, rank, thr)
                assert np.all(np.diff(rows) > 0)
    p = dict(_detect_cases())["special"]
    floor, mask, _ = ref.numpy_detect(p, 0, np.float32(2.0))
    assert np.isnan(floor[7]) and not mask[:, 7].any()                        # NaN sorts last: rank 0 of all-NaN is NaN
    assert floor[8] == 0.0 and not mask[:, 8].any()
    assert floor[9] == 0.0 and mask[:, 9].sum() == np.sum(p[:, 9] > 0)        # floor 0: everything positive is occupied
    assert not mask[np.isnan(p)].any()                                        # a NaN power is not occupied
    floor, mask, _ = ref.numpy_detect(p, p.shape[0] - 1, np.float32(2.0))
    assert np.all(np.isnan(floor[np.isnan(p).any(axis=0)]))                   # the last rank is a NaN where the frame has one


def test_rank_and_threshold_of_the_python_layer():
    assert [occupancy.floor_rank_of(c, 0.25) for c in (2, 3, 8, 64, 255, 256)] == [0, 0, 1, 15, 63, 63]
    assert occupancy.floor_rank_of(8, 0.0) == 0 and occupancy.floor_rank_of(8, 1.0) == 7
    t = occupancy.threshold_of(6.0)
    assert t.dtype == np.float32 and t == np.float32(10.0 ** 0.6)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            occupancy.floor_rank_of(8, bad)
    for bad in (float("nan"), 1000.0, -1000.0):
        with pytest.raises(ValueError):
            occupancy.threshold_of(bad)


def test_segments():
    m = np.zeros((4, 10), bool)
    m[0, :] = True
    m[1, 3:6] = True
    m[1, 9] = True
    m[3, 0] = True
    m[3, 2:4] = True
    assert occupancy.segments(m) == [(0, 0, 9), (1, 3, 5), (1, 9, 9), (3, 0, 0), (3, 2, 3)]
    assert occupancy.segments(np.zeros((3, 0), bool)) == [] and occupancy.segments(np.zeros((2, 5), np.uint8)) == []
    with pytest.raises(ValueError):
        occupancy.segments(np.zeros((5,), bool))


# ---- the survey of a recording, over injected computes ------------------------------------------------------------------
SURVEY = dict(C=8, N=128, frames=24, seed=1)


def _engine(frames):
    """An injected feature engine: 18 numbers that name the row's samples (any change of a sample changes them)."""
    f = np.asarray(frames)
    p = (np.abs(f.astype(np.complex128)) ** 2).sum(axis=1)
    return (p[:, None] * (1.0 + np.arange(18))[None, :]).astype(np.float32)


def _labeller(rows):
    return (np.asarray(rows)[:, 0] > 2000.0).astype(np.int32) + 3


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    out = {}
    for over in (1, 2):
        x, burst = ref.raster(SURVEY["C"], SURVEY["N"], SURVEY["frames"], over, SURVEY["seed"])
        stem, held = ref.write_sigmf(tmp_path_factory.mktemp(f"rec{over}"), x, "cf32_le")
        out[over] = (stem, held, burst)
    return out


@pytest.mark.parametrize("oversample", [1, 2])
def test_survey_sigmf_with_injected_computes(recording, oversample):
    from amcpy_amd import sigmf
    stem, held, burst = recording[oversample]
    Cn, N, F = SURVEY["C"], SURVEY["N"], SURVEY["frames"]
    ch = {"channels": Cn, "oversample": oversample}
    kw = dict(channelize=ch, bank_compute=bank_ref.numpy_bank, occupancy_compute=ref.numpy_occupancy, compute=_engine)
    full, frame_start = sigmf.extract_sigmf(stem, N, channelize=ch, bank_compute=bank_ref.numpy_bank, compute=_engine)
    assert full.shape == (Cn, F, 18)
    got = sigmf.survey_sigmf(stem, N, detect={"threshold_db": 6.0, "floor_quantile": 0.25}, model=_labeller, **kw)
    assert set(got) == {"features", "frame_start", "power", "floor", "occupied", "snr_db", "segments", "labels"}
    assert np.array_equal(got["frame_start"], frame_start) and got["frame_start"].dtype == np.int64
    occ = got["occupied"]
    assert occ.dtype == bool and occ.shape == (Cn, F) and got["power"].shape == (Cn, F) and got["floor"].shape == (F,)
    # the truth: the float64 route, and nothing near the threshold
    D = Cn // oversample
    y = bank_ref.numpy_bank(held, sigmf.resolve_channelize({"global": {}}, ch)[3], Cn, D)
    p64 = ref.power64(y[:, :F * N].reshape(Cn * F, N)).reshape(Cn, F)
    db = 10.0 * np.log10(p64 / np.sort(p64, axis=0)[1][None, :])
    assert not np.any(np.abs(db - 6.0) < 3.0)
    assert np.array_equal(occ, db > 6.0)
    assert occ[2].all() and np.flatnonzero(occ[5]).tolist() == list(range(burst[0], burst[1] + 1)) and occ.sum() == F + burst[1] - burst[0] + 1
    assert got["segments"] == [(2, 0, F - 1), (5, burst[0], burst[1])]
    # features and labels where occupied, NaN and -2 elsewhere
    assert np.array_equal(got["features"][occ], full[occ]) and np.all(np.isnan(got["features"][~occ]))
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"][occ], _labeller(full[occ])) and np.all(got["labels"][~occ] == -2)
    assert np.all(got["snr_db"][occ] > 15.0) and got["snr_db"].dtype == np.float32
    # without detect: every cell, as extract_sigmf, plus power and floor; labels everywhere
    plain = sigmf.survey_sigmf(stem, N, model=_labeller, **kw)
    assert set(plain) == {"features", "frame_start", "power", "floor", "labels"}
    assert np.array_equal(plain["features"], full) and np.array_equal(plain["power"], got["power"]) and np.array_equal(plain["floor"], got["floor"])
    assert np.array_equal(plain["labels"], _labeller(full.reshape(-1, 18)).reshape(Cn, F))
    # however the segment is read
    again = sigmf.survey_sigmf(stem, N, detect={}, chunk_samples=4099, **kw)
    assert np.array_equal(again["occupied"], occ) and np.array_equal(again["features"], got["features"], equal_nan=True)
    with pytest.raises(ValueError):
        sigmf.survey_sigmf(stem, N, channelize=ch, bank_compute=bank_ref.numpy_bank)          # the three go together
    with pytest.raises(ValueError):
        sigmf.survey_sigmf(stem, N, detect={"threshold": 6.0}, **kw)


def test_recording_command_occupancy_flags_and_annotation(recording, tmp_path):
    from scipy.io import loadmat
    from amcpy_amd import main as cli, sigmf
    stem, held, burst = recording[2]
    Cn, N, F = SURVEY["C"], SURVEY["N"], SURVEY["frames"]
    parse = cli.build_parser().parse_args
    base = ["recording", str(stem), "--frame-size", str(N)]
    chan = ["--channels", str(Cn), "--oversample", "2"]
    assert cli.recording_survey(parse(base)) is None and cli.recording_survey(parse(base + chan)) is None
    # every new flag without --channels is refused by name
    for flags in (["--detect"], ["--threshold-db", "3"], ["--floor-quantile", "0.5"], ["--model", "7"], ["--root", "."],
                  ["--mode", "test"], ["--annotate", "x.sigmf-meta"]):
        with pytest.raises(SystemExit, match=flags[0]):
            cli.recording_survey(parse(base + flags))
        with pytest.raises(SystemExit, match=flags[0]):
            cli.main(base[0:1] + base[1:] + flags)
    for flags, name in ((["--threshold-db", "3"], "--threshold-db"), (["--floor-quantile", "0.5"], "--floor-quantile"),
                        (["--annotate", "x"], "--annotate"), (["--root", "."], "--root"), (["--mode", "test"], "--mode"),
                        (["--model", "7"], "--model")):
        with pytest.raises(SystemExit, match=name):
            cli.recording_survey(parse(base + chan + flags))
    got = cli.recording_survey(parse(base + chan + ["--detect", "--threshold-db", "5", "--model", "7", "--root", "r", "--mode", "training"]))
    assert got == {"detect": {"threshold_db": 5.0, "floor_quantile": 0.25}, "model": "7", "root": Path("r"), "mode": "training",
                   "annotate": None}
    assert cli.recording_survey(parse(base + chan + ["--detect"]))["detect"] == {"threshold_db": 6.0, "floor_quantile": 0.25}
    # the files
    noted = tmp_path / "noted.sigmf-meta"
    args = parse(base + chan + ["--detect", "--model", "x.npz", "--root", str(tmp_path), "--annotate", str(noted),
                                "--out", str(tmp_path / "o.mat")])
    names = ["a", "b", "c", "weak", "strong"]
    out = cli.run_recording(args, compute=_engine, bank_compute=bank_ref.numpy_bank, occupancy_compute=ref.numpy_occupancy,
                            model=_labeller, class_names=names)
    mat = loadmat(out)
    assert {"features", "frame_start", "channel_freq_hz", "power", "floor", "occupied", "snr_db", "labels", "class_names"} <= set(mat)
    occ = mat["occupied"].astype(bool)
    assert occ.shape == (Cn, F) and mat["power"].shape == (Cn, F) and mat["floor"].size == F and mat["labels"].shape == (Cn, F)
    assert [str(np.ravel(v)[0]) for v in np.ravel(mat["class_names"])] == names
    assert np.all(np.isnan(mat["features"][~occ])) and np.all(mat["labels"][~occ] == -2)
    # without the new flags the file is what it was
    mat0 = loadmat(cli.run_recording(parse(base + chan + ["--out", str(tmp_path / "p.mat")]), compute=_engine, bank_compute=bank_ref.numpy_bank))
    assert "power" not in mat0 and np.array_equal(mat0["features"][occ], mat["features"][occ])
    # the annotations: one per segment, read back through read_meta and tune_from_annotation
    Path(str(tmp_path / "noted") + ".sigmf-data").write_bytes(Path(str(stem) + ".sigmf-data").read_bytes())
    rec = sigmf.read_meta(noted)
    anns = rec["meta"]["annotations"]
    D = Cn // 2
    freqs = mat["channel_freq_hz"].ravel()
    want = [(2, 0, F - 1), (5, burst[0], burst[1])]
    assert len(anns) == len(want)
    by_start = sorted(want, key=lambda s: s[1] * N * D)
    for k, (ann, (c, k0, k1)) in enumerate(zip(anns, by_start)):
        assert ann["core:sample_start"] == k0 * N * D and ann["core:sample_count"] == (k1 - k0 + 1) * N * D
        assert ann["core:freq_upper_edge"] - ann["core:freq_lower_edge"] == pytest.approx(1.0e6 / Cn)
        assert ann["core:label"] in ("weak", "strong")
        shift_hz, decim = sigmf.tune_from_annotation(rec["meta"], k, oversample=2.0)
        assert 100.0e6 - shift_hz == pytest.approx(freqs[c]) and decim == Cn // 2
    assert freqs[2] == pytest.approx(100.0e6 + 2 * 1.0e6 / Cn) and freqs[5] == pytest.approx(100.0e6 - 3 * 1.0e6 / Cn)
    # no sample rate: --annotate says what it needs
    meta = json.loads(Path(str(stem) + ".sigmf-meta").read_text())
    del meta["global"]["core:sample_rate"]
    (tmp_path / "norate.sigmf-meta").write_text(json.dumps(meta))
    (tmp_path / "norate.sigmf-data").write_bytes(Path(str(stem) + ".sigmf-data").read_bytes())
    with pytest.raises(SystemExit, match="sample_rate"):
        cli.run_recording(parse(["recording", str(tmp_path / "norate"), "--frame-size", str(N)] + chan +
                                ["--detect", "--annotate", str(tmp_path / "n2.sigmf-meta")]),
                          compute=_engine, bank_compute=bank_ref.numpy_bank, occupancy_compute=ref.numpy_occupancy)


def test_scaler_fit_is_shared_with_the_classify_command():
    """run_classification and the recording command's --model fit the scaler through one function."""
    import inspect
    from amcpy_amd import classifier, main as cli
    assert "fit_scaler(" in inspect.getsource(classifier.run_classification)
    assert "fit_scaler" in inspect.getsource(cli._survey_model)
    with pytest.raises(ValueError):
        classifier.fit_scaler(None, "other", None)
