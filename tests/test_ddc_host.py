"""The digital down-converter (include/amcx.h, ABI 11) on the host: the new symbols and their argument checks in the order
the header states, the tap design, the streaming bookkeeping over an injected numpy down-converter (tests/ddc_ref.py), the
tuned path of a SigMF recording and the command line's flags.  Needs no GPU."""
import ctypes as C
import json
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib, ddc
from tests import ddc_ref, stream_inputs

REPO = Path(__file__).resolve().parents[1]
NEW = ["amcx_tune_decimate", "amcx_tune_decimate_out_samples", "amcx_tune_decimate_plan", "amcx_kernel_name_ddc"]


def test_abi_11_symbols_exist_and_bind():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 11 and lib.amcx_abi_version() >= 11
    header = (REPO / "include" / "amcx.h").read_text()
    assert "#define AMCX_ABI_VERSION 11" in header
    assert header.index("#define AMCX_ABI_VERSION 11") < header.index("#define AMCX_ABI_VERSION 10")     # the live one first
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    flat = " ".join(header.split())
    assert "int64_t amcx_tune_decimate_out_samples(int64_t n_samples, int32_t n_taps, int32_t decim);" in flat
    assert ("int amcx_tune_decimate(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, uint64_t phase0, "
            "uint64_t phase_step, const float* taps_dev, int32_t n_taps, int32_t decim, void* out_c64_dev, "
            "int64_t out_capacity_samples, void* hip_stream);") in flat
    assert "int amcx_kernel_name_ddc(int32_t src_kind, char* buf, int32_t buf_len);" in flat
    assert _lib.kernel_name_ddc(_lib.SRC_C64) == "amcx_ddc_c64_kernel"
    assert _lib.kernel_name_ddc(_lib.SRC_SC16) == "amcx_ddc_sc16_kernel"
    assert _lib.kernel_name_ddc(_lib.SRC_CI8) == _lib.kernel_name_ddc(_lib.SRC_CU8) == "amcx_ddc_iq8_kernel"
    for kind in (_lib.SRC_C128, _lib.SRC_F32_SPLIT, 5, 10, -1):
        with pytest.raises(ValueError):
            _lib.kernel_name_ddc(kind)
    # the committed resource table knows the three kernels by the names the query gives: nothing spilled
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    for name in ("amcx_ddc_c64_kernel", "amcx_ddc_sc16_kernel", "amcx_ddc_iq8_kernel"):
        assert table[name]["spill"] == 0 and table[name]["scratch"] == 0, name


def test_out_samples_and_plan():
    lib = _lib.load()
    m = lib.amcx_tune_decimate_out_samples
    for T, D in ((1, 1), (7, 3), (5, 17), (2048, 4096), (129, 1)):
        assert [m(S, T, D) for S in (0, T - 1, T, T + D - 1, T + D)] == [0, 0, 1, 1, 2], (T, D)
        assert m(T + 1000 * D, T, D) == 1001 and m((1 << 40) - 1, T, D) == ((1 << 40) - 1 - T) // D + 1
        assert [ddc.out_samples(S, T, D) for S in (T - 1, T, T + D - 1, T + D)] == [0, 1, 1, 2]
    for S, T, D in ((-1, 1, 1), (1 << 40, 1, 1), (10, 0, 1), (10, 2049, 1), (10, 1, 0), (10, 1, 4097), (10, -1, 1)):
        assert m(S, T, D) == -1, (S, T, D)
        with pytest.raises(ValueError):
            ddc.out_samples(S, T, D)
    for T, D in ((1, 1), (2, 1), (7, 3), (5, 17), (63, 4), (64, 64), (129, 4096), (2048, 1), (2048, 4096)):
        tile, grid = _lib.tune_decimate_plan(T, D)
        assert tile >= 1 and grid >= 1
        assert (tile - 1) * D + T <= 6144 < tile * D + T                # the largest tile whose span the LDS stage holds
    for T, D in ((0, 1), (2049, 1), (1, 0), (1, 4097)):
        with pytest.raises(ValueError):
            _lib.tune_decimate_plan(T, D)


def test_refusals_come_in_the_documented_order_without_a_device():
    lib = _lib.load()
    f = lib.amcx_tune_decimate
    buf = (C.c_float * 256)()
    dummy = C.addressof(buf)
    dummy += -dummy % 16
    ok = dict(src=dummy, kind=_lib.SRC_CI8, S=100, scale=2.0 ** -7, taps=dummy, T=5, D=3, out=dummy, cap=32)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["src"], a["kind"], a["S"], a["scale"], 0, 1, a["taps"], a["T"], a["D"], a["out"], a["cap"], None)

    bad_ptr = dict(src=None, taps=None, out=None)
    # 1. the kind, whatever else is wrong
    for kind in (_lib.SRC_C128, _lib.SRC_F32_SPLIT, _lib.SRC_F64_SPLIT, 5, 6, 7, 10, -1):
        assert call(kind=kind) == _lib.EINVAL and call(kind=kind, S=0, **bad_ptr) == _lib.EINVAL
    # 2. the scale, for the integer kinds only -- also where the call would otherwise be the M == 0 no-op
    for kind in (_lib.SRC_SC16, _lib.SRC_CI8, _lib.SRC_CU8):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert call(kind=kind, scale=bad) == _lib.EINVAL and call(kind=kind, scale=bad, S=0, **bad_ptr) == _lib.EINVAL
    assert call(kind=_lib.SRC_C64, scale=float("nan"), S=0, **bad_ptr) == _lib.OK           # ignored for complex64
    # 3. ranges, in front of the no-op
    for kw in (dict(T=0), dict(T=2049), dict(D=0), dict(D=4097), dict(S=-1), dict(S=1 << 40)):
        assert call(**kw) == _lib.EINVAL and call(**{"S": 0, **kw}, **bad_ptr) == _lib.EINVAL, kw
    # 4. the capacity: M = (100 - 5) // 3 + 1 = 32
    assert call(cap=31) == _lib.EINVAL and call(cap=31, **bad_ptr) == _lib.EINVAL and call(cap=-1, S=0) == _lib.EINVAL
    # 5. nothing to write: fine with null pointers, with any capacity >= 0
    assert call(S=4, cap=0, **bad_ptr) == _lib.OK and call(S=0, cap=0, **bad_ptr) == _lib.OK
    # 6. null pointers and alignment
    for key in ("src", "taps", "out"):
        assert call(**{key: None}) == _lib.EINVAL, key
    assert call(src=dummy + 1) == _lib.EINVAL and call(kind=_lib.SRC_CU8, src=dummy + 1) == _lib.EINVAL
    assert call(kind=_lib.SRC_SC16, src=dummy + 2) == _lib.EINVAL
    assert call(kind=_lib.SRC_C64, src=dummy + 4) == _lib.EINVAL
    assert call(taps=dummy + 2) == _lib.EINVAL and call(out=dummy + 4) == _lib.EINVAL
    # a misaligned pointer does not matter where nothing is read or written
    assert call(S=4, cap=0, src=dummy + 1, taps=dummy + 2, out=dummy + 4) == _lib.OK


def test_phase_step_is_integer_arithmetic():
    assert ddc.phase_step_of(0.0) == 0 and ddc.phase_step_of(0.25) == 1 << 62 and ddc.phase_step_of(-0.25) == 3 << 62
    assert ddc.phase_step_of(1.0) == 0 and ddc.phase_step_of(-1.0) == 0 and ddc.phase_step_of(0.5) == ddc.phase_step_of(-0.5) == 1 << 63
    assert ddc.phase_step_of(Fraction(ddc_ref.ODD_STEP, 1 << 64)) == ddc_ref.ODD_STEP
    assert ddc.phase_step_of(Fraction(-1, 1 << 64)) == (1 << 64) - 1
    f = 1234567.0 / 20e6                                     # a float is taken at its exact value
    assert ddc.phase_step_of(-f) == (-int(round(Fraction(f) * (1 << 64)))) % (1 << 64)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ddc.phase_step_of(bad)


def test_design_lowpass():
    for D in (1, 2, 4, 16, 100):
        h = ddc.design_lowpass(D)
        assert h.dtype == np.float32 and h.shape == (16 * D + 1,)
        assert np.array_equal(h, h[::-1])
        assert abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
        if D > 1:
            # the default cutoff, 0.8 of the output Nyquist: passes 0.2 / D, stops the output Nyquist's image zone
            n = np.arange(h.shape[0])
            gain = lambda f: abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f * n)))
            assert gain(0.2 / D) > 0.99 and gain(0.4 / D) == pytest.approx(0.5, abs=0.02) and gain(0.75 / D) < 0.01
    assert ddc.design_lowpass(4, 33).shape == (33,) and ddc.design_lowpass(4, 32).shape == (32,)
    h = ddc.design_lowpass(4, 32)
    assert np.array_equal(h, h[::-1]) and abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
    assert ddc.design_lowpass(1, 1).tolist() == [1.0]
    wide, narrow = ddc.design_lowpass(8, 65, cutoff=0.05), ddc.design_lowpass(8, 65, cutoff=0.02)
    assert wide[32] > narrow[32] > 0
    for kw in (dict(decim=0), dict(decim=4097), dict(decim=4, n_taps=0), dict(decim=200), dict(decim=4, cutoff=0.0),
               dict(decim=4, cutoff=0.6)):
        with pytest.raises(ValueError):
            ddc.design_lowpass(**kw)


_stream = stream_inputs.stream


@pytest.mark.parametrize("fmt", ddc.FORMATS)
@pytest.mark.parametrize("T,D", [(1, 1), (7, 3), (5, 17), (33, 4)])
def test_channelizer_bookkeeping(fmt, T, D):
    """Random chunk lengths -- 0, 1 and below T among them -- give the one-call result bit for bit, and the tail and the
    absolute index are what the definition says."""
    rng = np.random.default_rng(100 * T + D)
    S = 40 * D + 3 * T + 11
    x = _stream(fmt, S, rng)
    taps = ddc_ref.make_taps(T)
    shift = Fraction(ddc_ref.ODD_STEP, 1 << 64)
    scale = None if fmt == "cf32" else 0.03125
    whole = ddc_ref.numpy_ddc(x, taps, D, shift=shift, scale=scale)
    assert whole.shape == (ddc.out_samples(S, T, D),) and whole.dtype == np.complex64
    for trial in range(4):
        cuts = [0, 0, 1, 1, T - 1, T - 1] + rng.integers(0, 3 * D + T, 200).tolist()
        rng.shuffle(cuts)
        chan = ddc.Channelizer(taps, D, shift, fmt, scale, compute=ddc_ref.numpy_ddc)
        got, pos = [], 0
        for n in cuts:
            y = chan.push(x[pos:pos + n])
            pos = min(S, pos + n)
            got.append(y)
            done = sum(len(g) for g in got)
            assert done == ddc.out_samples(pos, T, D) and chan.index == done * D
            assert chan._tail.shape[0] == max(0, pos - chan.index) and np.array_equal(chan._tail, x[chan.index:pos])
            assert y.dtype == np.complex64
            if pos == S:
                break
        assert pos == S
        assert np.concatenate(got).tobytes() == whole.tobytes(), (fmt, T, D, trial)
    with pytest.raises(TypeError):
        ddc.Channelizer(taps, D, shift, fmt, scale, compute=ddc_ref.numpy_ddc).push(np.zeros((4, 3), np.int8))
    with pytest.raises(ValueError):
        ddc.Channelizer(taps, D, shift, "cf64")
    with pytest.raises(ValueError):
        ddc.Channelizer(taps, 4097, shift, fmt)
    if fmt != "cf32":
        with pytest.raises(ValueError):
            ddc.Channelizer(taps, D, shift, fmt, scale=0.0)


def test_tune_decimate_type_errors_arrive_before_the_library_is_touched(monkeypatch):
    import torch

    def no_load(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "require_torch_runtime", no_load)
    taps = np.ones(3, np.float32)
    with pytest.raises(TypeError):
        ddc.tune_decimate(np.zeros(8, np.complex64), taps, 1)                       # not a tensor
    with pytest.raises(TypeError):
        ddc.tune_decimate(torch.zeros(8, dtype=torch.complex128), taps, 1)
    with pytest.raises(TypeError):
        ddc.tune_decimate(torch.zeros((8, 2), dtype=torch.complex64), taps, 1)
    with pytest.raises(TypeError):
        ddc.tune_decimate(torch.zeros((8, 3), dtype=torch.int8), taps, 1)
    with pytest.raises(TypeError):
        ddc.tune_decimate(torch.zeros(8, dtype=torch.int16), taps, 1)
    with pytest.raises(ValueError):
        ddc.tune_decimate(torch.zeros(8, dtype=torch.complex64), taps, 1)          # host memory
    with pytest.raises(ValueError):
        ddc.tune_decimate(torch.zeros((8, 2), dtype=torch.uint8), taps, 1, scale=float("nan"))


# ---- SigMF, tuned ---------------------------------------------------------------------------------------------------
def _write_recording(tmp_path, segs, header_bytes, extra_global=None, captures_extra=None, annotations=None, datatype="ci8"):
    blob, captures, start = b"", [], 0
    for j, (seg, hb) in enumerate(zip(segs, header_bytes)):
        blob += b"\xee" * hb + seg.tobytes()
        cap = {"core:sample_start": start, **((captures_extra or [{}] * len(segs))[j])}
        if hb:
            cap["core:header_bytes"] = hb
        captures.append(cap)
        start += len(seg)
    stem = tmp_path / "tuned"
    Path(str(stem) + ".sigmf-data").write_bytes(blob)
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps({
        "global": {"core:datatype": datatype, "core:version": "1.0.0", **(extra_global or {})}, "captures": captures,
        "annotations": annotations or []}))
    return stem


def test_annotation_arithmetic():
    from amcpy_amd import sigmf
    meta = {"global": {"core:sample_rate": 20e6},
            "captures": [{"core:sample_start": 0, "core:frequency": 100e6}, {"core:sample_start": 5000, "core:frequency": 433e6}],
            "annotations": [{"core:sample_start": 10, "core:freq_lower_edge": 102.5e6, "core:freq_upper_edge": 103.5e6},
                            {"core:sample_start": 5000, "core:freq_lower_edge": 430.0e6, "core:freq_upper_edge": 430.5e6},
                            {"core:sample_start": 4999, "core:freq_lower_edge": 90e6, "core:freq_upper_edge": 110e6},
                            {"core:sample_start": 7}]}
    # 1 MHz wide, 3 MHz above the first capture's centre: shift -3 MHz, D = floor(20 / (2 * 1)) = 10
    assert sigmf.tune_from_annotation(meta, 0) == (-3e6, 10)
    assert sigmf.tune_from_annotation(meta, 0, oversample=4) == (-3e6, 5)
    assert sigmf.tune_from_annotation(meta, 0, oversample=3) == (-3e6, 6)             # floor(6.67)
    # in the SECOND capture: its own centre frequency; 0.5 MHz wide, 2.75 MHz below
    assert sigmf.tune_from_annotation(meta, 1) == (2.75e6, 20)
    # the sample before the second capture still belongs to the first; the whole band: D = max(1, floor(0.5)) = 1
    assert sigmf.tune_from_annotation(meta, 2) == (0.0, 1)
    for k, field in ((3, "freq_lower_edge"), (4, "annotation 4"), (-1, "annotation -1")):
        with pytest.raises(ValueError, match=field):
            sigmf.tune_from_annotation(meta, k)
    with pytest.raises(ValueError, match="sample_rate"):
        sigmf.tune_from_annotation({**meta, "global": {}}, 0)
    with pytest.raises(ValueError, match="core:frequency"):
        sigmf.tune_from_annotation({**meta, "captures": [{"core:sample_start": 0}]}, 0)
    # resolve_tune: Hz over the sample rate, exactly; the default taps; a tap count; the taps themselves
    shift, D, taps = sigmf.resolve_tune(meta, {"annotation": 0})
    assert (shift, D) == (Fraction(-3, 20), 10) and np.array_equal(taps, ddc.design_lowpass(10))
    shift, D, taps = sigmf.resolve_tune(meta, {"shift_hz": 5e6, "decimate": 4, "taps": 33})
    assert (shift, D) == (Fraction(1, 4), 4) and np.array_equal(taps, ddc.design_lowpass(4, 33))
    assert sigmf.resolve_tune({"global": {}}, {"decimate": 2, "taps": [0.5, 0.5]})[2].tolist() == [0.5, 0.5]
    for bad in ({"shift_hz": 1.0}, {"annotation": 0, "decimate": 2}, {"decimate": 2, "oversample": 2}, {"decimate": 2, "x": 1}):
        with pytest.raises(ValueError):
            sigmf.resolve_tune(meta, bad)
    with pytest.raises(ValueError, match="sample_rate"):
        sigmf.resolve_tune({"global": {}}, {"shift_hz": 1.0, "decimate": 2})


@pytest.mark.parametrize("datatype", ["ci8", "cu8", "ci16_le", "cf32_le"])
def test_sigmf_tuned_with_injected_computes(tmp_path, datatype):
    from amcpy_amd import sigmf
    rng = np.random.default_rng(21)
    fmt = sigmf.DATATYPES[datatype][0]
    N, D, T = 8, 3, 7
    lens = [5 * N * D + 11, 3 * N * D + T + 1]
    segs = [_stream(fmt, n, rng) for n in lens]
    stem = _write_recording(tmp_path, segs, [0, 6], {"core:sample_rate": 8.0}, datatype=datatype)
    taps = ddc_ref.make_taps(T)
    tune = {"shift_hz": 1.0, "decimate": D, "taps": taps}                        # an eighth of a turn per sample
    seen = []

    def engine(frames):
        seen.append(np.array(frames))
        return np.full((frames.shape[0], 18), float(len(seen)), np.float32)
    scale = None if fmt == "cf32" else sigmf.DATATYPES[datatype][2]
    per_seg = [ddc_ref.numpy_ddc(seg, taps, D, shift=0.125, scale=scale) for seg in segs]
    n_frames = [len(y) // N for y in per_seg]
    assert n_frames == [5, 3]
    for chunk in (1 << 24, 13, 1):                                               # however the segment is read
        seen.clear()
        feats, frame_start = sigmf.extract_sigmf(stem, N, tune=tune, compute=engine, tune_compute=ddc_ref.numpy_ddc,
                                                 chunk_samples=chunk)
        assert feats.shape == (sum(n_frames), 18) and feats.dtype == np.float32 and frame_start.dtype == np.int64
        assert frame_start.tolist() == [k * N * D for k in range(n_frames[0])] + [lens[0] + k * N * D for k in range(n_frames[1])]
        assert feats[:, 0].tolist() == [1.0] * n_frames[0] + [2.0] * n_frames[1]         # one feature call per capture
        assert len(seen) == 2
        for got, y, n in zip(seen, per_seg, n_frames):                           # no frame holds a sample of the other capture
            assert got.dtype == np.complex64 and got.shape == (n, N) and got.tobytes() == y[:n * N].tobytes()
    feats, frame_start = sigmf.extract_sigmf(stem, N, tune=tune, compute=engine, tune_compute=ddc_ref.numpy_ddc,
                                             max_frames=n_frames[0] + 1, chunk_samples=17)
    assert frame_start.tolist() == [k * N * D for k in range(n_frames[0])] + [lens[0]]
    feats, frame_start = sigmf.extract_sigmf(stem, N, tune=tune, compute=engine, tune_compute=ddc_ref.numpy_ddc, max_frames=2)
    assert frame_start.tolist() == [0, N * D] and feats.shape == (2, 18)
    assert sigmf.extract_sigmf(stem, N, tune=tune, compute=engine, tune_compute=ddc_ref.numpy_ddc, max_frames=0)[0].shape == (0, 18)
    # a feature subset masks the injected engine's columns as on the untuned path
    feats, _ = sigmf.extract_sigmf(stem, N, tune=tune, compute=engine, tune_compute=ddc_ref.numpy_ddc, feature_ids=[3])
    assert np.isnan(feats[:, 0]).all() and not np.isnan(feats[:, 2]).any()


def test_recording_command_tuning_flags(tmp_path):
    from scipy.io import loadmat
    from amcpy_amd import main as cli
    rng = np.random.default_rng(22)
    N, D = 8, 2
    segs = [_stream("ci8", 3 * N * D + 40, rng), _stream("ci8", 2 * N * D + 40, rng)]
    ann = [{"core:sample_start": len(segs[0]) + 1, "core:freq_lower_edge": 99.0, "core:freq_upper_edge": 101.0}]
    stem = _write_recording(tmp_path, segs, [0, 2], {"core:sample_rate": 8.0},
                            [{"core:frequency": 90.0}, {"core:frequency": 101.0}], ann)
    parse = cli.build_parser().parse_args
    base = ["recording", str(stem), "--frame-size", str(N)]
    assert cli.recording_tune(parse(base)) is None
    assert cli.recording_tune(parse(base + ["--decimate", "4"])) == {"shift_hz": 0.0, "decimate": 4, "taps": None}
    assert cli.recording_tune(parse(base + ["--shift-hz", "-2.5", "--decimate", "4", "--taps", "33"])) == \
        {"shift_hz": -2.5, "decimate": 4, "taps": 33}
    assert cli.recording_tune(parse(base + ["--annotation", "0"])) == {"annotation": 0, "oversample": 2.0}
    assert cli.recording_tune(parse(base + ["--annotation", "1", "--oversample", "1.5"])) == {"annotation": 1, "oversample": 1.5}
    for flags in (["--shift-hz", "1"], ["--taps", "9"], ["--oversample", "2"], ["--annotation", "0", "--decimate", "2"],
                  ["--shift-hz", "1", "--decimate", "2", "--oversample", "3"], ["--annotation", "0", "--taps", "5"]):
        with pytest.raises(SystemExit):
            cli.recording_tune(parse(base + flags))

    def engine(frames):
        return np.tile(np.arange(18, dtype=np.float32), (frames.shape[0], 1))
    # annotation 0 lies in the second capture (centre 101): band centre 100 -> +1 Hz, D = floor(8 / (2 * 2)) = 2
    from amcpy_amd import sigmf
    assert sigmf.tune_from_annotation(sigmf.read_meta(stem)["meta"], 0) == (1.0, 2)
    out = cli.run_recording(parse(base + ["--annotation", "0"]), compute=engine, tune_compute=ddc_ref.numpy_ddc)
    got = loadmat(out)
    T = 16 * D + 1
    n0, n1 = ((len(segs[0]) - T) // D + 1) // N, ((len(segs[1]) - T) // D + 1) // N
    assert (n0, n1) == (3, 2)
    assert got["frame_start"].ravel().tolist() == [k * N * D for k in range(n0)] + [len(segs[0]) + k * N * D for k in range(n1)]
    assert got["features"].shape == (n0 + n1, 18)
    raw = tmp_path / "raw.cu8"
    raw.write_bytes(bytes(64))
    with pytest.raises(SystemExit):                                              # a raw stream has no sample rate
        cli.run_recording(parse(["recording", str(raw), "--frame-size", "8", "--format", "cu8", "--decimate", "2"]), compute=engine)
