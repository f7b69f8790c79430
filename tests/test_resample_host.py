"""The rational resampler (include/amcx.h, ABI 13) on the host: the new symbols and their argument checks in the order the
header states, M against enumeration, the tile plan against brute force, the ratio search and the tap design, the streaming
bookkeeping over an injected numpy resampler (tests/resample_ref.py), the rational tuned path of a SigMF recording and the
command line's flags.  Needs no GPU."""
import ctypes as C
import json
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib, bank, ddc, resample as rs
from tests import bank_ref, ddc_ref, resample_ref as ref, stream_inputs

REPO = Path(__file__).resolve().parents[1]
NEW = ["amcx_resample", "amcx_resample_out_samples", "amcx_resample_plan", "amcx_kernel_name_resample"]


def test_abi_13_symbols_exist_and_bind():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 13 and lib.amcx_abi_version() >= 13
    header = (REPO / "include" / "amcx.h").read_text()
    assert "#define AMCX_ABI_VERSION 13" in header
    for older in (12, 11, 10):                                               # the live one first, the older lines kept
        assert header.index("#define AMCX_ABI_VERSION 13") < header.index(f"#define AMCX_ABI_VERSION {older}")
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    flat = " ".join(header.split())
    assert ("int64_t amcx_resample_out_samples(int64_t n_samples, int32_t n_taps, int32_t interp, int32_t decim, "
            "int32_t phase_index0);") in flat
    assert ("int amcx_resample(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, uint64_t phase0, "
            "uint64_t phase_step, const float* taps_dev, int32_t n_taps, int32_t interp, int32_t decim, int32_t phase_index0, "
            "void* out_c64_dev, int64_t out_capacity_samples, void* hip_stream);") in flat
    assert ("int amcx_resample_plan(int32_t n_taps, int32_t interp, int32_t decim, int32_t* tile_outputs, "
            "int32_t* max_span_samples, int32_t* max_workgroups, int32_t* lds_bytes);") in flat
    assert "const char* amcx_kernel_name_resample(int32_t src_kind);" in flat
    assert _lib.kernel_name_resample(_lib.SRC_C64) == "amcx_resample_c64_kernel"
    assert _lib.kernel_name_resample(_lib.SRC_SC16) == "amcx_resample_sc16_kernel"
    assert _lib.kernel_name_resample(_lib.SRC_CI8) == _lib.kernel_name_resample(_lib.SRC_CU8) == "amcx_resample_iq8_kernel"
    for kind in (_lib.SRC_C128, _lib.SRC_F32_SPLIT, 5, 10, -1):
        with pytest.raises(ValueError):
            _lib.kernel_name_resample(kind)
    # the committed resource table knows the three kernels by the names the query gives: nothing spilled
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    for name in ("amcx_resample_c64_kernel", "amcx_resample_sc16_kernel", "amcx_resample_iq8_kernel"):
        assert table[name]["spill"] == 0 and table[name]["scratch"] == 0, name


def test_out_samples_against_enumeration():
    m = _lib.load().amcx_resample_out_samples
    for T in (1, 2, 5, 7, 23):
        for L in (1, 2, 3, 5, 8):
            for D in (1, 2, 3, 7, 50):
                for tau0 in range(L):
                    for S in range(40):
                        want = ref.out_samples_brute(S, T, L, D, tau0)
                        assert m(S, T, L, D, tau0) == want == rs.out_samples(S, T, L, D, tau0) == ref.out_samples(S, T, L, D, tau0), \
                            (S, T, L, D, tau0)
    # L = 1 is the down-converter's count
    for S, T, D in ((0, 5, 3), (4, 5, 3), (5, 5, 3), (100, 5, 3), (4096, 2048, 1), ((1 << 40) - 1, 7, 4096)):
        assert m(S, T, 1, D, 0) == ddc.out_samples(S, T, D)
    assert m((1 << 40) - 1, 4096, 256, 1, 255) == ((1 << 40) - 16) * 256 - 255
    for S, T, L, D, tau0 in ((-1, 1, 1, 1, 0), (1 << 40, 1, 1, 1, 0), (10, 0, 1, 1, 0), (10, 4097, 1, 1, 0), (10, 1, 0, 1, 0),
                             (10, 1, 257, 1, 0), (10, 1, 1, 0, 0), (10, 1, 1, 4097, 0), (10, 1, 3, 1, 3), (10, 1, 3, 1, -1),
                             (10, 1, 1, 1, 1)):
        assert m(S, T, L, D, tau0) == -1, (S, T, L, D, tau0)
        with pytest.raises(ValueError):
            rs.out_samples(S, T, L, D, tau0)


PLAN_SWEEP = [(1, 1, 1), (1, 256, 1), (4096, 1, 4096), (4096, 256, 1), (4095, 7, 4096), (4096, 1, 1), (2048, 1, 1), (7, 3, 2),
              (23, 5, 3), (64, 64, 1), (33, 2, 3), (129, 7, 4096), (2561, 160, 147), (4096, 256, 255), (4096, 255, 256),
              (161, 10, 7), (257, 3, 16), (2, 3, 50), (3, 5, 3), (4096, 256, 4096), (1, 1, 4096), (4081, 255, 1)]


@pytest.mark.parametrize("T,L,D", PLAN_SWEEP)
def test_plan_spans_fit_for_every_phase(T, L, D):
    """Every tile of every call -- every tau0, and every remainder (m0 D + tau0) mod L a tile can begin at -- stages at most
    max_span_samples samples, by brute force over the definition; the LDS holds that span and the taps."""
    tile, max_span, grid, lds = _lib.resample_plan(T, L, D)
    P = ref.phase_taps(T, L)
    assert 1 <= tile <= 4096 and grid >= 1 and P <= max_span
    assert 8 * max_span + 4 * T <= lds <= 65536                          # no attribute needed
    tau0 = np.arange(L, dtype=np.int64)[:, None]
    k = np.arange(L, dtype=np.int64)[None, :]                              # the remainder's cycle is at most L tiles long
    t_first = k * tile * D + tau0                                          # the tile's first output
    t_last = t_first + (tile - 1) * D                                      # ... and its last
    span = ((P - 1) + t_last // L) - t_first // L + 1                      # newest sample of the last - oldest of the first + 1
    assert int(span.max()) <= max_span, (int(span.max()), max_span)
    # the tile is not needlessly small: one more output would not fit the stage, or the cap holds
    assert tile == 4096 or (tile * D + L - 1) // L + P > 5632


def test_plan_refusals():
    for T, L, D in ((0, 1, 1), (4097, 1, 1), (1, 0, 1), (1, 257, 1), (1, 1, 0), (1, 1, 4097)):
        with pytest.raises(ValueError):
            _lib.resample_plan(T, L, D)
    assert _lib.load().amcx_resample_plan(7, 3, 2, None, None, None, None) == _lib.OK


def test_refusals_come_in_the_documented_order_without_a_device():
    lib = _lib.load()
    f = lib.amcx_resample
    buf = (C.c_float * 256)()
    dummy = C.addressof(buf)
    dummy += -dummy % 16
    # S = 100, T = 5, L = 2, D = 3: P = 3, M = ((100 - 3 + 1) * 2 - 1) // 3 + 1 = 66
    ok = dict(src=dummy, kind=_lib.SRC_CI8, S=100, scale=2.0 ** -7, taps=dummy, T=5, L=2, D=3, tau0=0, out=dummy, cap=66)
    assert rs.out_samples(100, 5, 2, 3) == 66

    def call(**kw):
        a = {**ok, **kw}
        return f(a["src"], a["kind"], a["S"], a["scale"], 0, 1, a["taps"], a["T"], a["L"], a["D"], a["tau0"], a["out"], a["cap"], None)

    bad_ptr = dict(src=None, taps=None, out=None)
    # 1. the kind, whatever else is wrong
    for kind in (_lib.SRC_C128, _lib.SRC_F32_SPLIT, _lib.SRC_F64_SPLIT, 5, 6, 7, 10, -1):
        assert call(kind=kind) == _lib.EINVAL and call(kind=kind, S=0, **bad_ptr) == _lib.EINVAL
    # 2. the scale, for the integer kinds only -- also where the call would otherwise be the M == 0 no-op
    for kind in (_lib.SRC_SC16, _lib.SRC_CI8, _lib.SRC_CU8):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert call(kind=kind, scale=bad) == _lib.EINVAL and call(kind=kind, scale=bad, S=0, **bad_ptr) == _lib.EINVAL
    assert call(kind=_lib.SRC_C64, scale=float("nan"), S=0, **bad_ptr) == _lib.OK           # ignored for complex64
    # 3. ranges, tau0 among them, in front of the no-op
    for kw in (dict(T=0), dict(T=4097), dict(L=0), dict(L=257), dict(D=0), dict(D=4097), dict(S=-1), dict(S=1 << 40),
               dict(tau0=-1), dict(tau0=2)):
        assert call(**kw) == _lib.EINVAL and call(**{"S": 0, **kw}, **bad_ptr) == _lib.EINVAL, kw
    # 4. the capacity
    assert call(cap=65) == _lib.EINVAL and call(cap=65, **bad_ptr) == _lib.EINVAL and call(cap=-1, S=0) == _lib.EINVAL
    assert call(tau0=1, cap=64) == _lib.EINVAL and rs.out_samples(100, 5, 2, 3, 1) == 65     # tau0 counts: M = 194 // 3 + 1
    # 5. nothing to write: fine with null pointers, with any capacity >= 0
    assert call(S=2, cap=0, **bad_ptr) == _lib.OK and call(S=0, cap=0, **bad_ptr) == _lib.OK
    # 6. null pointers and alignment
    for key in ("src", "taps", "out"):
        assert call(**{key: None}) == _lib.EINVAL, key
    assert call(src=dummy + 1) == _lib.EINVAL and call(kind=_lib.SRC_CU8, src=dummy + 1) == _lib.EINVAL
    assert call(kind=_lib.SRC_SC16, src=dummy + 2) == _lib.EINVAL
    assert call(kind=_lib.SRC_C64, src=dummy + 4) == _lib.EINVAL
    assert call(taps=dummy + 2) == _lib.EINVAL and call(out=dummy + 4) == _lib.EINVAL
    # a misaligned pointer does not matter where nothing is read or written
    assert call(S=2, cap=0, src=dummy + 1, taps=dummy + 2, out=dummy + 4) == _lib.OK


def test_rational_ratio():
    # exact ratios come back in lowest terms
    for L, D in ((1, 1), (2, 3), (160, 147), (256, 255), (1, 4096), (256, 1), (20, 39), (255, 4096), (7, 4093)):
        assert rs.rational_ratio(Fraction(L, D)) == (L, D)
        assert rs.rational_ratio(Fraction(3 * L, 3 * D)) == (L, D)
    assert rs.rational_ratio(0.5) == (1, 2) and rs.rational_ratio(2) == (2, 1) and rs.rational_ratio(0.75) == (3, 4)
    assert rs.rational_ratio(48000 / 44100) == (160, 147)
    # the nearest fraction within the limits, by brute force
    rng = np.random.default_rng(5)
    ratios = [Fraction(float(r)) for r in rng.uniform(1 / 40, 16, 60)] + [Fraction(355, 113), Fraction(1, 39), Fraction(31, 2)]
    for r in ratios:
        L, D = rs.rational_ratio(r, max_interp=16, max_decim=40)
        assert 1 <= L <= 16 and 1 <= D <= 40 and np.gcd(L, D) == 1
        best = min(abs(Fraction(a, b) - r) for a in range(1, 17) for b in range(1, 41))
        assert abs(Fraction(L, D) - r) == best, (r, L, D)
    for bad in (0, -0.5, float("nan"), float("inf"), 257, Fraction(1, 4097)):
        with pytest.raises(ValueError):
            rs.rational_ratio(bad)
    with pytest.raises(ValueError):
        rs.rational_ratio(0.5, max_interp=0)
    with pytest.raises(ValueError):
        rs.rational_ratio(17, max_interp=16, max_decim=40)


def test_design_resample_lowpass():
    for L, D in ((1, 1), (1, 8), (3, 2), (2, 3), (10, 7), (160, 147), (255, 254), (5, 16)):
        h = rs.design_resample_lowpass(L, D)
        assert h.dtype == np.float32 and h.shape == (16 * max(L, D) + 1,)
        assert np.array_equal(h, h[::-1])                                    # symmetric to the bit
        assert abs(float(h.astype(np.float64).sum()) - L) < 1e-5 * L         # DC gain L
    for L in (2, 3, 10, 160, 256):                                           # 16 taps per phase: every phase passes DC alike
        h = rs.design_resample_lowpass(L, 1, 16 * L).astype(np.float64)
        sums = h.reshape(16, L).sum(axis=0)
        assert np.all(np.abs(sums - 1.0) < 0.01), (L, float(np.abs(sums - 1.0).max()))
    assert np.array_equal(rs.design_resample_lowpass(1, 4), ddc.design_lowpass(4))        # L = 1: the down-converter's design
    assert rs.design_resample_lowpass(3, 2, 33).shape == (33,)
    wide, narrow = rs.design_resample_lowpass(3, 8, 65, cutoff=0.05), rs.design_resample_lowpass(3, 8, 65, cutoff=0.02)
    assert wide[32] > narrow[32] > 0
    for kw in (dict(interp=0, decim=1), dict(interp=257, decim=1), dict(interp=1, decim=0), dict(interp=1, decim=4097),
               dict(interp=1, decim=256), dict(interp=256, decim=1), dict(interp=3, decim=2, n_taps=0),
               dict(interp=3, decim=2, n_taps=4097), dict(interp=3, decim=2, cutoff=0.0), dict(interp=3, decim=2, cutoff=0.6)):
        with pytest.raises(ValueError):
            rs.design_resample_lowpass(**kw)
    assert rs.design_resample_lowpass(256, 1, 4096).shape == (4096,)


_stream = stream_inputs.stream


def test_numpy_resample_is_the_reference_and_the_down_converter():
    from tests import ddc_ref
    rng = np.random.default_rng(3)
    x = _stream("cf32", 300, rng)
    shift = Fraction(ref.ODD_STEP, 1 << 64)
    for T, L, D, tau0 in ((7, 3, 2, 0), (7, 3, 2, 2), (23, 5, 3, 4), (3, 5, 3, 1), (2, 3, 50, 0)):
        taps = ref.make_taps(T)
        y = ref.numpy_resample(x, taps, L, D, shift=shift, sample_index0=11, phase_index0=tau0)
        y64, s = ref.reference(x.astype(np.complex128), taps, L, D, tau0, (11 * ref.ODD_STEP) & ref.MASK64, ref.ODD_STEP)
        assert y.shape == y64.shape == (ref.out_samples(300, T, L, D, tau0),)
        assert ref.worst_ratio(y, y64, s, ref.phase_taps(T, L)) <= 1.0
    taps = ref.make_taps(9)
    assert ref.numpy_resample(x, taps, 1, 4, shift=shift, sample_index0=5).tobytes() == \
        ddc_ref.numpy_ddc(x, taps, 4, shift=shift, sample_index0=5).tobytes()


def test_resampler_bookkeeping_under_random_cuts():
    """200 random cuts of random (T, L, D) -- D > P L, chunks of 0 and 1 samples among them -- equal one call bit for bit;
    the index and tau0 are what the definition says after every push."""
    rng = np.random.default_rng(17)
    shift = Fraction(ref.ODD_STEP, 1 << 64)
    cases = [(2, 3, 50), (1, 1, 1), (3, 5, 3), (7, 1, 20)]                  # D > P L; the identity; empty phases; L = 1, D > T
    while len(cases) < 200:
        L, D = int(rng.integers(1, 12)), int(rng.integers(1, 40))
        cases.append((int(rng.integers(1, 40)), L, D))
    for trial, (T, L, D) in enumerate(cases):
        fmt = ddc.FORMATS[trial % 4]
        P = ref.phase_taps(T, L)
        S = int(rng.integers(0, 6 * max(D // L + 1, P) + 60))
        x = _stream(fmt, S, rng)
        taps = ref.make_taps(T)
        scale = None if fmt == "cf32" else 0.03125
        whole = ref.numpy_resample(x, taps, L, D, shift=shift, scale=scale)
        assert whole.shape == (rs.out_samples(S, T, L, D),) and whole.dtype == np.complex64
        r = rs.Resampler(taps, L, D, shift, fmt, scale, compute=ref.numpy_resample)
        got, pos = [], 0
        while True:
            n = int(rng.choice([0, 1, 1, int(rng.integers(0, 2 * (D // L + P) + 3))]))
            y = r.push(x[pos:pos + n])
            pos = min(S, pos + n)
            got.append(y)
            done = sum(len(g) for g in got)
            # every output the data so far completes -- as if the stream ended here -- has been delivered
            assert done == rs.out_samples(pos, T, L, D), (T, L, D, pos)
            assert (r.index, r.phase_index) == divmod(done * D, L)
            assert r._skip == max(0, r.index - pos) and r._tail.shape[0] == max(0, pos - r.index)
            assert np.array_equal(r._tail, x[r.index:pos]) and y.dtype == np.complex64
            if pos == S and n > 0 or S == 0:
                break
        assert np.concatenate(got).tobytes() == whole.tobytes(), (fmt, T, L, D, trial)
    taps = ref.make_taps(5)
    with pytest.raises(TypeError):
        rs.Resampler(taps, 3, 2, shift, "ci8", compute=ref.numpy_resample).push(np.zeros((4, 3), np.int8))
    with pytest.raises(ValueError):
        rs.Resampler(taps, 3, 2, shift, "cf64")
    for L, D in ((257, 1), (0, 1), (1, 4097)):
        with pytest.raises(ValueError):
            rs.Resampler(taps, L, D, shift)
    with pytest.raises(ValueError):
        rs.Resampler(taps, 3, 2, shift, "sc16", scale=0.0)


def test_resample_type_errors_arrive_before_the_library_is_touched(monkeypatch):
    import torch

    def no_load(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "require_torch_runtime", no_load)
    taps = np.ones(3, np.float32)
    with pytest.raises(TypeError):
        rs.resample(np.zeros(8, np.complex64), taps, 3, 2)                       # not a tensor
    with pytest.raises(TypeError):
        rs.resample(torch.zeros(8, dtype=torch.complex128), taps, 3, 2)
    with pytest.raises(TypeError):
        rs.resample(torch.zeros((8, 3), dtype=torch.int8), taps, 3, 2)
    with pytest.raises(ValueError):
        rs.resample(torch.zeros(8, dtype=torch.complex64), taps, 3, 2)          # host memory
    with pytest.raises(ValueError):
        rs.resample(torch.zeros((8, 2), dtype=torch.uint8), taps, 3, 2, scale=float("nan"))


# ---- SigMF, resampled -----------------------------------------------------------------------------------------------
def _write_recording(tmp_path, segs, header_bytes, extra_global=None, captures_extra=None, annotations=None, datatype="ci8"):
    blob, captures, start = b"", [], 0
    for j, (seg, hb) in enumerate(zip(segs, header_bytes)):
        blob += b"\xee" * hb + seg.tobytes()
        cap = {"core:sample_start": start, **((captures_extra or [{}] * len(segs))[j])}
        if hb:
            cap["core:header_bytes"] = hb
        captures.append(cap)
        start += len(seg)
    stem = tmp_path / "resampled"
    Path(str(stem) + ".sigmf-data").write_bytes(blob)
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps({
        "global": {"core:datatype": datatype, "core:version": "1.0.0", **(extra_global or {})}, "captures": captures,
        "annotations": annotations or []}))
    return stem


def test_annotation_gives_the_ratio_asked_for():
    from amcpy_amd import sigmf
    fs = 20e6
    bw = fs / 3.9                                              # the integer path: floor(3.9 / 2) = 1, 3.9x oversampled
    meta = {"global": {"core:sample_rate": fs}, "captures": [{"core:sample_start": 0, "core:frequency": 100e6}],
            "annotations": [{"core:sample_start": 10, "core:freq_lower_edge": 103e6 - bw / 2, "core:freq_upper_edge": 103e6 + bw / 2}]}
    shift_hz, D = sigmf.tune_from_annotation(meta, 0, 2)
    assert D == 1 and shift_hz == pytest.approx(-3e6)
    shift_r, (L, D) = sigmf.tune_from_annotation(meta, 0, 2, rational=True)
    assert shift_r == shift_hz and 1 <= L <= 256 and 1 <= D <= 4096 and np.gcd(L, D) == 1
    assert abs(L / D - 2 * bw / fs) <= 0.005 * 2 * bw / fs
    assert sigmf.tune_from_annotation(meta, 0, 2.0, rational=False) == (shift_hz, 1)      # the default stays
    shift, L2, D2, taps = sigmf.resolve_resample(meta, {"annotation": 0, "oversample": 2, "rational": True})
    assert (L2, D2) == (L, D) and shift == Fraction(shift_hz) / Fraction(fs)
    assert np.array_equal(taps, rs.design_resample_lowpass(L, D))
    shift, L2, D2, taps = sigmf.resolve_resample(meta, {"shift_hz": 5e6, "resample": (3, 4), "taps": 33})
    assert (shift, L2, D2) == (Fraction(1, 4), 3, 4) and np.array_equal(taps, rs.design_resample_lowpass(3, 4, 33))
    assert sigmf.resolve_resample({"global": {}}, {"resample": (2, 3), "taps": [0.5, 1.0, 0.5]})[3].tolist() == [0.5, 1.0, 0.5]
    for bad in ({"annotation": 0, "rational": True, "resample": (2, 3)}, {"shift_hz": 1.0, "rational": True},
                {"resample": (2, 3), "decimate": 2}, {"resample": (0, 3)}, {"resample": (2, 3), "x": 1}):
        with pytest.raises(ValueError):
            sigmf.resolve_resample(meta, bad)
    assert sigmf.is_rational_tune({"resample": (2, 3)}) and sigmf.is_rational_tune({"annotation": 0, "rational": True})
    assert not sigmf.is_rational_tune({"annotation": 0}) and not sigmf.is_rational_tune({"annotation": 0, "rational": False})


@pytest.mark.parametrize("datatype", ["ci8", "cu8", "ci16_le", "cf32_le"])
def test_sigmf_resampled_with_injected_computes(tmp_path, datatype):
    from amcpy_amd import sigmf
    rng = np.random.default_rng(23)
    fmt = sigmf.DATATYPES[datatype][0]
    N, L, D, T = 8, 3, 5, 11
    lens = [131, 97]
    segs = [_stream(fmt, n, rng) for n in lens]
    stem = _write_recording(tmp_path, segs, [0, 6], {"core:sample_rate": 8.0}, datatype=datatype)
    taps = ref.make_taps(T)
    tune = {"shift_hz": 1.0, "resample": (L, D), "taps": taps}                   # an eighth of a turn per sample
    seen = []

    def engine(frames):
        seen.append(np.array(frames))
        return np.full((frames.shape[0], 18), float(len(seen)), np.float32)
    scale = None if fmt == "cf32" else sigmf.DATATYPES[datatype][2]
    per_seg = [ref.numpy_resample(seg, taps, L, D, shift=0.125, scale=scale) for seg in segs]
    n_frames = [len(y) // N for y in per_seg]
    assert n_frames == [rs.out_samples(n, T, L, D) // N for n in lens] and min(n_frames) >= 2
    want_start = [k * N * D // L for k in range(n_frames[0])] + [lens[0] + k * N * D // L for k in range(n_frames[1])]
    for chunk in (1 << 24, 13, 1):                                               # however the segment is read
        seen.clear()
        feats, frame_start = sigmf.extract_sigmf(stem, N, tune=tune, compute=engine, tune_compute=ref.numpy_resample,
                                                 chunk_samples=chunk)
        assert feats.shape == (sum(n_frames), 18) and feats.dtype == np.float32 and frame_start.dtype == np.int64
        assert frame_start.tolist() == want_start
        assert feats[:, 0].tolist() == [1.0] * n_frames[0] + [2.0] * n_frames[1]         # one feature call per capture
        assert len(seen) == 2
        for got, y, n in zip(seen, per_seg, n_frames):                           # no frame holds a sample of the other capture
            assert got.dtype == np.complex64 and got.shape == (n, N) and got.tobytes() == y[:n * N].tobytes()
    feats, frame_start = sigmf.extract_sigmf(stem, N, tune=tune, compute=engine, tune_compute=ref.numpy_resample,
                                             max_frames=n_frames[0] + 1, chunk_samples=17)
    assert frame_start.tolist() == want_start[:n_frames[0] + 1]
    # an existing tune dict still goes through the down-converter
    from tests import ddc_ref
    old = {"shift_hz": 1.0, "decimate": 3, "taps": ref.make_taps(7)}
    seen.clear()
    feats, frame_start = sigmf.extract_sigmf(stem, N, tune=old, compute=engine, tune_compute=ddc_ref.numpy_ddc)
    assert seen[0].tobytes() == ddc_ref.numpy_ddc(segs[0], old["taps"], 3, shift=0.125, scale=scale)[:seen[0].size].tobytes()
    assert frame_start[:2].tolist() == [0, N * 3]


def test_recording_command_resampling_flags(tmp_path):
    from scipy.io import loadmat
    from amcpy_amd import main as cli, sigmf
    rng = np.random.default_rng(24)
    N = 8
    segs = [_stream("ci8", 300, rng), _stream("ci8", 200, rng)]
    # the band is 8 / 3.9 Hz wide at 2x oversampling: the integer path gives D = 1, the rational one 20 / 39
    bw = 8.0 / 3.9
    ann = [{"core:sample_start": len(segs[0]) + 1, "core:freq_lower_edge": 100.0 - bw / 2, "core:freq_upper_edge": 100.0 + bw / 2}]
    stem = _write_recording(tmp_path, segs, [0, 2], {"core:sample_rate": 8.0},
                            [{"core:frequency": 90.0}, {"core:frequency": 101.0}], ann)
    parse = cli.build_parser().parse_args
    base = ["recording", str(stem), "--frame-size", str(N)]
    assert cli.recording_tune(parse(base + ["--resample", "3/4"])) == {"shift_hz": 0.0, "resample": (3, 4), "taps": None}
    assert cli.recording_tune(parse(base + ["--shift-hz", "-2.5", "--resample", "160/147", "--taps", "33"])) == \
        {"shift_hz": -2.5, "resample": (160, 147), "taps": 33}
    assert cli.recording_tune(parse(base + ["--annotation", "0", "--rational"])) == {"annotation": 0, "oversample": 2.0, "rational": True}
    assert cli.recording_tune(parse(base + ["--annotation", "0", "--oversample", "1.5", "--rational"])) == \
        {"annotation": 0, "oversample": 1.5, "rational": True}
    assert cli.recording_tune(parse(base + ["--annotation", "0"])) == {"annotation": 0, "oversample": 2.0}       # as before
    for flags in (["--rational"], ["--resample", "3"], ["--resample", "a/b"], ["--resample", "3/4", "--decimate", "2"],
                  ["--resample", "3/4", "--rational"], ["--resample", "3/4", "--annotation", "0"],
                  ["--channels", "4", "--resample", "3/4"], ["--channels", "4", "--rational"]):
        with pytest.raises(SystemExit):
            cli.recording_tune(parse(base + flags))

    def engine(frames):
        return np.tile(np.arange(18, dtype=np.float32), (frames.shape[0], 1))
    shift_hz, (L, D) = sigmf.tune_from_annotation(sigmf.read_meta(stem)["meta"], 0, rational=True)
    assert shift_hz == pytest.approx(1.0) and abs(L / D - 2 / 3.9) < 0.005 * 2 / 3.9
    out = cli.run_recording(parse(base + ["--annotation", "0", "--rational"]), compute=engine, tune_compute=ref.numpy_resample)
    got = loadmat(out)
    assert int(got["interp"].ravel()[0]) == L and int(got["decim"].ravel()[0]) == D
    T = 16 * max(L, D) + 1
    n0, n1 = rs.out_samples(len(segs[0]), T, L, D) // N, rs.out_samples(len(segs[1]), T, L, D) // N
    assert n0 >= 2 and n1 >= 1
    assert got["frame_start"].ravel().tolist() == [k * N * D // L for k in range(n0)] + [len(segs[0]) + k * N * D // L for k in range(n1)]
    assert got["features"].shape == (n0 + n1, 18)
    out = cli.run_recording(parse(base + ["--resample", "2/3", "--taps", "9", "--out", str(tmp_path / "m.mat")]), compute=engine,
                            tune_compute=ref.numpy_resample)
    got = loadmat(out)
    assert int(got["interp"].ravel()[0]) == 2 and int(got["decim"].ravel()[0]) == 3 and got["frame_start"].ravel()[1] == N * 3 // 2


def test_annotation_ratio_always_has_a_filter(tmp_path):
    """A band that is no neat fraction of fs: the ratio the annotation form picks stays within 255 / 255, so the default taps
    exist, and it is close to what was asked -- for 0.123 and for a sweep of ratios from 0.05 up; through resolve_resample
    and through the command."""
    from scipy.io import loadmat
    from amcpy_amd import main as cli, sigmf
    assert rs.DESIGN_MAX == 255 and 16 * rs.DESIGN_MAX + 1 <= rs.MAX_TAPS < 16 * (rs.DESIGN_MAX + 1) + 1
    L, D = rs.rational_ratio(0.123)                           # the kernel's limits: no default design for this one
    assert max(L, D) > rs.DESIGN_MAX
    with pytest.raises(ValueError, match="rational_ratio"):
        rs.design_resample_lowpass(L, D)
    fs = 20e6

    def meta_for(ratio, oversample=2.0):
        bw = ratio * fs / oversample
        return {"global": {"core:sample_rate": fs}, "captures": [{"core:sample_start": 0, "core:frequency": 100e6}],
                "annotations": [{"core:sample_start": 0, "core:freq_lower_edge": 101e6 - bw / 2, "core:freq_upper_edge": 101e6 + bw / 2}]}
    rng = np.random.default_rng(9)
    worst = 0.0
    for ratio in [0.123] + rng.uniform(0.05, 1.0, 300).tolist() + rng.uniform(1.0, 8.0, 20).tolist():
        shift, L, D, taps = sigmf.resolve_resample(meta_for(ratio), {"annotation": 0, "oversample": 2.0, "rational": True})
        assert 1 <= L <= 255 and 1 <= D <= 255 and taps.shape == (16 * max(L, D) + 1,)
        worst = max(worst, abs(L / D - ratio) / ratio)
    assert worst <= 0.002, worst                              # |L / D - r| <= 1 / (2 * 255 * D), D about L / r: 0.2 % at r >= 0.05 ...
    assert sigmf.tune_from_annotation(meta_for(0.123), 0, 2.0, rational=True)[1] == rs.rational_ratio(
        Fraction(2.0) * Fraction(meta_for(0.123)["annotations"][0]["core:freq_upper_edge"]
                                 - meta_for(0.123)["annotations"][0]["core:freq_lower_edge"]) / Fraction(fs), 255, 255)
    # the annotation form takes taps too: a count, or the taps
    assert sigmf.resolve_resample(meta_for(0.123), {"annotation": 0, "rational": True, "taps": 99})[3].shape == (99,)
    with pytest.raises(ValueError):                           # narrower than fs / (255 * oversample): no fraction within 255 / 255
        sigmf.resolve_resample(meta_for(1 / 300), {"annotation": 0, "rational": True})
    # ... and the command: a recording whose annotation asks for 0.123
    rng = np.random.default_rng(25)
    N = 8
    segs = [_stream("ci8", 9000, rng)]
    m = meta_for(0.123)
    stem = _write_recording(tmp_path, segs, [0], {"core:sample_rate": fs}, [{"core:frequency": 100e6}], m["annotations"])

    def engine(frames):
        return np.zeros((frames.shape[0], 18), np.float32)
    _, L, D, taps = sigmf.resolve_resample(m, {"annotation": 0, "rational": True})
    args = cli.build_parser().parse_args(["recording", str(stem), "--frame-size", str(N), "--annotation", "0", "--rational"])
    got = loadmat(cli.run_recording(args, compute=engine, tune_compute=ref.numpy_resample))
    assert (int(got["interp"].ravel()[0]), int(got["decim"].ravel()[0])) == (L, D) and abs(L / D - 0.123) <= 0.002 * 0.123
    n = rs.out_samples(9000, taps.shape[0], L, D) // N
    assert n >= 2 and got["features"].shape == (n, 18) and got["frame_start"].ravel().tolist() == [k * N * D // L for k in range(n)]


def test_a_resolved_tune_is_taken_back_and_pushes_that_complete_nothing_do_not_launch():
    from amcpy_amd import sigmf
    resolved = sigmf.resolve_resample({"global": {}}, {"resample": (2, 3), "taps": [0.5, 1.0, 0.5]})
    assert sigmf.is_rational_tune(resolved) and sigmf.resolve_resample({"global": {}}, resolved) is resolved
    calls = []

    def counting(x, *a, **kw):
        calls.append(int(x.shape[0]))
        return ref.numpy_resample(x, *a, **kw)
    taps = ref.make_taps(7)                                   # L = 2: P = 4 -- three samples complete nothing
    r = rs.Resampler(taps, 2, 9, 0.0, "cf32", compute=counting)
    x = np.arange(40, dtype=np.complex64)
    for j in range(3):
        y = r.push(x[j:j + 1])
        assert y.shape == (0,) and y.dtype == np.complex64 and not calls and r._tail.shape == (j + 1,)
    assert r.push(x[3:5]).shape == (1,) and calls == [5]      # one output; the next window begins 4 samples on: one more to drop
    assert (r.index, r.phase_index, r._skip) == (4, 1, 0) and r._tail.shape == (1,)
    whole = ref.numpy_resample(x, taps, 2, 9)
    rest = r.push(x[5:])
    assert np.concatenate([whole[:1], rest]).tobytes() == whole.tobytes()


# ---- what the three stream modules share (amcpy_amd/_stream.py): taps and bookkeeping as recorded before they shared it ----
_DESIGNS = {
    "lowpass_d1": lambda: ddc.design_lowpass(1),                                  # the defaults at D = 1 and D = 7
    "lowpass_d7": lambda: ddc.design_lowpass(7),
    "lowpass_d4_t1": lambda: ddc.design_lowpass(4, 1),                            # T = 1, an even T, an odd T with a cutoff
    "lowpass_d4_t64": lambda: ddc.design_lowpass(4, 64),
    "lowpass_d3_t33_cut": lambda: ddc.design_lowpass(3, 33, cutoff=0.11),
    "bank_c2_p1": lambda: bank.design_bank_lowpass(2, 1),
    "bank_c8": lambda: bank.design_bank_lowpass(8),
    "bank_c64_p5_d32": lambda: bank.design_bank_lowpass(64, 5, 32),
    "resample_1_1": lambda: rs.design_resample_lowpass(1, 1),
    "resample_1_7": lambda: rs.design_resample_lowpass(1, 7),
    "resample_3_2": lambda: rs.design_resample_lowpass(3, 2),
    "resample_255_254": lambda: rs.design_resample_lowpass(255, 254),
    "resample_3_2_t1": lambda: rs.design_resample_lowpass(3, 2, 1),
    "resample_3_2_t64": lambda: rs.design_resample_lowpass(3, 2, 64),
    "resample_10_7_t161_cut": lambda: rs.design_resample_lowpass(10, 7, 161, cutoff=0.03),
}


def test_design_functions_return_the_recorded_taps_bit_for_bit():
    gold = np.load(REPO / "tests" / "golden" / "stream_design_taps.npz")
    assert sorted(gold.files) == sorted(_DESIGNS)
    for name, design in _DESIGNS.items():
        h = design()
        assert h.dtype == np.float32 == gold[name].dtype and h.tobytes() == gold[name].tobytes(), name


# (index, _skip, tail length[, phase_index]) after each push of 0, 1, T - 1, T + D, 1, 0, T + D, T - 1, T + D, 1 samples
_STATES = [
    (lambda: ddc.Channelizer(ddc_ref.make_taps(5), 3, 0.1, compute=ddc_ref.numpy_ddc), 5, 3,
     [(0, 0, 0), (0, 0, 1), (3, 0, 2), (9, 0, 4), (12, 0, 2), (12, 0, 2), (18, 0, 4), (24, 0, 2), (30, 0, 4), (33, 0, 2)]),
    (lambda: ddc.Channelizer(ddc_ref.make_taps(3), 7, 0.1, compute=ddc_ref.numpy_ddc), 3, 7,                  # decim > T
     [(0, 0, 0), (0, 0, 1), (7, 4, 0), (14, 1, 0), (14, 0, 0), (14, 0, 0), (28, 4, 0), (28, 2, 0), (35, 0, 1), (35, 0, 2)]),
    (lambda: bank.FilterBank(ddc_ref.make_taps(6), 4, 2, 0.1, compute=bank_ref.numpy_bank), 6, 2,
     [(0, 0, 0), (0, 0, 1), (2, 0, 4), (10, 0, 4), (10, 0, 5), (10, 0, 5), (18, 0, 5), (24, 0, 4), (32, 0, 4), (32, 0, 5)]),
    (lambda: bank.FilterBank(ddc_ref.make_taps(2), 8, 8, 0.1, compute=bank_ref.numpy_bank), 2, 8,             # decim > T
     [(0, 0, 0), (0, 0, 1), (8, 6, 0), (16, 4, 0), (16, 3, 0), (16, 3, 0), (24, 1, 0), (24, 0, 0), (40, 6, 0), (40, 5, 0)]),
    (lambda: rs.Resampler(ddc_ref.make_taps(7), 3, 2, 0.1, compute=ref.numpy_resample), 7, 2,
     [(0, 0, 0, 0), (0, 0, 1, 0), (5, 0, 2, 1), (14, 0, 2, 0), (15, 0, 2, 1), (15, 0, 2, 1), (24, 0, 2, 0), (30, 0, 2, 0),
      (39, 0, 2, 1), (40, 0, 2, 0)]),
    (lambda: rs.Resampler(ddc_ref.make_taps(4), 2, 9, 0.1, compute=ref.numpy_resample), 4, 9,                 # decim > P interp
     [(0, 0, 0, 0), (0, 0, 1, 0), (4, 0, 0, 1), (18, 1, 0, 0), (18, 0, 0, 0), (18, 0, 0, 0), (31, 0, 0, 1), (36, 2, 0, 0),
      (49, 2, 0, 1), (49, 1, 0, 1)]),
]


@pytest.mark.parametrize("case", range(len(_STATES)))
def test_streaming_state_after_every_push_is_the_recorded_one(case):
    make, T, D, want = _STATES[case]
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(400) + 1j * rng.standard_normal(400)).astype(np.complex64)
    s, pos = make(), 0
    for n, state in zip((0, 1, T - 1, T + D, 1, 0, T + D, T - 1, T + D, 1), want):
        s.push(x[pos:pos + n])
        pos += n
        got = (s.index, s._skip, int(s._tail.shape[0])) + ((s.phase_index,) if isinstance(s, rs.Resampler) else ())
        assert got == state, (case, pos)
