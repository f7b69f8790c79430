"""The polyphase filter bank (include/amcx.h, ABI 12) on the host: the new symbols and their argument checks in the order the
header states, the plan, the prototype filter, the channel raster, the streaming bookkeeping over an injected numpy bank
(tests/bank_ref.py), the channelized path of a SigMF recording and the command line's flags.  Needs no GPU."""
import ctypes as C
import json
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib, bank, ddc
from tests import bank_ref, ddc_ref, stream_inputs

REPO = Path(__file__).resolve().parents[1]
NEW = ["amcx_filter_bank", "amcx_filter_bank_out_samples", "amcx_filter_bank_plan", "amcx_kernel_name_bank"]
KERNELS = ("amcx_bank_c64_kernel", "amcx_bank_sc16_kernel", "amcx_bank_iq8_kernel")


def test_abi_12_symbols_exist_and_bind():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 12 and lib.amcx_abi_version() >= 12
    header = (REPO / "include" / "amcx.h").read_text()
    assert "#define AMCX_ABI_VERSION 12" in header
    for older in (11, 10):                                                       # the live one first
        assert header.index("#define AMCX_ABI_VERSION 12") < header.index(f"#define AMCX_ABI_VERSION {older}")
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    flat = " ".join(header.split())
    assert "int64_t amcx_filter_bank_out_samples(int64_t n_samples, int32_t n_taps, int32_t channels, int32_t decim);" in flat
    assert ("int amcx_filter_bank(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, uint64_t phase0, "
            "uint64_t phase_step, uint64_t sample_index0, const float* taps_dev, int32_t n_taps, int32_t channels, int32_t decim, "
            "void* out_c64_dev, int64_t out_channel_stride, int64_t out_capacity_samples, void* hip_stream);") in flat
    assert ("int amcx_filter_bank_plan(int32_t n_taps, int32_t channels, int32_t decim, int32_t* tile_outputs, "
            "int32_t* max_workgroups, int32_t* lds_bytes);") in flat
    assert "int amcx_kernel_name_bank(int32_t src_kind, char* buf, int32_t buf_len);" in flat
    assert _lib.SIGNATURES["amcx_filter_bank"][1] == [C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint64, C.c_uint64,
                                                      C.c_uint64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                      C.c_int64, C.c_int64, C.c_void_p]
    assert _lib.kernel_name_bank(_lib.SRC_C64) == KERNELS[0]
    assert _lib.kernel_name_bank(_lib.SRC_SC16) == KERNELS[1]
    assert _lib.kernel_name_bank(_lib.SRC_CI8) == _lib.kernel_name_bank(_lib.SRC_CU8) == KERNELS[2]
    for kind in (_lib.SRC_C128, _lib.SRC_F32_SPLIT, 5, 10, -1):
        with pytest.raises(ValueError):
            _lib.kernel_name_bank(kind)


def test_resource_table_lists_the_three_kernels_without_spills():
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    for name in KERNELS:
        assert table[name]["spill"] == 0 and table[name]["scratch"] == 0, name


SHAPES = [(1, 2, 1), (5, 2, 2), (4, 4, 4), (19, 8, 5), (64, 8, 8), (128, 8, 4), (4096, 2, 2), (4096, 8, 8), (200, 64, 32),
          (1024, 64, 64), (513, 256, 256), (2048, 256, 128), (4096, 256, 128), (4096, 256, 256), (4096, 256, 1), (1, 256, 256),
          # log2 C = 4, 5 and 7 (tests/test_gpu_bank.py), and the largest tap counts at every C (tests/chain_exact.py)
          (37, 16, 16), (256, 16, 11), (37, 16, 11), (256, 16, 16), (100, 32, 32), (1024, 32, 24), (300, 128, 128), (2048, 128, 96),
          (300, 128, 96), (512, 128, 128), (4096, 2, 1), (4095, 2, 2), (4096, 4, 4), (4093, 4, 3), (4096, 16, 16), (4095, 32, 32),
          (4096, 128, 96)]


def test_out_samples_and_plan():
    lib = _lib.load()
    m = lib.amcx_filter_bank_out_samples
    for T, Cn, D in SHAPES:
        assert [m(S, T, Cn, D) for S in (0, T - 1, T, T + D - 1, T + D)] == [0, 0, 1, 1, 2], (T, Cn, D)
        assert m(T + 1000 * D, T, Cn, D) == 1001 and m((1 << 40) - 1, T, Cn, D) == ((1 << 40) - 1 - T) // D + 1
        assert [bank.out_samples(S, T, Cn, D) for S in (T - 1, T, T + D - 1, T + D)] == [0, 1, 1, 2]
    bad = [(-1, 1, 2, 1), (1 << 40, 1, 2, 1), (10, 0, 2, 1), (10, 4097, 2, 1), (10, 1, 2, 0), (10, 1, 2, 3), (10, 1, 256, 257),
           (10, 1, 1, 1), (10, 1, 0, 1), (10, 1, 3, 1), (10, 1, 48, 4), (10, 1, 512, 4), (10, 1, -4, 1), (10, -1, 4, 1)]
    for S, T, Cn, D in bad:
        assert m(S, T, Cn, D) == -1, (S, T, Cn, D)
        with pytest.raises(ValueError):
            bank.out_samples(S, T, Cn, D)
    for T, Cn, D in SHAPES:
        tile, grid, lds = _lib.filter_bank_plan(T, Cn, D)
        assert tile >= 8 and grid >= 1, (T, Cn, D)                        # tile >= 8 fits everywhere
        span = (tile - 1) * D + T
        # the tile's span of mixed samples, the tile x C array, the taps: all within what the plan reports, within a CU's LDS
        assert 8 * span + 8 * tile * Cn + 4 * T <= lds <= 160 * 1024, (T, Cn, D, tile, lds)
    # the largest request of any shape is C = 2, T = 4096, D = 2 (amcx_bank_kernel.h): 131 072 bytes
    assert _lib.filter_bank_plan(4096, 2, 2)[2] == 131072
    assert max(_lib.filter_bank_plan(4096, Cn, D)[2] for Cn in (2, 4, 8, 16, 32, 64, 128, 256) for D in (1, 2, Cn // 2, Cn)) == 131072
    # C = 128 is the one channel count whose tile is 32 (tests/test_gpu_bank.py runs it)
    assert _lib.filter_bank_plan(300, 128, 96)[0] == 32 and _lib.filter_bank_plan(4096, 128, 128)[0] == 32
    for T, Cn, D in ((0, 2, 1), (4097, 2, 1), (1, 2, 0), (1, 2, 3), (1, 3, 1), (1, 512, 1), (1, 1, 1)):
        with pytest.raises(ValueError):
            _lib.filter_bank_plan(T, Cn, D)
    lib.amcx_filter_bank_plan(16, 4, 4, None, None, None)                  # any pointer may be NULL


def test_refusals_come_in_the_documented_order_without_a_device():
    lib = _lib.load()
    f = lib.amcx_filter_bank
    buf = (C.c_float * 256)()
    dummy = C.addressof(buf)
    dummy += -dummy % 16
    # M = (100 - 6) // 3 + 1 = 32, C = 4: the capacity is 3 * 40 + 32 = 152
    ok = dict(src=dummy, kind=_lib.SRC_CI8, S=100, scale=2.0 ** -7, taps=dummy, T=6, Cn=4, D=3, out=dummy, stride=40, cap=152)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["src"], a["kind"], a["S"], a["scale"], 0, 1, 5, a["taps"], a["T"], a["Cn"], a["D"], a["out"], a["stride"],
                 a["cap"], None)

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
    for kw in (dict(Cn=0), dict(Cn=1), dict(Cn=3), dict(Cn=6), dict(Cn=512), dict(T=0), dict(T=4097), dict(D=0), dict(D=5),
               dict(S=-1), dict(S=1 << 40)):
        assert call(**kw) == _lib.EINVAL and call(**{"S": 0, **kw}, **bad_ptr) == _lib.EINVAL, kw
    # 4. the stride, then the capacity of the whole buffer
    assert call(stride=31, cap=1000) == _lib.EINVAL and call(stride=31, cap=1000, **bad_ptr) == _lib.EINVAL
    assert call(stride=-1, S=0, cap=1000) == _lib.EINVAL
    assert call(cap=151) == _lib.EINVAL and call(cap=151, **bad_ptr) == _lib.EINVAL and call(cap=-1, S=0, stride=0) == _lib.EINVAL
    assert call(stride=32, cap=127) == _lib.EINVAL
    assert call(stride=1 << 62, cap=(1 << 63) - 1) == _lib.EINVAL            # (C - 1) stride + M does not fit an int64
    # 5. nothing to write: fine with null pointers, with any stride >= 0 whose buffer the capacity holds
    assert call(S=5, stride=0, cap=0, **bad_ptr) == _lib.OK and call(S=0, stride=0, cap=0, **bad_ptr) == _lib.OK
    assert call(S=5, stride=7, cap=21, **bad_ptr) == _lib.OK and call(S=5, stride=7, cap=20, **bad_ptr) == _lib.EINVAL
    # 6. null pointers and alignment
    for key in ("src", "taps", "out"):
        assert call(**{key: None}) == _lib.EINVAL, key
    assert call(src=dummy + 1) == _lib.EINVAL and call(kind=_lib.SRC_CU8, src=dummy + 1) == _lib.EINVAL
    assert call(kind=_lib.SRC_SC16, src=dummy + 2) == _lib.EINVAL
    assert call(kind=_lib.SRC_C64, src=dummy + 4) == _lib.EINVAL
    assert call(taps=dummy + 2) == _lib.EINVAL and call(out=dummy + 4) == _lib.EINVAL
    # a misaligned pointer does not matter where nothing is read or written
    assert call(S=5, stride=0, cap=0, src=dummy + 1, taps=dummy + 2, out=dummy + 4) == _lib.OK


def test_design_bank_lowpass():
    for Cn, P in ((2, 16), (8, 16), (64, 16), (256, 16), (16, 8), (4, 32)):
        h = bank.design_bank_lowpass(Cn, P)
        assert h.dtype == np.float32 and h.shape == (Cn * P,)
        assert np.array_equal(h, h[::-1])
        assert abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
        n = np.arange(h.shape[0])
        gain = lambda f: abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f * n)))
        assert gain(0.5 / Cn) == pytest.approx(0.5, abs=0.02)              # the -6 dB edge at half the channel spacing
        if P >= 16:
            assert gain(0.2 / Cn) > 0.99
        for f in (1.0 / Cn, 1.25 / Cn, 1.5 / Cn):                         # the neighbour's centre and beyond: 40 dB down
            if f <= 0.5:
                assert gain(f) < 0.01, (Cn, P, f, gain(f))
    assert bank.design_bank_lowpass(8).shape == (128,) and bank.design_bank_lowpass(8, decim=4).shape == (128,)
    for kw in (dict(channels=3), dict(channels=512), dict(channels=1), dict(channels=8, taps_per_channel=0),
               dict(channels=256, taps_per_channel=17), dict(channels=8, decim=9), dict(channels=8, decim=0)):
        with pytest.raises(ValueError):
            bank.design_bank_lowpass(**kw)


def test_channel_frequencies():
    f = bank.channel_frequencies(8)
    assert f.dtype == np.float64 and f.tolist() == [0.0, 0.125, 0.25, 0.375, -0.5, -0.375, -0.25, -0.125]
    assert np.array_equal(f, np.fft.fftfreq(8))
    assert bank.channel_frequencies(4, 20e6, 100e6).tolist() == [100e6, 105e6, 90e6, 95e6]
    # the pre-mixer moves the input UP by the shift: channel c holds what was at c / C - shift; half a channel
    assert bank.channel_frequencies(4, 8.0, 0.0, shift=Fraction(1, 8)).tolist() == [-1.0, 1.0, 3.0, -3.0]
    assert bank.channel_frequencies(2, 1.0, 0.0, shift=0.25).tolist() == [-0.25, 0.25]
    assert bank.channel_frequencies(4, 1.0, 0.0, shift=1.0).tolist() == bank.channel_frequencies(4).tolist()
    for bad in (3, 0, 512):
        with pytest.raises(ValueError):
            bank.channel_frequencies(bad)


_stream = stream_inputs.stream


def test_numpy_bank_is_the_reference():
    """the injected bank of the tests below computes what the definition says: every channel against the float64 reference"""
    rng = np.random.default_rng(5)
    for T, Cn, D, index0 in ((1, 2, 1, 3), (5, 2, 2, 1), (19, 8, 5, 11), (40, 8, 8, 5), (3, 4, 4, 2)):
        x = _stream("ci8", 6 * D + T + 3, rng)
        taps = ddc_ref.make_taps(T)
        shift = Fraction(ddc_ref.ODD_STEP, 1 << 64)
        y = bank_ref.numpy_bank(x, taps, Cn, D, shift=shift, sample_index0=index0, scale=0.5)
        p0 = (index0 * ddc_ref.ODD_STEP) & ddc_ref.MASK64
        y64, s = bank_ref.reference(ddc_ref.widen(x, "ci8", 0.5), taps, Cn, D, p0, ddc_ref.ODD_STEP, index0)
        assert y.shape == y64.shape == (Cn, bank.out_samples(x.shape[0], T, Cn, D))
        assert bank_ref.worst_ratio(y, y64, s, T, Cn) <= 1.0, (T, Cn, D)          # (float64 arithmetic rounded once: far below)
        # the reference the GPU tests use is the definition -- one down-converter per channel -- with the shared work done once
        d64, ds = bank_ref.reference_by_definition(ddc_ref.widen(x, "ci8", 0.5), taps, Cn, D, p0, ddc_ref.ODD_STEP, index0)
        assert np.allclose(s, ds, rtol=1e-13, atol=0) and float(np.max(np.abs(y64 - d64) / s)) < 1e-12, (T, Cn, D)
        some = bank_ref.reference(ddc_ref.widen(x, "ci8", 0.5), taps, Cn, D, p0, ddc_ref.ODD_STEP, index0, channels=[Cn - 1, 0])[0]
        assert np.array_equal(some, y64[[Cn - 1, 0]])


@pytest.mark.parametrize("fmt", ddc.FORMATS)
@pytest.mark.parametrize("T,Cn,D", [(1, 2, 1), (7, 4, 3), (3, 8, 8), (33, 8, 4)])
def test_filter_bank_bookkeeping(fmt, T, Cn, D):
    """Random chunk lengths -- 0, 1 and below T among them -- give the one-call result bit for bit, and the tail and the
    absolute index are what the definition says."""
    rng = np.random.default_rng(100 * T + D)
    S = 40 * D + 3 * T + 11
    x = _stream(fmt, S, rng)
    taps = ddc_ref.make_taps(T)
    shift = Fraction(ddc_ref.ODD_STEP, 1 << 64)
    scale = None if fmt == "cf32" else 0.03125
    whole = bank_ref.numpy_bank(x, taps, Cn, D, shift=shift, scale=scale)
    assert whole.shape == (Cn, bank.out_samples(S, T, Cn, D)) and whole.dtype == np.complex64
    for trial in range(3):
        cuts = [0, 0, 1, 1, T - 1, T - 1] + rng.integers(0, 3 * D + T, 200).tolist()
        rng.shuffle(cuts)
        fb = bank.FilterBank(taps, Cn, D, shift, fmt, scale, compute=bank_ref.numpy_bank)
        got, pos = [], 0
        for n in cuts:
            y = fb.push(x[pos:pos + n])
            pos = min(S, pos + n)
            got.append(y)
            done = sum(g.shape[1] for g in got)
            assert y.shape[0] == Cn and y.dtype == np.complex64
            assert done == bank.out_samples(pos, T, Cn, D) and fb.index == done * D
            assert fb._tail.shape[0] == max(0, pos - fb.index) and np.array_equal(fb._tail, x[fb.index:pos])
            if pos == S:
                break
        assert pos == S
        assert np.concatenate(got, axis=1).tobytes() == whole.tobytes(), (fmt, T, Cn, D, trial)
    with pytest.raises(TypeError):
        bank.FilterBank(taps, Cn, D, shift, fmt, scale, compute=bank_ref.numpy_bank).push(np.zeros((4, 3), np.int8))
    with pytest.raises(ValueError):
        bank.FilterBank(taps, Cn, D, shift, "cf64")
    for bad in (dict(channels=3, decim=1), dict(channels=Cn, decim=Cn + 1), dict(channels=512, decim=1)):
        with pytest.raises(ValueError):
            bank.FilterBank(taps, bad["channels"], bad["decim"], shift, fmt)
    if fmt != "cf32":
        with pytest.raises(ValueError):
            bank.FilterBank(taps, Cn, D, shift, fmt, scale=0.0)


def test_filter_bank_type_errors_arrive_before_the_library_is_touched(monkeypatch):
    import torch

    def no_load(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "require_torch_runtime", no_load)
    taps = np.ones(3, np.float32)
    with pytest.raises(TypeError):
        bank.filter_bank(np.zeros(8, np.complex64), taps, 2, 1)                       # not a tensor
    with pytest.raises(TypeError):
        bank.filter_bank(torch.zeros(8, dtype=torch.complex128), taps, 2, 1)
    with pytest.raises(TypeError):
        bank.filter_bank(torch.zeros((8, 3), dtype=torch.int8), taps, 2, 1)
    with pytest.raises(ValueError):
        bank.filter_bank(torch.zeros(8, dtype=torch.complex64), taps, 2, 1)          # host memory


# ---- SigMF, channelized ---------------------------------------------------------------------------------------------
def _write_recording(tmp_path, segs, header_bytes, extra_global=None, captures_extra=None, datatype="ci8"):
    blob, captures, start = b"", [], 0
    for j, (seg, hb) in enumerate(zip(segs, header_bytes)):
        blob += b"\xee" * hb + seg.tobytes()
        cap = {"core:sample_start": start, **((captures_extra or [{}] * len(segs))[j])}
        if hb:
            cap["core:header_bytes"] = hb
        captures.append(cap)
        start += len(seg)
    stem = tmp_path / "raster"
    Path(str(stem) + ".sigmf-data").write_bytes(blob)
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps({
        "global": {"core:datatype": datatype, "core:version": "1.0.0", **(extra_global or {})}, "captures": captures,
        "annotations": []}))
    return stem


@pytest.mark.parametrize("oversample", [1, 2])
def test_sigmf_channelized_with_injected_computes(tmp_path, oversample):
    from amcpy_amd import sigmf
    rng = np.random.default_rng(23)
    N, Cn, P = 8, 4, 3
    D, T = Cn // oversample, Cn * P
    lens = [5 * N * D + T + 2, 3 * N * D + T - 1 + 3]
    segs = [_stream("ci8", n, rng) for n in lens]
    stem = _write_recording(tmp_path, segs, [0, 6], {"core:sample_rate": 8.0})
    taps = ddc_ref.make_taps(T)
    ch = {"channels": Cn, "oversample": oversample, "taps": taps, "shift_hz": 1.0}          # an eighth of a turn: half a channel
    seen = []

    def engine(frames):
        seen.append(np.array(frames))
        return np.full((frames.shape[0], 18), float(len(seen)), np.float32) + np.arange(frames.shape[0], dtype=np.float32)[:, None] / 1024
    per_seg = [bank_ref.numpy_bank(seg, taps, Cn, D, shift=0.125, scale=2.0 ** -7) for seg in segs]
    n_frames = [y.shape[1] // N for y in per_seg]
    assert n_frames == [5, 3]
    for chunk in (1 << 24, 13, 1):                                               # however the segment is read
        seen.clear()
        feats, frame_start = sigmf.extract_sigmf(stem, N, channelize=ch, compute=engine, bank_compute=bank_ref.numpy_bank,
                                                 chunk_samples=chunk)
        assert feats.shape == (Cn, sum(n_frames), 18) and feats.dtype == np.float32 and frame_start.dtype == np.int64
        assert frame_start.tolist() == [k * N * D for k in range(n_frames[0])] + [lens[0] + k * N * D for k in range(n_frames[1])]
        assert len(seen) == 2                                                    # one feature call per capture
        for j, (got, y, n) in enumerate(zip(seen, per_seg, n_frames)):           # no frame holds a sample of the other capture
            assert got.dtype == np.complex64 and got.shape == (Cn * n, N)
            assert got.tobytes() == np.ascontiguousarray(y[:, :n * N]).tobytes()
            k0 = sum(n_frames[:j])
            # row c * n + k of the engine's result is channel c, frame k
            want = float(j + 1) + (np.arange(Cn)[:, None] * n + np.arange(n)[None, :]).astype(np.float32) / 1024
            assert np.array_equal(feats[:, k0:k0 + n, 0], want.astype(np.float32))
    kw = dict(channelize=ch, compute=engine, bank_compute=bank_ref.numpy_bank)
    feats, frame_start = sigmf.extract_sigmf(stem, N, max_frames=n_frames[0] + 1, chunk_samples=17, **kw)
    assert frame_start.tolist() == [k * N * D for k in range(n_frames[0])] + [lens[0]] and feats.shape == (Cn, n_frames[0] + 1, 18)
    feats, frame_start = sigmf.extract_sigmf(stem, N, max_frames=2, **kw)
    assert frame_start.tolist() == [0, N * D] and feats.shape == (Cn, 2, 18)
    assert sigmf.extract_sigmf(stem, N, max_frames=0, **kw)[0].shape == (Cn, 0, 18)
    # the default prototype: taps_per_channel
    shift, c2, d2, h = sigmf.resolve_channelize({"global": {}}, {"channels": 8, "oversample": 2, "taps_per_channel": 4})
    assert (shift, c2, d2) == (0, 8, 4) and np.array_equal(h, bank.design_bank_lowpass(8, 4))
    assert np.array_equal(sigmf.resolve_channelize({"global": {}}, {"channels": 8})[3], bank.design_bank_lowpass(8, 16))
    assert sigmf.resolve_channelize({"global": {"core:sample_rate": 8.0}}, {"channels": 4, "shift_hz": -2.0})[0] == Fraction(-1, 4)
    with pytest.raises(ValueError, match="exclude"):
        sigmf.extract_sigmf(stem, N, tune={"decimate": 2}, **kw)
    for bad in ({"oversample": 2}, {"channels": 4, "oversample": 3}, {"channels": 4, "x": 1},
                {"channels": 4, "taps": taps, "taps_per_channel": 3}):
        with pytest.raises(ValueError):
            sigmf.resolve_channelize({"global": {"core:sample_rate": 8.0}}, bad)
    with pytest.raises(ValueError, match="sample_rate"):
        sigmf.resolve_channelize({"global": {}}, {"channels": 4, "shift_hz": 1.0})


def test_recording_command_filter_bank_flags(tmp_path):
    from scipy.io import loadmat
    from amcpy_amd import main as cli
    rng = np.random.default_rng(24)
    N, Cn, P = 8, 4, 2
    segs = [_stream("ci8", 3 * N * Cn + Cn * P + 5, rng), _stream("ci8", 2 * N * Cn + Cn * P + 5, rng)]
    stem = _write_recording(tmp_path, segs, [0, 2], {"core:sample_rate": 8.0}, [{"core:frequency": 90.0}, {"core:frequency": 101.0}])
    parse = cli.build_parser().parse_args
    base = ["recording", str(stem), "--frame-size", str(N)]
    assert cli.recording_channelize(parse(base)) is None
    assert cli.recording_channelize(parse(base + ["--channels", "64"])) == \
        {"channels": 64, "oversample": 1, "taps_per_channel": 16, "shift_hz": 0.0}
    args = parse(base + ["--channels", "8", "--oversample", "2", "--taps-per-channel", "4", "--shift-hz", "-0.5"])
    assert cli.recording_channelize(args) == {"channels": 8, "oversample": 2, "taps_per_channel": 4, "shift_hz": -0.5}
    assert cli.recording_tune(args) is None                                     # the bank's flags are no tuning
    for flags in (["--channels", "8", "--decimate", "2"], ["--channels", "8", "--annotation", "0"], ["--channels", "8", "--taps", "9"],
                  ["--channels", "8", "--oversample", "3"], ["--channels", "8", "--oversample", "1.5"]):
        with pytest.raises(SystemExit):
            cli.recording_channelize(parse(base + flags))
    with pytest.raises(SystemExit):
        cli.recording_tune(parse(base + ["--taps-per-channel", "4"]))

    def engine(frames):
        return np.tile(np.arange(18, dtype=np.float32), (frames.shape[0], 1))
    flags = ["--channels", str(Cn), "--taps-per-channel", str(P), "--shift-hz", "1.0"]
    out = cli.run_recording(parse(base + flags), compute=engine, bank_compute=bank_ref.numpy_bank)
    got = loadmat(out)
    assert {"features", "frame_start", "channel_freq_hz"} <= set(got)
    assert got["features"].shape == (Cn, 5, 18)
    assert got["frame_start"].ravel().tolist() == [k * N * Cn for k in range(3)] + [len(segs[0]) + k * N * Cn for k in range(2)]
    # 8 Hz over 4 channels, moved up by 1 Hz, around the first capture's 90 Hz
    assert got["channel_freq_hz"].ravel().tolist() == [89.0, 91.0, 93.0, 87.0]
    # no sample rate: no channel frequencies (and no shift in Hz)
    (tmp_path / "b").mkdir()
    stem2 = _write_recording(tmp_path / "b", segs, [0, 2])
    got = loadmat(cli.run_recording(parse(["recording", str(stem2), "--frame-size", str(N), "--channels", str(Cn),
                                           "--taps-per-channel", str(P)]), compute=engine, bank_compute=bank_ref.numpy_bank))
    assert "channel_freq_hz" not in got and got["features"].shape == (Cn, 5, 18)
    raw = tmp_path / "raw.cu8"
    raw.write_bytes(bytes(64))
    with pytest.raises(SystemExit):                                              # a raw stream has no raster
        cli.run_recording(parse(["recording", str(raw), "--frame-size", "8", "--format", "cu8", "--channels", "4"]), compute=engine)
