"""16-bit integer IQ (sc16: include/amcx.h, ABI 9) on the host: the new symbols, their argument checks, which kernel a call
runs, the staging of sc16 rows, the occupancy of the sc16 kernels read from the built library, and the Python entry points'
type and shape errors.  Needs no GPU."""
import ctypes as C
import importlib.util
import inspect
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib

REPO = Path(__file__).resolve().parents[1]
TYPED_SIZES = [128, 256, 512, 1024, 2048, 4096]
NEW = ["amcx_features_sc16", "amcx_features_sc16_workspace_bytes", "amcx_kernel_name_sc16", "amcx_ctx_set_sc16_scale",
       "amcx_ctx_features18_sc16_host"]


def test_abi_9_symbols_exist_and_bind():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 9 and lib.amcx_abi_version() >= 9
    assert _lib.SRC_SC16 == 4 and _lib.SC16_SCALE == 2.0 ** -15
    header = (REPO / "include" / "amcx.h").read_text()
    assert "#define AMCX_SRC_SC16 4" in header
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1]
    from amcpy_amd import features, feature_extraction
    assert "scale" in inspect.signature(features.features18_sc16).parameters
    assert "scale" in inspect.signature(features.features18_sc16_host).parameters
    params = inspect.signature(feature_extraction.extract_raw_stream).parameters
    assert params["sample_format"].default == "cf32" and params["scale"].default == 2.0 ** -15


def test_sc16_entry_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    f = lib.amcx_features_sc16
    buf = (C.c_float * 64)()
    dummy = C.addressof(buf)
    assert dummy % 4 == 0
    ok = dict(n=4, N=2048, stride=2048, scale=2.0 ** -15, out_stride=18, variant=0, mask=0x5154)

    def call(iq=dummy, out=dummy, ws=None, ws_bytes=0, **kw):
        a = {**ok, **kw}
        return f(iq, a["n"], a["N"], a["stride"], a["scale"], out, a["out_stride"], None, a["variant"], a["mask"], ws, ws_bytes)

    for bad in (0.0, -1.0, -0.0, float("inf"), float("-inf"), float("nan")):
        assert call(scale=bad) == _lib.EINVAL, bad
        assert call(scale=bad, n=0, iq=None, out=None) == _lib.EINVAL, bad          # ... checked before the no-op
    for mask in (0, 1 << 18, 0xFFFFFFFF):
        assert call(mask=mask) == _lib.EINVAL
    assert call(iq=None) == _lib.EINVAL and call(out=None) == _lib.EINVAL
    assert call(stride=2047) == _lib.EINVAL and call(out_stride=17) == _lib.EINVAL and call(n=-1) == _lib.EINVAL
    assert call(N=1) == _lib.EINVAL and call(variant=3) == _lib.EINVAL
    assert call(N=1000, stride=1000, variant=_lib.VARIANT_WAVE) == _lib.ENOTSUP
    assert call(iq=dummy + 2) == _lib.EINVAL                                        # not 4-byte aligned
    assert call(n=0, iq=None, out=None) == _lib.OK
    # a size without an sc16 kernel needs the widened copy's room: none, or too little, is refused
    need = lib.amcx_features_sc16_workspace_bytes(1000, 4, 0)
    assert need == (8 * 1000 * 4 + 255) // 256 * 256
    assert call(N=1000, stride=1000) == _lib.EINVAL
    assert call(N=1000, stride=1000, ws=dummy, ws_bytes=need - 256) == _lib.EINVAL
    assert call(N=2048, stride=2048, variant=_lib.VARIANT_BLOCK) == _lib.EINVAL
    assert lib.amcx_ctx_set_sc16_scale(None, 1.0) == _lib.EINVAL
    assert lib.amcx_ctx_features18_sc16_host(None, dummy, 1, 2048, 2048, dummy, 18, 0) == _lib.EINVAL


def test_workspace_bytes():
    lib = _lib.load()
    w = lib.amcx_features_sc16_workspace_bytes
    for N in TYPED_SIZES:
        assert w(N, 1000, _lib.VARIANT_AUTO) == 0 and w(N, 1000, _lib.VARIANT_WAVE) == 0
        assert w(N, 1000, _lib.VARIANT_BLOCK) == (8 * N * 1000 + 255) // 256 * 256
    for N, v in ((1000, 0), (8192, 0), (16384, 0), (32767, 0), (32768, 2), (9000, 1)):
        head = (8 * N * 7 + 255) // 256 * 256
        assert w(N, 7, v) == head + lib.amcx_features18_workspace_bytes(N, 7, v)
        assert w(N, 0, v) == 0
    assert w(2048, -1, 0) == -1 and w(1, 4, 0) == -1 and w(1000, 4, _lib.VARIANT_WAVE) == -1


@pytest.mark.parametrize("N", TYPED_SIZES)
def test_kernel_name_sc16_names_an_sc16_kernel(N):
    fam = "short" if N <= 512 else "wave"
    for variant in (_lib.VARIANT_AUTO, _lib.VARIANT_WAVE):
        assert _lib.kernel_name_sc16(N, variant) == f"amcx_features18_{fam}_sc16_kernel<{N}>"
        assert _lib.kernel_name_sc16(N, variant, 1 | (1 << 12)) == f"amcx_features18_{fam}_sc16_kernel<{N}>"
        for mask in (_lib.FEATURES_NO_SPECTRAL, 0x5154, 1 << 3):
            assert _lib.kernel_name_sc16(N, variant, mask) == f"amcx_features_subset_{fam}_sc16_kernel<{N}, 1>"
        for mask in (_lib.FEATURES_CUMULANTS, 1 << 12):
            assert _lib.kernel_name_sc16(N, variant, mask) == f"amcx_features_subset_{fam}_sc16_kernel<{N}, 2>"
    # the block variant widens and runs the complex64 kernel
    assert _lib.kernel_name_sc16(N, _lib.VARIANT_BLOCK, 0x5154) == _lib.kernel_name(N, _lib.VARIANT_BLOCK)


@pytest.mark.parametrize("N,variant", [(1000, 0), (8192, 0), (8192, 2), (16384, 0), (32767, 0), (32768, 2), (64, 0)])
def test_kernel_name_sc16_elsewhere_is_the_complex64_kernel(N, variant):
    for mask in (_lib.FEATURES_ALL, _lib.FEATURES_CUMULANTS, 0x5154):
        name = _lib.kernel_name_sc16(N, variant, mask)
        assert name == _lib.kernel_name_subset(N, variant, mask) and "sc16" not in name
    with pytest.raises(ValueError):
        _lib.kernel_name_sc16(N, variant, 0)


def test_stage_host_copies_sc16_rows_as_they_lie():
    lib = _lib.load()
    rng = np.random.default_rng(9)
    S, K, N, L = 2, 5, 48, 61                                       # rows of 61 samples, 48 used
    src = rng.integers(-32768, 32768, (S, K, L, 2)).astype(np.int16)
    want = np.ascontiguousarray(src[:, :, :N]).reshape(S * K, N, 2)
    for threads in (1, 3):
        dst = np.full((S * K, N, 2), 999, np.int16)
        pm, inner = C.c_int32(-1), C.c_int32(-1)
        rc = lib.amcx_stage_host(src.ctypes.data, None, _lib.SRC_SC16, S, K, N, K * L, L, 1, 0, S * K, dst.ctypes.data,
                                 dst.nbytes, threads, C.byref(pm), C.byref(inner))
        assert rc == _lib.OK and pm.value == 0
        assert dst.tobytes() == want.tobytes()
    # a part of the frames, and a destination one byte short
    dst = np.full((4, N, 2), 999, np.int16)
    assert lib.amcx_stage_host(src.ctypes.data, None, _lib.SRC_SC16, S, K, N, K * L, L, 1, 3, 4, dst.ctypes.data, dst.nbytes,
                               1, None, None) == _lib.OK
    assert dst.tobytes() == want[3:7].tobytes()
    assert lib.amcx_stage_host(src.ctypes.data, None, _lib.SRC_SC16, S, K, N, K * L, L, 1, 3, 4, dst.ctypes.data,
                               dst.nbytes - 1, 1, None, None) == _lib.EINVAL
    # planes are refused: [sample][snr][frame] and [sample][frame][snr]
    for strides in ((K, 1, S * K), (1, S, S * K)):
        assert lib.amcx_stage_host(src.ctypes.data, None, _lib.SRC_SC16, S, K, N, *strides, 0, N, dst.ctypes.data,
                                   1 << 30, 1, None, None) == _lib.ENOTSUP
    assert lib.amcx_stage_host(src.ctypes.data, None, 5, S, K, N, K * L, L, 1, 0, 1, dst.ctypes.data, dst.nbytes, 1, None,
                               None) == _lib.EINVAL


def test_stage_file_reads_sc16_rows(tmp_path):
    lib = _lib.load()
    rng = np.random.default_rng(10)
    K, N = 9, 40
    src = rng.integers(-32768, 32768, (K, N, 2)).astype(np.int16)
    path = tmp_path / "rows.sc16"
    path.write_bytes(b"\x01" * 12 + src.tobytes())
    dst = np.zeros((K, N, 2), np.int16)
    with open(path, "rb") as fh:
        rc = lib.amcx_stage_file(fh.fileno(), 12, -1, _lib.SRC_SC16, 1, K, N, 0, N, 1, 0, K, dst.ctypes.data, dst.nbytes, 2,
                                 None, None)
        assert rc == _lib.OK and dst.tobytes() == src.tobytes()
        # the file ends inside the last row
        with pytest.raises(OSError):
            _lib.check(lib.amcx_stage_file(fh.fileno(), 16, -1, _lib.SRC_SC16, 1, K, N, 0, N, 1, 0, K, dst.ctypes.data,
                                           dst.nbytes, 1, None, None))


def _float_twin(name):
    return name.replace("_sc16", "")


def test_sc16_kernels_keep_their_float_kernels_occupancy():
    """From the BUILT library (tools/resource_usage.py): every sc16 kernel runs as many waves per SIMD as the complex64
    kernel of the same size and plan.  Waves per SIMD of these kernels: one workgroup per CU (their LDS), so the
    workgroup's waves / 4, unless the registers allow fewer -- 512 VGPRs per SIMD lane in steps of 8: 128 -> 4, 168 -> 3,
    256 -> 2 (the steps tests/test_host_cpu.py::test_kernel_resources_match_the_committed_table names).  The spills are
    held to amcpy_amd/csrc/kernel_resources.json by that test."""
    spec = importlib.util.spec_from_file_location("resource_usage", REPO / "tools" / "resource_usage.py")
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    rows = ru.read()

    def waves(r):
        by_regs = 512 // ((r["vgpr"] + 7) // 8 * 8)
        return min(by_regs, r["max_threads"] // 64 // 4, 8)

    typed = sorted(k for k in rows if "sc16" in k and "features" in k)
    assert len(typed) == 21, typed
    for size in TYPED_SIZES:
        assert sum(f"<{size}>" in k or f"<{size}," in k for k in typed) == (5 if size == 2048 else 3) + (1 if size == 2048 else 0), size
    for k in typed:
        twin = _float_twin(k)
        assert twin in rows, twin
        assert rows[k]["max_threads"] == rows[twin]["max_threads"], k
        assert waves(rows[k]) == waves(rows[twin]), (k, rows[k], rows[twin])
    assert "amcx_sc16_to_c64_kernel" in rows and rows["amcx_sc16_to_c64_kernel"]["spill"] == 0


def test_python_errors_arrive_before_the_library_is_touched(monkeypatch):
    import torch
    from amcpy_amd import features
    from amcpy_amd.feature_extraction import HipEngine, extract_raw_stream

    def no_load(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "require_torch_runtime", no_load)
    good = torch.zeros((3, 64, 2), dtype=torch.int16)
    with pytest.raises(TypeError):
        features.features18_sc16(good.to(torch.int32))                       # wrong dtype
    with pytest.raises(TypeError):
        features.features18_sc16(good.numpy())                               # not a tensor
    with pytest.raises(TypeError):
        features.features18_sc16(torch.zeros((3, 64, 3), dtype=torch.int16))  # last dimension is not (I, Q)
    with pytest.raises(TypeError):
        features.features18_sc16(torch.zeros((64,), dtype=torch.int16))
    with pytest.raises(ValueError):
        features.features18_sc16(torch.zeros((3, 2, 64), dtype=torch.int16).transpose(1, 2))   # planes of I and of Q
    with pytest.raises(ValueError):
        features.features18_sc16(torch.zeros((3, 64, 4), dtype=torch.int16)[:, :, ::2])         # pairs 8 bytes apart
    with pytest.raises(ValueError):
        features.features18_sc16(good)                                       # host memory
    with pytest.raises(ValueError):
        features.features18_sc16(good, frame_size=65)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-50):               # 1e-50 is 0 as a float32
        with pytest.raises(ValueError):
            features.features18_sc16(good, scale=bad)
        with pytest.raises(ValueError):
            features.features18_sc16_host(good.numpy(), scale=bad)
        with pytest.raises(ValueError):
            HipEngine(64, device=0, sc16_scale=bad)
    with pytest.raises(KeyError):
        features.features18_sc16(good, feature_ids=[19])
    x = np.zeros((3, 64, 2), np.int16)
    with pytest.raises(TypeError):
        features.features18_sc16_host(x.astype(np.int32))
    with pytest.raises(TypeError):
        features.features18_sc16_host(np.zeros((3, 64, 3), np.int16))
    with pytest.raises(ValueError):
        features.features18_sc16_host(x, frame_size=65)
    with pytest.raises(ValueError):
        features.sc16_view(np.zeros((3, 2, 64), np.int16).transpose(0, 2, 1))
    with pytest.raises(ValueError):
        HipEngine(64, device=0)(np.zeros((3, 64, 4), np.int16)[:, :, ::2])
    with pytest.raises(ValueError):
        extract_raw_stream("nowhere.bin", 64, sample_format="sc8")
    v = features.sc16_view(x)
    assert v.shape == (3, 64) and v.dtype == features.SC16 and v.dtype.itemsize == 4


def test_extract_raw_stream_sc16_with_an_injected_engine(tmp_path):
    """The file is cut as documented (leading samples skipped, a trailing partial frame dropped) and an injected engine
    sees the widened complex64 frames."""
    from amcpy_amd.feature_extraction import extract_raw_stream
    rng = np.random.default_rng(11)
    N, K = 32, 6
    x = rng.integers(-32768, 32768, (K, N, 2)).astype(np.int16)
    path = tmp_path / "s.sc16"
    path.write_bytes(np.zeros((5, 2), np.int16).tobytes() + x.tobytes() + np.ones((N - 1, 2), np.int16).tobytes())
    seen = []

    def engine(frames):
        seen.append(np.array(frames))
        return np.zeros((frames.shape[0], 18), np.float32)
    scale = float(np.float32(1.0 / 30000.0))
    out = extract_raw_stream(path, N, skip_samples=5, sample_format="sc16", scale=scale, compute=engine)
    assert out.shape == (K, 18)
    wide = (x.astype(np.float32) * np.float32(scale)).view(np.complex64)[..., 0]
    assert seen[0].dtype == np.complex64 and np.array_equal(seen[0], wide)
    assert extract_raw_stream(path, N, skip_samples=5, sample_format="sc16", max_frames=2, compute=engine).shape == (2, 18)
    # `scale` belongs to sc16: a cf32 caller is not held to it, an sc16 caller is
    assert extract_raw_stream(path, N, sample_format="cf32", scale=0.0, compute=engine).shape[1] == 18
    with pytest.raises(ValueError):
        extract_raw_stream(path, N, sample_format="sc16", scale=0.0, compute=engine)
