"""8-bit IQ (ci8 / cu8: include/amcx.h, ABI 10) and SigMF recordings on the host: the new symbols, their argument checks,
which kernel a call runs, the staging of 8-bit rows (also under the sanitizers, as a stand-alone program), the Python entry
points' type and shape errors, and the cut of a SigMF recording into frames.  Needs no GPU."""
import ctypes as C
import inspect
import json
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib

REPO = Path(__file__).resolve().parents[1]
TYPED_SIZES = [128, 256, 512, 1024, 2048, 4096]
NEW = ["amcx_features_iq8", "amcx_features_iq8_workspace_bytes", "amcx_kernel_name_iq8", "amcx_ctx_set_iq8_scale",
       "amcx_ctx_features18_iq8_host"]


def _r256(n):
    return (n + 255) // 256 * 256


def test_abi_10_symbols_exist_and_bind():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 10 and lib.amcx_abi_version() >= 10
    assert (_lib.SRC_CI8, _lib.SRC_CU8) == (8, 9) and (_lib.IQ8_CI8, _lib.IQ8_CU8) == (0, 1) and _lib.IQ8_SCALE == 2.0 ** -7
    header = (REPO / "include" / "amcx.h").read_text()
    for line in ("#define AMCX_SRC_CI8 8", "#define AMCX_SRC_CU8 9", "#define AMCX_IQ8_CI8 0", "#define AMCX_IQ8_CU8 1",
                 "#define AMCX_ABI_VERSION 10"):
        assert line in header, line
    assert "127.5" in header and "5, 6 and 7" in header
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_iq8_entry_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    f = lib.amcx_features_iq8
    buf = (C.c_float * 64)()
    dummy = C.addressof(buf)
    dummy += -dummy % 8
    ok = dict(n=4, N=2048, stride=2048, fmt=0, scale=2.0 ** -7, out_stride=18, variant=0, mask=0x5154)
    need = lib.amcx_features_iq8_workspace_bytes(2048, 4, 0)

    def call(iq=dummy, out=dummy, ws=dummy, ws_bytes=need, **kw):
        a = {**ok, **kw}
        return f(iq, a["n"], a["N"], a["stride"], a["fmt"], a["scale"], out, a["out_stride"], None, a["variant"], a["mask"],
                 ws, ws_bytes)

    def both(**kw):
        """the refusal, with frames and as what would otherwise be the n_frames == 0 no-op"""
        return {call(**kw), call(**{"n": 0, **kw})}

    assert call(n=0) == _lib.OK and call(n=0, iq=None, out=None, ws=None, ws_bytes=0) == _lib.OK
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert both(scale=bad) == {_lib.EINVAL}, bad
    for bad in (-1, 2):
        assert both(fmt=bad) == {_lib.EINVAL}, bad
    assert both(iq=dummy + 1) == {_lib.EINVAL}                                       # an odd address
    assert both(stride=2047) == {_lib.EINVAL} and both(out_stride=17) == {_lib.EINVAL} and call(n=-1) == _lib.EINVAL
    for mask in (0, 1 << 18, 0xFFFFFFFF):
        assert both(mask=mask) == {_lib.EINVAL}
    assert both(ws=dummy + 4) == {_lib.EINVAL}                                       # 4-byte aligned
    assert call(ws=None, ws_bytes=0) == _lib.EINVAL                                  # missing
    assert call(ws_bytes=need - 256) == _lib.EINVAL                                  # short
    assert call(iq=None) == _lib.EINVAL and call(out=None) == _lib.EINVAL
    assert both(N=1000, stride=1000, variant=_lib.VARIANT_WAVE) == {_lib.ENOTSUP}
    assert lib.amcx_ctx_set_iq8_scale(None, 1.0) == _lib.EINVAL
    assert lib.amcx_ctx_features18_iq8_host(None, dummy, 1, 2048, 2048, 0, dummy, 18, 0) == _lib.EINVAL
    assert lib.amcx_ctx_features18_iq8_host(None, dummy, 1, 2048, 2048, 2, dummy, 18, 0) == _lib.EINVAL


def test_workspace_bytes():
    lib = _lib.load()
    w = lib.amcx_features_iq8_workspace_bytes
    assert w(2048, 4, _lib.VARIANT_AUTO) == _r256(4 * 2048 * 4)
    assert w(1000, 4, _lib.VARIANT_AUTO) == _r256(8 * 1000 * 4) + lib.amcx_features18_workspace_bytes(1000, 4, 0)
    assert w(2048, 4, _lib.VARIANT_BLOCK) == _r256(8 * 2048 * 4) + lib.amcx_features18_workspace_bytes(2048, 4, 1)
    for N in TYPED_SIZES:
        assert w(N, 1001, _lib.VARIANT_WAVE) == _r256(4 * N * 1001)
    for N, v in ((8192, 0), (16384, 0), (32767, 0), (9000, 1)):
        assert w(N, 7, v) == _r256(8 * N * 7) + lib.amcx_features18_workspace_bytes(N, 7, v)
        assert w(N, 0, v) == 0
    assert w(2048, 0, 0) == 0
    assert w(2048, -1, 0) == -1 and w(1, 4, 0) == -1 and w(1000, 4, _lib.VARIANT_WAVE) == -1


def test_kernel_name_iq8():
    for N in TYPED_SIZES:
        for variant in (_lib.VARIANT_AUTO, _lib.VARIANT_WAVE):
            for mask in (_lib.FEATURES_ALL, _lib.FEATURES_CUMULANTS, _lib.FEATURES_NO_SPECTRAL, 0x5154):
                name = _lib.kernel_name_iq8(N, variant, mask)
                assert name == _lib.kernel_name_sc16(N, variant, mask) and "sc16" in name
        assert _lib.kernel_name_iq8(N, _lib.VARIANT_BLOCK) == _lib.kernel_name(N, _lib.VARIANT_BLOCK)
    for N, variant in ((1000, 0), (8192, 0), (8193, 0), (2048, 1), (32768, 2), (64, 0)):
        for mask in (_lib.FEATURES_ALL, _lib.FEATURES_CUMULANTS, 0x5154):
            name = _lib.kernel_name_iq8(N, variant, mask)
            assert name == _lib.kernel_name_subset(N, variant, mask) and "sc16" not in name
    with pytest.raises(ValueError):
        _lib.kernel_name_iq8(2048, 0, 0)


@pytest.mark.parametrize("kind,dtype", [(8, np.int8), (9, np.uint8)])
def test_stage_host_copies_8_bit_rows_as_they_lie(kind, dtype):
    lib = _lib.load()
    rng = np.random.default_rng(kind)
    S, K, N, L = 2, 5, 48, 61                                       # rows of 61 samples, 48 used
    src = rng.integers(0, 256, (S, K, L, 2)).astype(np.uint8).view(dtype)
    want = np.ascontiguousarray(src[:, :, :N]).reshape(S * K, N, 2)
    for threads in (1, 3):
        dst = np.full((S * K, N, 2), 99, dtype)
        pm = C.c_int32(-1)
        rc = lib.amcx_stage_host(src.ctypes.data, None, kind, S, K, N, K * L, L, 1, 0, S * K, dst.ctypes.data, dst.nbytes,
                                 threads, C.byref(pm), None)
        assert rc == _lib.OK and pm.value == 0
        assert dst.tobytes() == want.tobytes()
    # a run that starts mid-container, crosses the snr seam and ends on a ragged last unit; then a destination one byte short
    dst = np.full((6, N, 2), 99, dtype)
    args = (src.ctypes.data, None, kind, S, K, N, K * L, L, 1, 3, 6, dst.ctypes.data)
    assert lib.amcx_stage_host(*args, dst.nbytes, 2, None, None) == _lib.OK
    assert dst.tobytes() == want[3:9].tobytes()
    assert lib.amcx_stage_host(*args, dst.nbytes - 1, 1, None, None) == _lib.EINVAL
    dst1 = np.full((1, N, 2), 99, dtype)
    assert lib.amcx_stage_host(src.ctypes.data, None, kind, S, K, N, K * L, L, 1, S * K - 1, 1, dst1.ctypes.data, dst1.nbytes,
                               4, None, None) == _lib.OK
    assert dst1.tobytes() == want[-1:].tobytes()
    assert lib.amcx_stage_host(src.ctypes.data, None, kind, S, K, N, K * L, L, 1, S * K - 1, 2, dst.ctypes.data, dst.nbytes,
                               1, None, None) == _lib.EINVAL
    # planes are refused: [sample][snr][frame] and [sample][frame][snr]
    for strides in ((K, 1, S * K), (1, S, S * K)):
        assert lib.amcx_stage_host(src.ctypes.data, None, kind, S, K, N, *strides, 0, N, dst.ctypes.data, 1 << 30, 1, None,
                                   None) == _lib.ENOTSUP
    for no_kind in (5, 6, 7, 10, -1):
        assert lib.amcx_stage_host(src.ctypes.data, None, no_kind, S, K, N, K * L, L, 1, 0, 1, dst.ctypes.data, dst.nbytes, 1,
                                   None, None) == _lib.EINVAL


@pytest.mark.parametrize("kind,dtype", [(8, np.int8), (9, np.uint8)])
def test_stage_file_reads_8_bit_rows_at_an_odd_sample_offset(tmp_path, kind, dtype):
    lib = _lib.load()
    rng = np.random.default_rng(10 + kind)
    K, N, skip = 9, 40, 7
    src = rng.integers(0, 256, (K, N, 2)).astype(np.uint8).view(dtype)
    path = tmp_path / "rows.iq8"
    path.write_bytes(b"\x01" * (2 * skip) + src.tobytes())
    dst = np.zeros((K, N, 2), dtype)
    with open(path, "rb") as fh:
        rc = lib.amcx_stage_file(fh.fileno(), 2 * skip, -1, kind, 1, K, N, 0, N, 1, 0, K, dst.ctypes.data, dst.nbytes, 2, None,
                                 None)
        assert rc == _lib.OK and dst.tobytes() == src.tobytes()
        assert lib.amcx_stage_file(fh.fileno(), 2 * skip + 1, -1, kind, 1, K, N, 0, N, 1, 0, K - 1, dst.ctypes.data, dst.nbytes,
                                   2, None, None) == _lib.OK                         # an odd BYTE offset is a file's business
        assert dst.tobytes()[:2 * N * (K - 1)] == src.tobytes()[1:1 + 2 * N * (K - 1)]
        # the file ends inside the last row
        assert lib.amcx_stage_file(fh.fileno(), 2 * skip + 2, -1, kind, 1, K, N, 0, N, 1, 0, K, dst.ctypes.data, dst.nbytes, 1,
                                   None, None) == _lib.EIO
        with pytest.raises(OSError):
            _lib.check(_lib.EIO)


def test_python_errors_arrive_before_the_library_is_touched(monkeypatch):
    import torch
    from amcpy_amd import features
    from amcpy_amd.feature_extraction import HipEngine

    def no_load(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "require_torch_runtime", no_load)
    for dt in (torch.int8, torch.uint8):
        good = torch.zeros((3, 64, 2), dtype=dt)
        with pytest.raises(TypeError):
            features.features18_iq8(good.to(torch.int16))                        # int16 input
        with pytest.raises(TypeError):
            features.features18_iq8(good.numpy())                                # not a tensor
        with pytest.raises(TypeError):
            features.features18_iq8(torch.zeros((3, 64, 3), dtype=dt))           # last dimension is not (I, Q)
        with pytest.raises(TypeError):
            features.features18_iq8(torch.zeros((64,), dtype=dt))
        with pytest.raises(ValueError):
            features.features18_iq8(torch.zeros((3, 2, 64), dtype=dt).transpose(1, 2))     # planes of I and of Q
        with pytest.raises(ValueError):
            features.features18_iq8(torch.zeros((3, 64, 4), dtype=dt)[:, :, ::2])          # pairs 4 bytes apart
        with pytest.raises(ValueError):
            features.features18_iq8(good)                                        # host tensor
        with pytest.raises(ValueError):
            features.features18_iq8(good, frame_size=65)
        with pytest.raises(ValueError):
            features.features18_iq8(good, chunk_frames=0)
        for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-50):               # 1e-50 is 0 as a float32
            with pytest.raises(ValueError):
                features.features18_iq8(good, scale=bad)
            with pytest.raises(ValueError):
                features.features18_iq8_host(good.numpy(), scale=bad)
            with pytest.raises(ValueError):
                HipEngine(64, device=0, iq8_scale=bad)
        with pytest.raises(KeyError):
            features.features18_iq8(good, feature_ids=[19])
        with pytest.raises(KeyError):
            features.features18_iq8_host(good.numpy(), feature_ids=[19])
    for dt, sample in ((np.int8, features.CI8), (np.uint8, features.CU8)):
        x = np.zeros((3, 64, 2), dt)
        with pytest.raises(TypeError):
            features.features18_iq8_host(x.astype(np.int16))
        with pytest.raises(TypeError):
            features.features18_iq8_host(np.zeros((3, 64, 3), dt))
        with pytest.raises(ValueError):
            features.features18_iq8_host(x, frame_size=65)
        with pytest.raises(TypeError):
            features.iq8_view(x.astype(np.int16))
        with pytest.raises(TypeError):
            features.iq8_view(np.zeros((3, 64, 3), dt))
        with pytest.raises(ValueError):
            features.iq8_view(np.zeros((3, 2, 64), dt).transpose(0, 2, 1))       # planes of I and of Q
        with pytest.raises(ValueError):
            features.iq8_view(np.zeros((3, 64, 4), dt)[:, :, ::2])               # pairs 4 bytes apart
        with pytest.raises(ValueError):
            HipEngine(64, device=0)(np.zeros((3, 64, 4), dt)[:, :, ::2])
        with pytest.raises(ValueError):
            HipEngine(65, device=0)(x)                                           # frame_size > L
        v = features.iq8_view(x)
        assert v.shape == (3, 64) and v.dtype == sample and v.dtype.itemsize == 2
        assert np.shares_memory(v, x)


@pytest.mark.parametrize("fmt", ["ci8", "cu8"])
def test_extract_raw_stream_8_bit_with_an_injected_engine(tmp_path, fmt):
    """The file is cut as documented (leading samples skipped, a trailing partial frame dropped) and an injected engine
    sees the widened complex64 frames."""
    from amcpy_amd.feature_extraction import extract_raw_stream
    params = inspect.signature(extract_raw_stream).parameters
    assert params["scale"].default == 2.0 ** -15 and params["scale8"].default == 2.0 ** -7
    rng = np.random.default_rng(11)
    N, K = 32, 6
    x = rng.integers(0, 256, (K, N, 2)).astype(np.uint8)
    x[0, :, 0] = np.arange(0, 256, 8)
    x[1].reshape(-1)[:] = np.arange(192, 256)                        # both halves of the byte range
    path = tmp_path / "s.iq8"
    path.write_bytes(np.zeros((5, 2), np.uint8).tobytes() + x.tobytes() + np.ones((N - 1, 2), np.uint8).tobytes())
    seen = []

    def engine(frames):
        seen.append(np.array(frames))
        return np.zeros((frames.shape[0], 18), np.float32)
    scale8 = float(np.float32(1.0 / 100.0))
    out = extract_raw_stream(path, N, skip_samples=5, sample_format=fmt, scale8=scale8, compute=engine)
    assert out.shape == (K, 18)
    ints = x.view(np.int8).astype(np.float32) if fmt == "ci8" else (x.astype(np.int16) - 128).astype(np.float32)
    wide = (ints * np.float32(scale8)).view(np.complex64)[..., 0]
    assert seen[0].dtype == np.complex64 and seen[0].tobytes() == wide.tobytes()
    assert extract_raw_stream(path, N, skip_samples=5, sample_format=fmt, max_frames=2, compute=engine).shape == (2, 18)
    # `scale8` belongs to the 8-bit formats, `scale` to sc16: neither is held to the other's
    assert extract_raw_stream(path, N, sample_format=fmt, scale=0.0, compute=engine).shape[1] == 18
    assert extract_raw_stream(path, N, sample_format="sc16", scale8=0.0, compute=engine).shape[1] == 18
    with pytest.raises(ValueError):
        extract_raw_stream(path, N, sample_format=fmt, scale8=0.0, compute=engine)


# ---- SigMF -----------------------------------------------------------------------------------------------------------
SIGMF = {"cf32_le": np.dtype("<c8"), "ci16_le": np.dtype("<i2"), "ci8": np.dtype("i1"), "cu8": np.dtype("u1")}


def _write_recording(tmp_path, datatype, seg_lens, header_bytes, rng, name="rec"):
    """A recording of len(seg_lens) captures; capture j is preceded by header_bytes[j] bytes.  -> (stem, [segments as stored])"""
    store = SIGMF[datatype]
    segs, blob, captures, start = [], b"", [], 0
    for n, hb in zip(seg_lens, header_bytes):
        if datatype == "cf32_le":
            seg = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        else:
            info = np.iinfo(store)
            seg = rng.integers(info.min, info.max + 1, (n, 2)).astype(store)
        segs.append(seg)
        blob += b"\xee" * hb + seg.tobytes()
        cap = {"core:sample_start": start}
        if hb:
            cap["core:header_bytes"] = hb
        captures.append(cap)
        start += n
    stem = tmp_path / name
    Path(str(stem) + ".sigmf-data").write_bytes(blob)
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps(
        {"global": {"core:datatype": datatype, "core:version": "1.0.0"}, "captures": captures, "annotations": []}))
    return stem, segs


def _widened(seg, datatype, scale):
    if datatype == "cf32_le":
        return seg
    ints = seg.astype(np.int16) - (128 if datatype == "cu8" else 0)
    return (ints.astype(np.float32) * np.float32(scale)).view(np.complex64)[..., 0]


@pytest.mark.parametrize("datatype", list(SIGMF))
def test_sigmf_recordings_are_cut_per_capture(tmp_path, datatype):
    from amcpy_amd import sigmf
    rng = np.random.default_rng(12)
    N = 16
    lens = [3 * N + 5, 4 * N + 2]                                   # the first segment is no multiple of N
    stem, segs = _write_recording(tmp_path, datatype, lens, [0, 6], rng)
    seen = []

    def engine(frames):
        seen.append(np.array(frames))
        return np.full((frames.shape[0], 18), float(len(seen)), np.float32)
    scale = {"cf32_le": 1.0, "ci16_le": 2.0 ** -15, "ci8": 2.0 ** -7, "cu8": 2.0 ** -7}[datatype]
    meta = sigmf.read_meta(stem)
    assert meta["datatype"] == datatype and meta["scale"] == scale
    assert meta["segments"] == [(0, 0, lens[0]), (lens[0], 6 + lens[0] * meta["store"].itemsize, lens[1])]
    for name in (stem, str(stem) + ".sigmf-meta", str(stem) + ".sigmf-data"):
        seen.clear()
        feats, frame_start = sigmf.extract_sigmf(name, N, compute=engine)
        assert feats.shape == (7, 18) and feats.dtype == np.float32
        assert frame_start.dtype == np.int64
        assert frame_start.tolist() == [0, N, 2 * N] + [lens[0] + k * N for k in range(4)]
        assert feats[:, 0].tolist() == [1.0] * 3 + [2.0] * 4                 # one engine call per segment
        by_hand = [_widened(segs[0], datatype, scale)[:3 * N].reshape(3, N),
                   _widened(segs[1], datatype, scale)[:4 * N].reshape(4, N)]
        assert len(seen) == 2
        for got, want in zip(seen, by_hand):
            assert got.dtype == np.complex64 and got.tobytes() == want.tobytes()
    feats, frame_start = sigmf.extract_sigmf(stem, N, max_frames=4, compute=engine)
    assert frame_start.tolist() == [0, N, 2 * N, lens[0]]
    if datatype != "cf32_le":
        seen.clear()
        sigmf.extract_sigmf(stem, N, scale=0.25, compute=engine)
        assert seen[0].tobytes() == _widened(segs[0], datatype, 0.25)[:3 * N].tobytes()
        with pytest.raises(ValueError):
            sigmf.extract_sigmf(stem, N, scale=0.0, compute=engine)


@pytest.mark.parametrize("datatype", ["rf32_le", "ri16_le", "ru8", "cf32_be", "ci16_be", "cf64_le", "ci32_le", "cu16_le",
                                      "ci16"])
def test_sigmf_refuses_other_datatypes_by_name(tmp_path, datatype):
    from amcpy_amd import sigmf
    stem = tmp_path / "other"
    Path(str(stem) + ".sigmf-data").write_bytes(b"\0" * 64)
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps({"global": {"core:datatype": datatype}, "captures": []}))
    with pytest.raises(ValueError, match=datatype):
        sigmf.read_meta(stem)
    with pytest.raises(ValueError, match=datatype):
        sigmf.extract_sigmf(stem, 8, compute=lambda fr: np.zeros((len(fr), 18), np.float32))


def test_sigmf_meta_without_a_datatype_and_without_captures(tmp_path):
    from amcpy_amd import sigmf
    stem = tmp_path / "bare"
    Path(str(stem) + ".sigmf-data").write_bytes(np.arange(40, dtype=np.uint8).tobytes())
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps({"global": {"core:version": "1.0.0"}, "captures": []}))
    with pytest.raises(ValueError, match="core:datatype"):
        sigmf.read_meta(stem)
    # no captures: the whole file is one segment; trailing bytes are no samples
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps({"global": {"core:datatype": "cu8", "core:trailing_bytes": 4}}))
    assert sigmf.read_meta(stem)["segments"] == [(0, 0, 18)]
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps({"global": {"core:datatype": "cu8", "core:num_channels": 2}}))
    with pytest.raises(ValueError, match="num_channels"):
        sigmf.read_meta(stem)


def test_recording_command_writes_features_and_frame_start(tmp_path):
    from scipy.io import loadmat
    from amcpy_amd import main as cli
    rng = np.random.default_rng(13)
    N = 16
    stem, _ = _write_recording(tmp_path, "ci8", [2 * N + 3, N], [0, 2], rng)

    def engine(frames):
        return np.tile(np.arange(18, dtype=np.float32), (frames.shape[0], 1))
    args = cli.build_parser().parse_args(["recording", str(stem) + ".sigmf-meta", "--frame-size", str(N), "--features", "3,5"])
    out = cli.run_recording(args, compute=engine)
    assert out == tmp_path / "rec_features.mat" and not list(tmp_path.glob("*.tmp"))
    got = loadmat(out)
    assert got["frame_start"].ravel().tolist() == [0, N, 2 * N + 3]
    assert got["features"].shape == (3, 18) and got["features"][0, 2] == 2.0 and np.isnan(got["features"][0, 0])
    raw = tmp_path / "raw.cu8"
    raw.write_bytes(rng.integers(0, 256, (3 * N + 1, 2)).astype(np.uint8).tobytes())
    with pytest.raises(SystemExit):
        cli.run_recording(cli.build_parser().parse_args(["recording", str(raw), "--frame-size", str(N)]), compute=engine)
    with pytest.raises(SystemExit):
        cli.run_recording(cli.build_parser().parse_args(["recording", str(stem), "--frame-size", str(N), "--format", "ci8"]),
                          compute=engine)
    args = cli.build_parser().parse_args(["recording", str(raw), "--frame-size", str(N), "--format", "cu8", "--scale", "0.5",
                                          "--out", str(tmp_path / "o.mat")])
    got = loadmat(cli.run_recording(args, compute=engine))
    assert got["frame_start"].ravel().tolist() == [0, N, 2 * N] and got["features"].shape == (3, 18)


# ---- the staging threads under the sanitizers ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,flags", [
    ("asan_ubsan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
    ("tsan", ["-O1", "-g", "-fsanitize=thread"]),
    ("plain", ["-O2"])])
def test_8_bit_staging_under_the_sanitizers(tmp_path, name, flags):
    """amcx_upload.h's 8-bit row path as a stand-alone program (tests/host_san/stage_iq8.cc, its own main; nothing is
    preloaded, nothing is loaded into python): random padded containers, runs that start mid-container and end ragged,
    1 ... 8 threads, memory and a file at an odd byte offset, compared with a byte copy; a short file says EIO."""
    exe = tmp_path / f"stage_iq8_{name}"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *flags,
           str(REPO / "tests" / "host_san" / "stage_iq8.cc"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    for seed in ("2026", "7"):
        r = subprocess.run([str(exe), seed], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "STAGE_IQ8_OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-6000:])
        assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr \
            and "runtime error" not in r.stderr, r.stderr[-6000:]
