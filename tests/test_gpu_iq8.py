"""8-bit IQ (ci8 / cu8: include/amcx.h, ABI 10) on the GPU.

THE ORACLE IS EXACT.  A component is (int8)(byte ^ flip) -- the byte itself for ci8, byte - 128 for cu8 -- and widening it to
int16 is sign extension, so an 8-bit call must equal amcx_features_sc16 on ``int16(x)`` and amcx_features_c64_subset on
``float32(int16(x)) * float32(scale)``, both built here with numpy, same variant and feature mask, bit for bit
(``array_equal`` with ``equal_nan``).  The widening kernels themselves are read back: the head of the workspace is
numpy's widening, nothing behind the workspace is touched.

Every frame holds every byte value 0 ... 255 as I and as Q where a frame has the 256 samples that takes; shorter frames
(N = 128, 130, 136) hold them over each two consecutive frames.  The rest is seeded random."""
import functools
import json
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib

pytestmark = pytest.mark.gpu

FORMATS = {"ci8": (np.int8, _lib.IQ8_CI8), "cu8": (np.uint8, _lib.IQ8_CU8)}
TYPED_SIZES = [128, 256, 512, 1024, 2048, 4096]
SCALE = 2.0 ** -7
GUARD = 256


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _ids(mask):
    return None if mask == _lib.FEATURES_ALL else [j + 1 for j in range(18) if (mask >> j) & 1]


def _r256(n):
    return (n + 255) // 256 * 256


@functools.lru_cache(maxsize=None)
def _bytes(F, N, seed=0):
    """(F, N, 2) uint8, read-only: the raw bytes of F frames, whichever format reads them"""
    rng = np.random.default_rng(77 * N + F + seed)
    x = rng.integers(0, 256, (F, N, 2)).astype(np.uint8)
    m = min(N, 256)
    for f in range(F):
        vals = (np.arange(m) + (128 * f if N < 256 else 0)) % 256
        x[f, rng.permutation(N)[:m], 0] = vals
        x[f, rng.permutation(N)[:m], 1] = 255 - vals
    if N >= 256:
        assert all(len(set(x[f, :, c].tolist())) == 256 for f in range(F) for c in (0, 1))
    elif F > 1:
        assert all(len(set(x[f:f + 2, :, c].ravel().tolist())) == 256 for f in range(F - 1) for c in (0, 1))
    x.setflags(write=False)
    return x


def _ints(raw, fmt):
    """THE REFERENCE: the int16 an 8-bit sample stands for"""
    return raw.view(np.int8).astype(np.int16) if fmt == "ci8" else raw.astype(np.int16) - 128


def _widen(raw, fmt, scale=SCALE):
    w = _ints(raw, fmt).astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(w).view(np.complex64)[..., 0]


def _typed(raw, fmt):
    """the array a caller holds: int8 for ci8, uint8 for cu8"""
    return np.ascontiguousarray(raw).view(FORMATS[fmt][0])


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _where(a, b):
    return np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b)))).tolist()[:8]


def _raw_call(buf, byte_off, F, N, stride, fmt, variant=_lib.VARIANT_AUTO, mask=_lib.FEATURES_ALL, scale=SCALE):
    """amcx_features_iq8 over bytes of the uint8 device tensor `buf` with a polluted caller workspace, GUARD bytes longer
    than asked -> (features (F, 18), the workspace read back ONCE: head, rest and guard)"""
    torch = _torch()
    lib = _lib.load()
    need = lib.amcx_features_iq8_workspace_bytes(N, F, variant)
    assert need > 0
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((F, 18), -5.0, dtype=torch.float32, device="cuda")
    assert ws.data_ptr() % 16 == 0
    _lib.check(lib.amcx_features_iq8(buf.data_ptr() + byte_off, F, N, stride, FORMATS[fmt][1], scale, out.data_ptr(), 18,
                                     torch.cuda.current_stream().cuda_stream, variant, mask, ws.data_ptr(), need))
    torch.cuda.synchronize()
    return out.cpu().numpy(), ws.cpu().numpy()


@pytest.mark.parametrize("N", [128, 130, 136, 1000])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_widening_meets_every_seam(fmt, N):
    """Rows N, N + 1, N + 7, N + 8 samples apart, starting 0, 1, 3, 8 samples into the buffer, 1, 3 and 65 of them: rows that
    start on 16 bytes take the vector path, the others the general one -- with an odd stride both within one launch -- and
    N = 130, 136, 1000 end on it or not.  The padding between rows holds a second pattern."""
    torch = _torch()
    typed = N in TYPED_SIZES
    for F in (1, 3, 65):
        raw = _bytes(F, N)
        wide16 = _ints(raw, fmt)
        packed = torch.from_numpy(np.array(raw)).cuda().reshape(-1)
        ref, ws = _raw_call(packed, 0, F, N, N, fmt)
        for stride in (N, N + 1, N + 7, N + 8):
            for off in (0, 1, 3, 8):
                host = np.full((off + F * stride + 8, 2), 0x3C, np.uint8)
                rows = host[off:off + F * stride].reshape(F, stride, 2)
                rows[:, :N] = raw
                aligned = [(2 * (off + f * stride)) % 16 == 0 for f in range(F)]
                if F == 65 and stride % 2:
                    assert any(aligned) and not all(aligned), "a launch with both paths"
                got, ws = _raw_call(torch.from_numpy(host).cuda().reshape(-1), 2 * off, F, N, stride, fmt)
                case = (fmt, N, F, stride, off)
                assert _same(got, ref), (case, _where(got, ref))
                head = 4 * N * F if typed else 8 * N * F
                assert (ws[-GUARD:] == 0xA5).all(), case
                if typed:
                    assert len(ws) == _r256(head) + GUARD
                    assert (ws[head:_r256(head)] == 0xA5).all(), case
                    assert ws[:head].view(np.int16).tobytes() == wide16.tobytes(), case
                else:
                    assert ws[:head].view(np.float32).tobytes() == _widen(raw, fmt).view(np.float32).tobytes(), case
                    assert (ws[head:_r256(head)] == 0xA5).all(), case


@pytest.mark.parametrize("N", TYPED_SIZES)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_equals_the_sc16_and_complex64_runs(fmt, N):
    torch = _torch()
    from amcpy_amd.features import features18, features18_iq8, features18_sc16
    raw = np.array(_bytes(37, N))
    raw[5] = 0x00 if fmt == "ci8" else 0x80                        # an all-zero frame
    raw[6] = 0x91                                                  # a frame of one constant
    x8 = torch.from_numpy(_typed(raw, fmt)).cuda()
    x16 = torch.from_numpy(_ints(raw, fmt)).cuda()
    xc = torch.from_numpy(_widen(raw, fmt)).cuda()
    assert (_widen(raw, fmt)[5] == 0).all()
    for name, mask in (("all", _lib.FEATURES_ALL), ("cumulants plan", (1 << 12) | (1 << 14)), ("no spectral", 0x5154)):
        ids = _ids(mask)
        assert "sc16" in _lib.kernel_name_iq8(N, 0, mask)
        got = features18_iq8(x8, feature_ids=ids)
        a = features18_sc16(x16, scale=SCALE, feature_ids=ids)
        b = features18(xc, feature_ids=ids)
        torch.cuda.synchronize()
        got, a, b = got.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy()
        assert _same(got, a), ((fmt, N, name), _where(got, a))
        assert _same(got, b), ((fmt, N, name), _where(got, b))
        if mask != _lib.FEATURES_ALL:
            assert np.isnan(got[:, [j for j in range(18) if not (mask >> j) & 1]]).all()


@pytest.mark.parametrize("N,variant", [(1000, "auto"), (8192, "auto"), (8193, "auto"), (2048, "block")])
def test_sizes_without_an_sc16_kernel(N, variant):
    torch = _torch()
    from amcpy_amd.features import features18, features18_iq8
    lib = _lib.load()
    v = _lib.VARIANTS[variant]
    F = 5
    assert "sc16" not in _lib.kernel_name_iq8(N, v)
    assert lib.amcx_features_iq8_workspace_bytes(N, F, v) == _r256(8 * N * F) + lib.amcx_features18_workspace_bytes(N, F, v)
    for fmt in FORMATS:
        raw = _bytes(F, N)
        got = features18_iq8(torch.from_numpy(_typed(raw, fmt)).cuda(), variant=variant)
        ref = features18(torch.from_numpy(_widen(raw, fmt)).cuda(), variant=variant)
        torch.cuda.synchronize()
        got, ref = got.cpu().numpy(), ref.cpu().numpy()
        assert _same(got, ref), ((fmt, N, variant), _where(got, ref))


def test_chunking_and_capture():
    torch = _torch()
    from amcpy_amd.features import features18_iq8
    lib = _lib.load()
    for N in (2048, 1000):
        raw = _bytes(17, N)
        x8 = torch.from_numpy(_typed(raw, "cu8")).cuda()
        whole = features18_iq8(x8, chunk_frames=17).cpu().numpy()
        for chunk in (5, None):
            got = features18_iq8(x8, chunk_frames=chunk, feature_ids=None).cpu().numpy()
            assert _same(got, whole), (N, chunk)
        # captured with a caller workspace, replayed twice over changed input
        other = torch.from_numpy(_typed(_bytes(17, N, seed=1), "cu8")).cuda()
        eager = [whole, features18_iq8(other).cpu().numpy()]
        assert not _same(eager[0], eager[1])
        need = lib.amcx_features_iq8_workspace_bytes(N, 17, 0)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        xin = x8.clone()
        out = torch.zeros((17, 18), dtype=torch.float32, device="cuda")

        def launch():
            _lib.check(lib.amcx_features_iq8(xin.data_ptr(), 17, N, N, _lib.IQ8_CU8, SCALE, out.data_ptr(), 18,
                                             torch.cuda.current_stream().cuda_stream, 0, _lib.FEATURES_ALL, ws.data_ptr(), need))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            launch()                                               # the stream's first call is outside the capture
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                launch()
        for src, want in ((other, eager[1]), (x8, eager[0])):
            xin.copy_(src)
            out.fill_(-1.0)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert _same(out.cpu().numpy(), want), N


def _device_result(raw, fmt, N, scale=SCALE):
    torch = _torch()
    from amcpy_amd.features import features18_iq8
    y = features18_iq8(torch.from_numpy(_typed(raw, fmt)).cuda(), scale=scale, frame_size=N)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_host_paths_equal_the_device_result(tmp_path):
    from amcpy_amd import sigmf
    from amcpy_amd.feature_extraction import DeviceFanOut, HipEngine, extract_raw_stream
    from amcpy_amd.features import features18_iq8_host
    N, F = 2048, 37
    raw = _bytes(F, N)
    for fmt in FORMATS:
        x = _typed(raw, fmt)
        want = _device_result(raw, fmt, N)
        eng = HipEngine(N, chunk_bytes=48 << 10)                   # 12 frames per slot: 12, 12, 12 and a tail of 1
        try:
            got = eng(x)
            assert _same(got, want), (fmt, _where(got, want))
            assert eng.stats["chunks"] >= 3 and (2 * N * F) % (48 << 10) != 0
            assert eng.stats["pcie_bytes"] == 2 * N * F and eng.stats["source_bytes"] == 2 * N * F
        finally:
            eng.close()
        # the small-call graph: one shape, twice, two scales -- the second must not replay the first's captured scale
        for _ in range(2):
            for scale in (SCALE, 1.0):
                got = features18_iq8_host(x[:3], scale=scale)
                assert _same(got, _device_result(raw[:3], fmt, N, scale)), (fmt, scale)
        # a size without an sc16 kernel, through the host path: widened to complex64 behind the slot
        xo = _bytes(5, 1000)
        assert _same(features18_iq8_host(_typed(xo, fmt)), _device_result(xo, fmt, 1000)), fmt
    # a raw cu8 stream: five leading samples skipped, a trailing partial frame dropped
    path = tmp_path / "capture.cu8"
    path.write_bytes(bytes([7]) * 10 + raw.tobytes() + bytes([9]) * N)
    got = extract_raw_stream(path, N, sample_format="cu8", skip_samples=5)
    assert got.shape == (F, 18) and _same(got, _device_result(raw, "cu8", N))
    # SigMF: two captures, the second behind 6 header bytes, the first no multiple of N
    for fmt in FORMATS:
        n0, n1 = 3 * N + 5, 4 * N + 2
        flat = np.array(_bytes(8, N)).reshape(-1, 2)
        seg0, seg1 = flat[:n0], flat[n0:n0 + n1]
        stem = tmp_path / f"rec_{fmt}"
        Path(str(stem) + ".sigmf-data").write_bytes(seg0.tobytes() + b"\xee" * 6 + seg1.tobytes())
        Path(str(stem) + ".sigmf-meta").write_text(json.dumps({
            "global": {"core:datatype": fmt, "core:version": "1.0.0"},
            "captures": [{"core:sample_start": 0}, {"core:sample_start": n0, "core:header_bytes": 6}]}))
        feats, start = sigmf.extract_sigmf(stem, N)
        assert start.dtype == np.int64 and start.tolist() == [0, N, 2 * N] + [n0 + k * N for k in range(4)]
        want = np.concatenate([_device_result(seg0[:3 * N].reshape(3, N, 2), fmt, N),
                               _device_result(seg1[:4 * N].reshape(4, N, 2), fmt, N)])
        assert _same(feats, want), (fmt, _where(feats, want))
    fan = DeviceFanOut(N, devices=[0])
    try:
        got = fan(_typed(raw, "ci8"))
        assert _same(got, _device_result(raw, "ci8", N))
    finally:
        fan.close()


def test_parity_contract_on_the_widened_frames():
    """The parity contract of tests/test_gpu_parity.py (its criterion, imported) against the float64 oracle evaluated on
    the widened frames: six modulations x SNR (-10, 0, 10, 20) x 4 frames at N = 2048, quantised to 8 bits behind a per-frame
    gain that puts a component's RMS at 30 of 127 -- a receiver's AGC; what still clips, clips, and is part of the frame
    both sides compute on.

    NO TWO NEIGHBOURING SAMPLES ARE EXACTLY ANTIPARALLEL (checked below in integers).  On an 8-bit lattice such pairs are
    common -- the same quantisation leaves 79 of them in 52 of these 96 frames -- and their phase step is +-pi exactly: the
    reference takes its sign from the last bit of two float64 arctangents (d = pi + 1 ulp wraps to -pi, d = pi stays), the
    kernels from the sign of the raw difference (amcx_math.h, exact_step), and in 7 of the 79 the two differ, which moves
    sigma_af and mu42^f by 1e-4 ... 1e-3 of their value.  Neither sign is the right one and the criterion, a relative error
    against the reference, is not defined there (as for the degenerate frames of tests/test_gpu_sc16.py): the second sample
    of each such pair is moved by one LSB across the line through the first.  Frames with exact ties are held to the complex64 path bit for bit by every
    other test of this file, whose random bytes are full of them."""
    torch = _torch()
    from amcpy_amd import synth
    from amcpy_amd.features import features18_iq8
    from oracle import iq_features_oracle as orc
    from tests.test_gpu_parity import _assert_parity
    N = 2048
    x = np.concatenate([synth.host_block(m, snr, 4, N, seed=N + 31 * i + j)
                        for i, m in enumerate(synth.MODS6) for j, snr in enumerate((-10.0, 0.0, 10.0, 20.0))])
    assert x.shape == (96, N)
    parts = np.stack([x.real, x.imag], axis=-1)
    gain = 30.0 / np.sqrt(np.mean(parts ** 2, axis=(1, 2), keepdims=True))
    q = np.clip(np.rint(parts * gain), -128, 127).astype(np.int64)

    def antiparallel(q):
        i, r = q[..., 0], q[..., 1]
        cross = i[:, :-1] * r[:, 1:] - r[:, :-1] * i[:, 1:]
        dot = i[:, :-1] * i[:, 1:] + r[:, :-1] * r[:, 1:]
        return (cross == 0) & (dot < 0)
    for _ in range(8):
        f, n = np.nonzero(antiparallel(q))
        if f.size == 0:
            break
        c = np.where(q[f, n, 1] != 0, 0, 1)                      # the component whose LSB turns the pair: I, or Q behind an on-axis sample
        q[f, n + 1, c] += np.where(q[f, n + 1, c] < 127, 1, -1)
    assert not antiparallel(q).any()
    q = q.astype(np.int8)
    for fmt in FORMATS:
        raw = q.view(np.uint8) if fmt == "ci8" else (q.astype(np.int16) + 128).astype(np.uint8)
        wide = _widen(raw, fmt)
        assert np.array_equal(wide, _widen(q.view(np.uint8), "ci8"))
        gold = orc.features18_batch(wide)
        assert np.isfinite(gold).all()
        got = features18_iq8(torch.from_numpy(_typed(raw, fmt)).cuda())
        torch.cuda.synchronize()
        _assert_parity(got.cpu().numpy(), gold, wide, f"{fmt} N={N}")
