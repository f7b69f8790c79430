"""16-bit integer IQ (sc16: include/amcx.h, ABI 9) on the GPU.

THE ORACLE IS EXACT.  int16 -> float32 is exact and the product with a float32 scale is one IEEE rounding, so the frame an
sc16 call computes on is ``x.astype(float32) * float32(scale)`` -- built here with numpy or torch, never by the code under
test -- and the sc16 result must equal the EXISTING complex64 path on that frame, same variant and feature mask, bit for
bit (``array_equal`` with ``equal_nan``): the kernels that read int16 themselves (128 ... 4096), the N = 2048 ring and LDS
forms, the widening path of every other size and variant, and the host paths.  The parity contract against the float64
oracle is checked with the criterion of tests/test_gpu_parity.py, imported, not copied."""
import functools

import numpy as np
import pytest

from amcpy_amd import _lib

pytestmark = pytest.mark.gpu

TYPED_SIZES = [128, 256, 512, 1024, 2048, 4096]
MASKS = {"all": _lib.FEATURES_ALL, "no_spectral": _lib.FEATURES_NO_SPECTRAL, "cumulants": _lib.FEATURES_CUMULANTS,
         "used": 0x5154, "id13": 1 << 12}
SCALES = [2.0 ** -15, 1.0, float(np.float32(1.0 / 30000.0)), 2.0 ** 40, 2.0 ** -60]   # 2^40, 2^-60: the range re-run


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _ids(mask):
    return [j + 1 for j in range(18) if (mask >> j) & 1]


def _quantise(x):
    """complex -> (F, N, 2) int16: round(x * 2048), clipped."""
    q = np.stack([x.real, x.imag], axis=-1)
    return np.clip(np.rint(q * 2048.0), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _signal_frames(N, per_cell=3):
    """synth.host_block for six modulations x SNR (-10, 10, 40) and noiseless balanced QPSK (the cancellation path)."""
    from amcpy_amd import synth
    blocks = [synth.host_block(m, snr, per_cell, N, seed=N + 31 * i + j)
              for i, m in enumerate(synth.MODS6) for j, snr in enumerate((-10.0, 10.0, 40.0))]
    rng = np.random.default_rng(N)
    pts = np.exp(1j * (np.pi / 4 + np.pi / 2 * np.arange(4)))
    n_sym = -(-N // 8)
    for _ in range(6):
        sym = np.concatenate([rng.choice([0, 2], n_sym // 2), rng.choice([1, 3], n_sym - n_sym // 2)])
        rng.shuffle(sym)
        blocks.append((np.repeat(pts[sym], 8)[:N] * np.exp(1j * rng.uniform(0, 2 * np.pi)))[None, :])
    out = _quantise(np.concatenate(blocks))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _frames(N):
    """(F, N, 2) int16, read-only: the signal frames and the degenerate ones."""
    rng = np.random.default_rng(1000 + N)
    n = np.arange(N)
    alt = np.where(n % 2 == 0, 1, -1)
    special = np.zeros((11, N, 2), np.int16)
    special[0, :, 0] = 1000 * alt                                  # alternating sign: every phase step is +-pi
    special[1, :, 0], special[1, :, 1] = 700 * alt, 700 * alt
    special[2, :, 0], special[2, :, 1] = 1200 * alt, rng.integers(-1, 2, N)   # ... and within a rounding of it
    special[3, :, 0], special[3, :, 1] = -32768 * (alt < 0) + 32767 * (alt > 0), 0
    # special[4]: all zeros
    special[5, :, 0], special[5, :, 1] = 123, -45                  # a constant
    special[6, N // 3, 0], special[6, N // 3, 1] = -7, 3           # one non-zero sample
    special[7] = rng.integers(-1, 2, (N, 2))                       # +-1 LSB noise
    special[8] = rng.choice(np.array([-32768, 32767], np.int16), (N, 2))      # full scale, -32768 included
    special[9] = rng.integers(-32768, 32768, (N, 2))
    special[10] = -32768
    out = np.concatenate([_signal_frames(N), special])
    out.setflags(write=False)
    return out


def _three_per_modulation(N):
    """(18, N, 2) int16: three frames of EACH of the six modulations, one per SNR (-10, 10, 40).  _signal_frames is ordered
    modulation, SNR, frame -- nine rows per modulation -- so row 9 m + 3 j is modulation m's first frame at SNR j."""
    rows = [9 * m + 3 * j for m in range(6) for j in range(3)]
    return np.ascontiguousarray(_signal_frames(N)[rows])


def _widen(x16, scale):
    """THE REFERENCE FRAME: complex64(float32(I) * scale, float32(Q) * scale), with numpy."""
    w = x16.astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(w).view(np.complex64)[..., 0]


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _where(a, b):
    return np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b)))).tolist()[:8]


def _ref(xc_dev, N, variant, mask):
    """the complex64 path on widened frames (device tensor) -> numpy (F, 18)"""
    torch = _torch()
    from amcpy_amd.features import features18
    y = features18(xc_dev, frame_size=N, variant=variant, feature_ids=None if mask == _lib.FEATURES_ALL else _ids(mask))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _sc16(x16_dev, N, variant, mask, scale, count=None, out_cols=21):
    """features18_sc16 on the first `count` rows of a (F, L, 2) int16 device tensor; 21 output columns, the last three
    a sentinel that must stay"""
    torch = _torch()
    from amcpy_amd.features import features18_sc16
    x = x16_dev if count is None else x16_dev[:count]
    out = torch.full((x.shape[0], out_cols), -5.0, dtype=torch.float32, device="cuda")
    features18_sc16(x, out=out, scale=scale, frame_size=N, variant=variant,
                    feature_ids=None if mask == _lib.FEATURES_ALL else _ids(mask))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:, 18:] == -5.0).all(), "columns beyond 18 were written"
    return got[:, :18]


@pytest.mark.parametrize("N", TYPED_SIZES)
def test_typed_kernels_equal_the_widened_complex64_run(N):
    """1. The kernels that read int16 themselves: every size, variant, mask, scale and frame count, rows N + 13 samples
    apart (4-byte aligned, not 8), 21 output columns."""
    torch = _torch()
    x16 = _frames(N)
    F = x16.shape[0]
    assert F - 1 > 64                                              # more than one finaliser batch of every kernel
    pad = np.full((F, N + 13, 2), 12345, np.int16)
    pad[:, :N] = x16
    xd = torch.from_numpy(pad).cuda()
    for mask_name in MASKS:
        for variant in ("wave", "auto"):
            assert "sc16" in _lib.kernel_name_sc16(N, _lib.VARIANTS[variant], MASKS[mask_name])
    for scale in SCALES:
        wide = torch.from_numpy(_widen(x16, scale)).cuda()
        for mask_name, mask in MASKS.items():
            for variant in ("wave", "auto"):
                ref = _ref(wide, N, variant, mask)
                for count in (1, 37, F - 1):
                    got = _sc16(xd, N, variant, mask, scale, count)
                    assert _same(got, ref[:count]), ((N, scale, mask_name, variant, count), _where(got, ref[:count]))
        if scale in (2.0 ** 40, 2.0 ** -60):                       # the re-run path was taken, and gave numbers: the
            full = _ref(wide, N, "wave", _lib.FEATURES_ALL)        # scale-free features 2 ... 5 are finite there
            assert np.isfinite(full[:3, 1:5]).all()


def test_ring_and_lds_forms_at_2048():
    """2. N = 2048: the ring form (64 frames per wave finalised at a time) at the counts around a batch and at one that
    fills every wave's ring and leaves three frames over; a captured graph, which runs the LDS form, equals the eager
    call on both replays."""
    torch = _torch()
    from amcpy_amd.features import features18, features18_sc16
    N, scale = 2048, 2.0 ** -15
    assert "wave_sc16_kernel<2048>" in _lib.kernel_name_sc16(N)
    base = torch.from_numpy(np.array(_frames(N))).cuda()
    rng = np.random.default_rng(5)
    big = 256 * 16 * 64 + 3
    idx = torch.from_numpy(rng.integers(0, base.shape[0], size=big)).cuda()
    x = base[idx].contiguous()                                                     # (big, N, 2) int16, drawn with replacement
    wide = torch.view_as_complex((x.to(torch.float32) * np.float32(scale)).contiguous())   # widened with torch, exactly
    ref = features18(wide, variant="wave")
    for count in (1, 63, 64, 65, big):
        got = features18_sc16(x[:count], scale=scale, variant="wave")
        r = ref[:count]
        ok = ((got == r) | (got.isnan() & r.isnan())).all()
        torch.cuda.synchronize()
        assert bool(ok), count
    del wide, ref
    # graph capture: no ring under capture, so the LDS form runs
    xs = x[:4099]
    eager = features18_sc16(xs, scale=scale).cpu().numpy()
    out = torch.zeros((xs.shape[0], 18), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        features18_sc16(xs, out=out, scale=scale)                  # the stream's first call is outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            features18_sc16(xs, out=out, scale=scale)
    for _ in range(2):
        out.fill_(-1.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy(), eager)


@pytest.mark.parametrize("N,variant", [(1000, "auto"), (8192, "auto"), (16384, "auto"), (32767, "auto"), (2048, "block"),
                                       (8192, "block")])
def test_sizes_without_a_typed_kernel(N, variant):
    """3. Every other size and variant: widened into the workspace, then the complex64 path unchanged."""
    torch = _torch()
    lib = _lib.load()
    v = _lib.VARIANTS[variant]
    x16 = _three_per_modulation(N)
    F = x16.shape[0]
    need = lib.amcx_features_sc16_workspace_bytes(N, F, v)
    head = (8 * N * F + 255) // 256 * 256
    assert need == head + lib.amcx_features18_workspace_bytes(N, F, v) and need > 0
    assert "sc16" not in _lib.kernel_name_sc16(N, v)
    for typed in TYPED_SIZES:
        assert lib.amcx_features_sc16_workspace_bytes(typed, F, _lib.VARIANT_AUTO) == 0
    xd = torch.from_numpy(np.array(x16)).cuda()
    for scale in (2.0 ** -15, float(np.float32(1.0 / 30000.0))):
        wide = torch.from_numpy(_widen(x16, scale)).cuda()
        for mask in (_lib.FEATURES_ALL, 0x5154):
            ref = _ref(wide, N, variant, mask)
            got = _sc16(xd, N, variant, mask, scale)
            assert _same(got, ref), ((N, variant, scale, mask), _where(got, ref))
    # a workspace that does not hold the widened copy
    out = torch.zeros((F, 18), dtype=torch.float32, device="cuda")
    ws = torch.zeros(head, dtype=torch.uint8, device="cuda")
    for short in (0, head - 256):
        rc = lib.amcx_features_sc16(xd.data_ptr(), F, N, N, 2.0 ** -15, out.data_ptr(), 18, None, v, _lib.FEATURES_ALL,
                                    ws.data_ptr() if short else None, short)
        assert rc == _lib.EINVAL, short
    torch.cuda.synchronize()
    assert (out == 0).all()


@pytest.mark.parametrize("N", [128, 1024, 2048, 4096])
def test_parity_contract_on_the_widened_frames(N):
    """4. The parity contract of tests/test_gpu_parity.py (its criterion, imported) against the float64 oracle evaluated
    on the widened frames: the six modulations x SNR (-10, 10, 40).  The noiseless QPSK frames are not in it: quantised,
    their envelope is constant to the bit, the reference's own mu42^a of them is NaN (0 / 0) and its |C41|, |C61| exactly
    0, and the criterion -- a relative error -- is not defined there; such frames belong to the degenerate-frame rule of
    tests/test_gpu_parity.py::test_golden_edges, and the tests above hold them to the complex64 path bit for bit."""
    torch = _torch()
    from oracle import iq_features_oracle as orc
    from tests.test_gpu_parity import _assert_parity
    x16 = _signal_frames(N)[:54]
    for scale in (2.0 ** -15, 1.0):
        wide = _widen(x16, scale)
        gold = orc.features18_batch(wide)
        assert np.isfinite(gold).all()
        got = _sc16(torch.from_numpy(np.array(x16)).cuda(), N, "auto", _lib.FEATURES_ALL, scale)
        _assert_parity(got, gold, wide, f"sc16 N={N} scale={scale}")


def _device_result(x16, N, scale, mask=_lib.FEATURES_ALL, variant="auto"):
    torch = _torch()
    return _sc16(torch.from_numpy(np.ascontiguousarray(x16)).cuda(), N, variant, mask, scale)


def test_host_paths_equal_the_device_result(tmp_path):
    """5. features18_sc16_host and HipEngine: the small-graph path (one frame, two scales on one shape), a call cut into
    chunks, a call above 1 MiB (staging threads); the bytes over the link are 4 N F; a raw sc16 stream from its file."""
    from amcpy_amd.feature_extraction import HipEngine, extract_raw_stream
    from amcpy_amd.features import features18_sc16_host
    N = 2048
    x16 = np.array(_frames(N))
    # one frame, twice, two scales: the second must not replay the first's captured scale
    for _ in range(2):
        for scale in (2.0 ** -15, 1.0):
            got = features18_sc16_host(x16[3:4], scale=scale)
            assert _same(got, _device_result(x16[3:4], N, scale)), scale
    got = features18_sc16_host(x16[:5], scale=2.0 ** -15, feature_ids=_ids(0x5154))
    assert _same(got, _device_result(x16[:5], N, 2.0 ** -15, 0x5154))
    # sizes without a typed kernel, through the host path: widened on the device behind the slot
    for n_other, variant in ((1000, "auto"), (2048, "block")):
        xo = _three_per_modulation(n_other)
        assert _same(features18_sc16_host(xo, scale=1.0, variant=variant), _device_result(xo, n_other, 1.0, variant=variant))
    # several chunks
    eng = HipEngine(N, chunk_bytes=64 << 10, sc16_scale=2.0 ** -15)
    try:
        F = x16.shape[0]
        got = eng(x16)
        assert _same(got, _device_result(x16, N, 2.0 ** -15))
        assert eng.stats["chunks"] > 1
        assert eng.stats["pcie_bytes"] == 4 * N * F and eng.stats["source_bytes"] == 4 * N * F
    finally:
        eng.close()
    # above 1 MiB: the staging threads
    rng = np.random.default_rng(3)
    big = x16[rng.integers(0, x16.shape[0], 300)]
    assert big.nbytes > (1 << 20)
    eng = HipEngine(N, sc16_scale=float(np.float32(1.0 / 30000.0)))
    try:
        got = eng(big)
        assert _same(got, _device_result(big, N, float(np.float32(1.0 / 30000.0))))
        assert eng.stats["pcie_bytes"] == 4 * N * 300 and eng.stats["source_bytes"] == 4 * N * 300
        assert eng.stats["gather_threads"] >= 1
    finally:
        eng.close()
    # a raw stream: five leading samples skipped, a trailing partial frame dropped
    path = tmp_path / "capture.sc16"
    lead = np.full((5, 2), 77, np.int16)
    tail = np.full((N // 2, 2), -3, np.int16)
    path.write_bytes(lead.tobytes() + x16[:40].tobytes() + tail.tobytes())
    got = extract_raw_stream(path, N, sample_format="sc16", skip_samples=5, scale=2.0 ** -15)
    assert got.shape == (40, 18)
    assert _same(got, _device_result(x16[:40], N, 2.0 ** -15))


def test_misuse_is_refused():
    """6. A scale that is not a finite float32 > 0, a base pointer that is not 4-byte aligned, planes of sc16."""
    torch = _torch()
    lib = _lib.load()
    N = 1024
    x = torch.zeros((4, N + 1, 2), dtype=torch.int16, device="cuda")
    out = torch.zeros((4, 18), dtype=torch.float32, device="cuda")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        rc = lib.amcx_features_sc16(x.data_ptr(), 4, N, N + 1, bad, out.data_ptr(), 18, None, 0, _lib.FEATURES_ALL, None, 0)
        assert rc == _lib.EINVAL, bad
    rc = lib.amcx_features_sc16(x.data_ptr() + 2, 4, N, N + 1, 1.0, out.data_ptr(), 18, None, 0, _lib.FEATURES_ALL, None, 0)
    assert rc == _lib.EINVAL
    rc = lib.amcx_features_sc16(x.data_ptr() + 4, 3, N, N + 1, 1.0, out.data_ptr(), 18, None, 0, _lib.FEATURES_ALL, None, 0)
    assert rc == _lib.OK                                           # 4-byte aligned is enough
    torch.cuda.synchronize()
    ctx = _lib.HostContext(0)
    try:
        planes = np.zeros((N, 8, 2), np.int16)                     # [sample][frame]: the frame axis contiguous
        res = np.zeros((8, 18), np.float32)
        with pytest.raises(_lib.AmcxError) as err:
            ctx.run_strided(planes.ctypes.data, None, _lib.SRC_SC16, 1, 8, N, (0, 1, 8), res)
        assert err.value.code == _lib.ENOTSUP
        with pytest.raises(ValueError):
            ctx.set_scale("sc16", 0.0)
    finally:
        ctx.close()
