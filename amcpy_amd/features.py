"""The 18 per-frame IQ features on MI355X.

Mirror of the reference's per-frame seam (src/amcpy/features.py:214-232):

    calculate_features(feature_ids, signal) -> list[float]

with the same argument meaning, result order and ``KeyError`` for an unknown
id -- computed by the HIP kernels behind the C ABI (include/amcx.h), never on
the CPU.  The batch entry points the extraction driver uses are
:func:`features18` (torch tensor in HBM -> torch tensor in HBM, asynchronous on
the current stream) and :func:`features18_host` (numpy in, numpy out);
:func:`features18_sc16` / :func:`features18_sc16_host` take 16-bit integer IQ
(int16 (I, Q) pairs: UHD sc16, SigMF ci16_le) as it lies, half the bytes;
:func:`features18_iq8` / :func:`features18_iq8_host` take 8-bit IQ (int8 pairs:
ci8; uint8 pairs: cu8), a quarter of the bytes, which the device widens first.

Feature ids (reference config.py:118-137): 1 gamma_max, 2 sigma_ap,
3 sigma_dp, 4 sigma_aa, 5 sigma_af, 6 X, 7 X2, 8 mu42^a, 9 mu42^f,
10..18 |C20| |C21| |C40| |C41| |C42| |C60| |C61| |C62| |C63|.
"""
from __future__ import annotations

import threading
from typing import Iterable, List

import numpy as np

from . import _lib

FEATURE_IDS = tuple(range(1, _lib.NUM_FEATURES + 1))


def _variant(v) -> int:
    return _lib.VARIANTS[v] if isinstance(v, str) else int(v)


def _mask(feature_ids):
    """None (all 18: the 18-feature entry points) or the feature mask of ``feature_ids`` (KeyError for an unknown id)."""
    return None if feature_ids is None else _lib.feature_mask(feature_ids)


def _frame_size(frame_size, L: int) -> int:
    N = L if frame_size is None else int(frame_size)
    if N > L:
        raise ValueError(f"frame_size {N} exceeds row length {L}")
    return N


def _flat_frames(iq, L: int, N: int, tail: tuple = ()):
    """Flatten the frame tensor (..., L) + tail without a copy -> (lead, n_frames, row_stride in samples).
    ``tail``: the trailing dimensions of one sample -- () for complex64, (2,) for int16 (I, Q) pairs."""
    per = 2 if tail else 1                                  # tensor elements per sample
    lead = iq.shape[:iq.dim() - 1 - len(tail)]
    n_frames = int(np.prod(lead)) if lead else 1
    flat = iq.reshape((n_frames, L) + tail) if iq.dim() != 2 + len(tail) else iq
    if flat.data_ptr() != iq.data_ptr() or (n_frames > 1 and (flat.stride(0) % per if tail else flat.stride(1) != 1)):
        raise ValueError("frames must be uniformly strided (no copy is made)")
    return lead, n_frames, (flat.stride(0) // per if n_frames > 1 else max(L, N))


def _out_frames(iq, out, lead, n_frames: int):
    """Make or validate ``out`` for frames of ``iq`` with leading shape ``lead`` -> (out, oflat, out_stride)."""
    import torch
    if out is None:
        out = torch.empty(lead + (_lib.NUM_FEATURES,), dtype=torch.float32, device=iq.device)
    else:
        if out.dtype != torch.float32 or out.device != iq.device:
            raise TypeError("out must be float32 on the same device")
        if tuple(out.shape[:-1]) != tuple(lead) or out.shape[-1] < _lib.NUM_FEATURES:
            raise ValueError("out must have shape (..., >=18) matching iq")
    oflat = out.reshape(n_frames, out.shape[-1]) if out.dim() != 2 else out
    if oflat.data_ptr() != out.data_ptr() or oflat.stride(-1) != 1:
        raise ValueError("out must be uniformly strided with unit stride in the last dimension")
    return out, oflat, (oflat.stride(0) if n_frames > 1 else out.shape[-1])


def features18(iq, out=None, *, frame_size: int | None = None, variant="auto", feature_ids=None):
    """All 18 features of every frame of a complex64 CUDA(HIP) tensor.

    iq   : torch.complex64 tensor on a GPU, shape (..., L) with unit stride in the
           last dimension and uniformly strided frames (any leading shape that
           flattens to [n_frames][row_stride], e.g. the reference's
           (n_snr, n_frames, L) container).  Only the first ``frame_size``
           samples of each row are used (feature_extraction.py:68).
    out  : optional float32 tensor (..., >=18) on the same device.
    feature_ids : None (all 18), or the ids (1 ... 18) to compute: amcx_features_c64_subset runs only the work they
           need; the output stays 18 wide, the columns asked for bit-identical to the full computation and the others
           NaN.  An unknown id raises ``KeyError`` before anything is launched.
    Returns the float32 tensor (..., 18); the launch is asynchronous on the
    current torch stream.
    """
    import torch

    mask = _mask(feature_ids)

    _lib.require_torch_runtime()
    if not isinstance(iq, torch.Tensor) or iq.dtype != torch.complex64:
        raise TypeError("iq must be a torch.complex64 tensor")
    if not iq.is_cuda:
        raise ValueError("iq must live in GPU memory (use features18_host for numpy input)")
    if iq.dim() < 1:
        raise ValueError("iq needs at least one dimension")
    L = iq.shape[-1]
    N = _frame_size(frame_size, L)
    if iq.stride(-1) != 1 and L > 1:
        raise ValueError("last dimension must have unit stride")
    lead, n_frames, row_stride = _flat_frames(iq, L, N)
    out, oflat, out_stride = _out_frames(iq, out, lead, n_frames)
    lib = _lib.load()
    v = _variant(variant)
    with torch.cuda.device(iq.device):
        stream = torch.cuda.current_stream(iq.device).cuda_stream
        # The any-size path above 8192 samples wants a workspace for its FFT form (amcx_features18_workspace_bytes: 0 for
        # every other size).  It comes from TORCH's allocator here -- the allocator that owns this process's device
        # memory -- through amcx_features18_c64_ws: left to amcx_features18_c64_ex it would come from HIP's own
        # stream-ordered pool, which knows nothing of what torch has cached, and a failed allocation there silently
        # selects the O(N^2) form (~100x slower at N = 32767).  torch raises if it cannot provide the bytes.
        need = int(lib.amcx_features18_workspace_bytes(N, n_frames, v)) if n_frames > 0 else 0
        if mask is not None:
            ws = torch.empty(need, dtype=torch.uint8, device=iq.device) if need > 0 else None
            _lib.check(lib.amcx_features_c64_subset(iq.data_ptr(), n_frames, N, row_stride, oflat.data_ptr(), out_stride,
                                                    stream, v, mask, None if ws is None else ws.data_ptr(), need))
            if ws is not None:
                ws.record_stream(torch.cuda.current_stream(iq.device))
        elif need > 0:
            ws = torch.empty(need, dtype=torch.uint8, device=iq.device)
            _lib.check(lib.amcx_features18_c64_ws(iq.data_ptr(), n_frames, N, row_stride, oflat.data_ptr(), out_stride,
                                                  stream, v, ws.data_ptr(), need))
            ws.record_stream(torch.cuda.current_stream(iq.device))       # freed for reuse behind the launch, not before
        else:
            _lib.check(lib.amcx_features18_c64_ex(
                iq.data_ptr(), n_frames, N, row_stride, oflat.data_ptr(), out_stride, stream, v))
    return out[..., :_lib.NUM_FEATURES]


def features18_iq_pairs(iq_pairs, **kw):
    """Zero-copy entry for data stored as float32 (I, Q) pairs: RadioML-style
    ``(..., N, 2)`` float32 arrays and raw GNU-Radio complex64 streams reshaped to
    ``(F, N, 2)`` (reference old/dataset.py:50-56, old/read_binary_stream.py:28,48) are
    bit-identical to the kernel's complex64 layout, so the tensor is only re-viewed."""
    import torch
    if not isinstance(iq_pairs, torch.Tensor) or iq_pairs.dtype != torch.float32 or iq_pairs.shape[-1] != 2:
        raise TypeError("expected a float32 tensor whose last dimension is (I, Q)")
    if iq_pairs.stride(-1) != 1 or (iq_pairs.shape[-2] > 1 and iq_pairs.stride(-2) != 2):
        raise ValueError("(I, Q) pairs must be interleaved in memory")
    return features18(torch.view_as_complex(iq_pairs), **kw)


# one sc16 sample as numpy sees it: two little-endian int16, I then Q (include/amcx.h, amcx_features_sc16)
SC16 = np.dtype([("i", "<i2"), ("q", "<i2")])


def _sc16_scale(scale) -> float:
    """``scale`` as the float32 the library multiplies by; ValueError unless it is finite and > 0."""
    s = float(np.float32(scale))
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError(f"scale must be a finite float32 > 0, got {scale!r}")
    return s


def sc16_view(pairs: np.ndarray) -> np.ndarray:
    """(..., L, 2) int16 -> (..., L) view of :data:`SC16` samples (no copy).  TypeError for another dtype or a last
    dimension that is not 2, ValueError for pairs that are not interleaved in memory."""
    if not isinstance(pairs, np.ndarray) or pairs.dtype != np.int16 or pairs.ndim < 2 or pairs.shape[-1] != 2:
        raise TypeError("expected an int16 array whose last dimension is (I, Q)")
    if pairs.strides[-1] != 2 or any(st % 4 for st in pairs.strides[:-1]):
        raise ValueError("(I, Q) int16 pairs must be interleaved in memory")
    return pairs.view(SC16)[..., 0]


def features18_sc16(iq, out=None, *, scale=_lib.SC16_SCALE, frame_size: int | None = None, variant="auto",
                    feature_ids=None):
    """The features of every frame of 16-bit integer IQ in GPU memory, read as it lies (amcx_features_sc16).

    iq    : torch.int16 tensor on a GPU, shape (..., L, 2): I then Q, interleaved (unit stride in the last dimension, 2
            in the one before it), frames uniformly strided as for :func:`features18`.
    scale : a finite float32 > 0.  The frame's value is complex64(float32(I) * scale, float32(Q) * scale), and the
            result is BIT-IDENTICAL to :func:`features18` (same variant and feature_ids) on that complex64 frame.
    out, frame_size, variant, feature_ids: as :func:`features18`.
    At 128 ... 4096 (wave / auto) kernels read the int16 themselves; every other size and variant widens the frames
    into a workspace from torch's allocator and runs the complex64 path."""
    import torch

    mask = _lib.FEATURES_ALL if feature_ids is None else _lib.feature_mask(feature_ids)
    scale = _sc16_scale(scale)
    if not isinstance(iq, torch.Tensor) or iq.dtype != torch.int16:
        raise TypeError("iq must be a torch.int16 tensor")
    if iq.dim() < 2 or iq.shape[-1] != 2:
        raise TypeError("iq must have shape (..., L, 2): the last dimension is (I, Q)")
    L = iq.shape[-2]
    if iq.stride(-1) != 1 or (L > 1 and iq.stride(-2) != 2):
        raise ValueError("(I, Q) pairs must be interleaved in memory")
    if not iq.is_cuda:
        raise ValueError("iq must live in GPU memory (use features18_sc16_host for numpy input)")
    N = _frame_size(frame_size, L)
    lead, n_frames, row_stride = _flat_frames(iq, L, N, (2,))
    out, oflat, out_stride = _out_frames(iq, out, lead, n_frames)
    _lib.require_torch_runtime()
    lib = _lib.load()
    v = _variant(variant)
    with torch.cuda.device(iq.device):
        stream = torch.cuda.current_stream(iq.device).cuda_stream
        # the widened copy and the any-size path's FFT workspace, from torch's allocator (see features18)
        need = int(lib.amcx_features_sc16_workspace_bytes(N, n_frames, v)) if n_frames > 0 else 0
        ws = torch.empty(need, dtype=torch.uint8, device=iq.device) if need > 0 else None
        _lib.check(lib.amcx_features_sc16(iq.data_ptr(), n_frames, N, row_stride, scale, oflat.data_ptr(), out_stride,
                                          stream, v, mask, None if ws is None else ws.data_ptr(), max(need, 0)))
        if ws is not None:
            ws.record_stream(torch.cuda.current_stream(iq.device))
    return out[..., :_lib.NUM_FEATURES]


# one 8-bit sample as numpy sees it: two bytes, I then Q (include/amcx.h, amcx_features_iq8) -- int8 (ci8), or uint8
# around the zero level 128 (cu8)
CI8 = np.dtype([("i", "i1"), ("q", "i1")])
CU8 = np.dtype([("i", "u1"), ("q", "u1")])


def _iq8_scale(scale) -> float:
    return _sc16_scale(scale)


def iq8_view(pairs: np.ndarray) -> np.ndarray:
    """(..., L, 2) int8 / uint8 -> (..., L) view of :data:`CI8` / :data:`CU8` samples (no copy).  TypeError for another
    dtype or a last dimension that is not 2, ValueError for pairs that are not interleaved in memory."""
    if not isinstance(pairs, np.ndarray) or pairs.dtype not in (np.int8, np.uint8) or pairs.ndim < 2 or pairs.shape[-1] != 2:
        raise TypeError("expected an int8 or uint8 array whose last dimension is (I, Q)")
    if pairs.strides[-1] != 1 or any(st % 2 for st in pairs.strides[:-1]) or (pairs.shape[-2] > 1 and pairs.strides[-2] != 2):
        raise ValueError("(I, Q) byte pairs must be interleaved in memory")
    return pairs.view(CI8 if pairs.dtype == np.int8 else CU8)[..., 0]


def features18_iq8(iq, out=None, *, scale=_lib.IQ8_SCALE, frame_size: int | None = None, variant="auto",
                   feature_ids=None, chunk_frames: int | None = None):
    """The features of every frame of 8-bit IQ in GPU memory (amcx_features_iq8): widened on the device, then the
    kernels :func:`features18_sc16` (128 ... 4096, wave / auto) or :func:`features18` run.

    iq    : torch.int8 (ci8) or torch.uint8 (cu8: zero level 128) tensor on a GPU, shape (..., L, 2): I then Q,
            interleaved, frames uniformly strided as for :func:`features18`.  The dtype picks the format.
    scale : a finite float32 > 0.  The frame's value is complex64(float32(i) * scale, float32(q) * scale), i, q in
            -128 ... 127, and the result is BIT-IDENTICAL to :func:`features18_sc16` on the int16 of the same values and to
            :func:`features18` on that complex64 frame (same variant and feature_ids).
    chunk_frames : frames per library call.  All calls share ONE workspace from torch's allocator, which holds the widened
            copy of a chunk -- so a resident 8-bit arena need not find a multiple of its own size.  Default (None): all
            frames in one call, the widened copy 2 x (sc16) or 4 x (complex64) the 8-bit frames: a default of 64 MiB
            chunks measured x0.37 ... 0.51 of sc16's rate where one call reaches x0.72 ... 0.77
            (profiles/r14_iq8_bench.json: calls of a few thousand frames are launch-bound).  Frames are independent: the
            result does not depend on it, bit for bit.
    out, frame_size, variant, feature_ids: as :func:`features18`."""
    import torch

    mask = _lib.FEATURES_ALL if feature_ids is None else _lib.feature_mask(feature_ids)
    scale = _iq8_scale(scale)
    if not isinstance(iq, torch.Tensor) or iq.dtype not in (torch.int8, torch.uint8):
        raise TypeError("iq must be a torch.int8 (ci8) or torch.uint8 (cu8) tensor")
    if iq.dim() < 2 or iq.shape[-1] != 2:
        raise TypeError("iq must have shape (..., L, 2): the last dimension is (I, Q)")
    L = iq.shape[-2]
    if iq.stride(-1) != 1 or (L > 1 and iq.stride(-2) != 2):
        raise ValueError("(I, Q) pairs must be interleaved in memory")
    if not iq.is_cuda:
        raise ValueError("iq must live in GPU memory (use features18_iq8_host for numpy input)")
    N = _frame_size(frame_size, L)
    if chunk_frames is not None and int(chunk_frames) < 1:
        raise ValueError("chunk_frames must be at least 1")
    lead, n_frames, row_stride = _flat_frames(iq, L, N, (2,))
    out, oflat, out_stride = _out_frames(iq, out, lead, n_frames)
    _lib.require_torch_runtime()
    lib = _lib.load()
    v = _variant(variant)
    fmt = _lib.IQ8_CI8 if iq.dtype == torch.int8 else _lib.IQ8_CU8
    if n_frames == 0:
        _lib.check(lib.amcx_features_iq8(None, 0, N, row_stride, fmt, scale, None, out_stride, None, v, mask, None, 0))
        return out[..., :_lib.NUM_FEATURES]
    per_call = n_frames if chunk_frames is None else min(int(chunk_frames), n_frames)
    with torch.cuda.device(iq.device):
        cur = torch.cuda.current_stream(iq.device)
        need = int(lib.amcx_features_iq8_workspace_bytes(N, per_call, v))
        if need < 0:                       # the call itself says what is wrong with the arguments
            need = 0
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=iq.device)
        for f0 in range(0, n_frames, per_call):
            n = min(per_call, n_frames - f0)
            _lib.check(lib.amcx_features_iq8(iq.data_ptr() + 2 * f0 * row_stride, n, N, row_stride, fmt, scale,
                                             oflat.data_ptr() + 4 * f0 * out_stride, out_stride, cur.cuda_stream, v, mask,
                                             ws.data_ptr(), need))
        ws.record_stream(cur)
    return out[..., :_lib.NUM_FEATURES]


_tls = threading.local()


def _host_context(device: int) -> "_lib.HostContext":
    """This thread's reusable context for `device` (amcx_ctx_*: stream + device scratch kept
    across calls, so calculate_features in a loop is not allocation-bound)."""
    cache = getattr(_tls, "ctx", None)
    if cache is None:
        cache = _tls.ctx = {}
    ctx = cache.get(device)
    if ctx is None:
        ctx = cache[device] = _lib.HostContext(device)
    return ctx


def _run_on_host_context(ctx, x2: np.ndarray, N: int, lead, variant, mask) -> np.ndarray:
    """The flattened frames ``x2`` through the context ``ctx`` -> (lead..., 18) float32."""
    out = np.empty((x2.shape[0], _lib.NUM_FEATURES), dtype=np.float32)
    ctx.set_feature_mask(_lib.FEATURES_ALL if mask is None else mask)
    ctx.run(x2, N, out, _variant(variant))
    return out.reshape(tuple(lead) + (_lib.NUM_FEATURES,))


def features18_host(frames: np.ndarray, *, frame_size: int | None = None, device: int = 0,
                    variant="auto", feature_ids=None) -> np.ndarray:
    """numpy (..., L) complex -> numpy (..., 18) float32 via the GPU.

    complex128 input (MATLAB doubles) is uploaded as it is and rounded to complex64,
    the engine's input type, on the GPU.  ``feature_ids``: as :func:`features18` (NaN in the
    columns not asked for).  Raises if no MI355X is present (AMCX_ENODEV)."""
    mask = _mask(feature_ids)
    x = np.asarray(frames)
    if not np.iscomplexobj(x):
        x = x.astype(np.complex64)
    L = x.shape[-1]
    N = _frame_size(frame_size, L)
    lead = x.shape[:-1]
    if x.dtype == np.complex128:
        # MATLAB doubles: uploaded as they are, rounded to complex64 on the GPU
        x2 = np.ascontiguousarray(x.reshape(-1, L))
    else:
        x2 = np.ascontiguousarray(x.reshape(-1, L), dtype=np.complex64)
    return _run_on_host_context(_host_context(int(device)), x2, N, lead, variant, mask)


def features18_sc16_host(frames: np.ndarray, *, scale=_lib.SC16_SCALE, frame_size: int | None = None, device: int = 0,
                         variant="auto", feature_ids=None) -> np.ndarray:
    """numpy (..., L, 2) int16 (I, Q) pairs -> numpy (..., 18) float32 via the GPU.  The samples cross the link as
    they lie, 4 bytes each, and are never widened on the host; the result equals :func:`features18_sc16`'s."""
    mask = _mask(feature_ids)
    scale = _sc16_scale(scale)
    x = frames
    if not isinstance(x, np.ndarray) or x.dtype != np.int16 or x.ndim < 2 or x.shape[-1] != 2:
        raise TypeError("expected an int16 array whose last dimension is (I, Q)")
    L = x.shape[-2]
    N = _frame_size(frame_size, L)
    lead = x.shape[:-2]
    x2 = np.ascontiguousarray(x.reshape(-1, L, 2))
    ctx = _host_context(int(device))
    ctx.set_sc16_scale(scale)
    return _run_on_host_context(ctx, x2, N, lead, variant, mask)


def calculate_features(feature_ids: Iterable[int], signal, *, device: int = 0,
                       variant="auto") -> List[float]:
    """Drop-in for the reference's ``calculate_features`` (features.py:214-232):
    values in the order of ``feature_ids`` (repeats and subsets allowed); an id
    outside 1..18 raises ``KeyError`` before anything is launched.  Only the
    features asked for are computed (features18_host(feature_ids=...)); the values
    are bit-identical to those of a full computation."""
    ids = list(feature_ids)
    for fid in ids:
        if fid not in FEATURE_IDS:
            raise KeyError(fid)
    sig = np.asarray(signal)
    if sig.ndim != 1:
        raise ValueError("signal must be one frame (1-D complex array)")
    if not ids:
        return []
    row = features18_host(sig[None, :], device=device, variant=variant, feature_ids=ids)[0]
    return [float(row[fid - 1]) for fid in ids]


def features18_iq8_host(frames: np.ndarray, *, scale=_lib.IQ8_SCALE, frame_size: int | None = None, device: int = 0,
                        variant="auto", feature_ids=None) -> np.ndarray:
    """numpy (..., L, 2) int8 (ci8) / uint8 (cu8) (I, Q) pairs -> numpy (..., 18) float32 via the GPU.  The samples cross
    the link as they lie, 2 bytes each, and are widened by the device; the result equals :func:`features18_iq8`'s."""
    mask = _mask(feature_ids)
    scale = _iq8_scale(scale)
    x = frames
    if not isinstance(x, np.ndarray) or x.dtype not in (np.int8, np.uint8) or x.ndim < 2 or x.shape[-1] != 2:
        raise TypeError("expected an int8 or uint8 array whose last dimension is (I, Q)")
    L = x.shape[-2]
    N = _frame_size(frame_size, L)
    lead = x.shape[:-2]
    x2 = np.ascontiguousarray(x.reshape(-1, L, 2))
    ctx = _host_context(int(device))
    ctx.set_iq8_scale(scale)
    return _run_on_host_context(ctx, x2, N, lead, variant, mask)
