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

from . import _formats, _lib
from ._formats import CI8, CU8, SC16, iq8_view, sc16_view  # noqa: F401  (their home; imported from here by name)

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
    return _features_on_device(iq, out, _formats.get("cf32"), L, N, variant, mask)


def _features_on_device(iq, out, fmt, L: int, N: int, variant, mask, scale=None, chunk_frames=None):
    """What :func:`features18`, :func:`features18_sc16` and :func:`features18_iq8` do once their arguments have passed: the
    frames of ``iq`` (samples of ``fmt``, rows of L of which N are used) flattened, ``out`` made or checked, the workspace
    taken from torch's allocator, the library called on the current stream -- once, or, ``chunk_frames``, once per chunk --
    and the (..., 18) result."""
    import torch

    family = fmt.family
    lead, n_frames, row_stride = _flat_frames(iq, L, N, fmt.tail)
    out, oflat, out_stride = _out_frames(iq, out, lead, n_frames)
    _lib.require_torch_runtime()
    lib = _lib.load()
    v = _variant(variant)
    if family is None:
        query = lib.amcx_features18_workspace_bytes
    else:
        query, entry = getattr(lib, f"amcx_features_{family}_workspace_bytes"), getattr(lib, f"amcx_features_{family}")
        head = (scale,) if fmt.iq8 is None else (fmt.iq8, scale)
    if n_frames == 0 and family == "iq8":                  # nothing to widen: the call only checks the other arguments
        _lib.check(entry(None, 0, N, row_stride, *head, None, out_stride, None, v, mask, None, 0))
        return out[..., :_lib.NUM_FEATURES]
    per_call = n_frames if chunk_frames is None else min(int(chunk_frames), n_frames)
    with torch.cuda.device(iq.device):
        cur = torch.cuda.current_stream(iq.device)
        # The workspace -- the widened copy of the integer frames that no kernel reads as they lie, and what the any-size
        # path above 8192 samples wants for its FFT form; 0 bytes for complex64 at every other size -- comes from TORCH's
        # allocator, the one that owns this process's device memory: left to amcx_features18_c64_ex it would come from
        # HIP's own stream-ordered pool, which knows nothing of what torch has cached, and a failed allocation there
        # silently selects the O(N^2) form (~100x slower at N = 32767).  torch raises if it cannot provide the bytes.
        # (A negative answer: the call itself says what is wrong with the arguments.)
        need = max(0, int(query(N, per_call, v))) if n_frames > 0 else 0
        ws = torch.empty(need, dtype=torch.uint8, device=iq.device) if need > 0 else None
        ws_ptr = None if ws is None else ws.data_ptr()
        for f0 in range(0, max(n_frames, 1), max(per_call, 1)):              # (no frames: still the one call)
            src = (iq.data_ptr() + fmt.store.itemsize * f0 * row_stride, min(per_call, n_frames - f0), N, row_stride)
            dst = (oflat.data_ptr() + 4 * f0 * out_stride, out_stride, cur.cuda_stream, v)
            if family is not None:
                rc = entry(*src, *head, *dst, mask, ws_ptr, need)
            elif mask is not None:
                rc = lib.amcx_features_c64_subset(*src, *dst, mask, ws_ptr, need)
            elif need > 0:
                rc = lib.amcx_features18_c64_ws(*src, *dst, ws_ptr, need)
            else:                                          # allocates nothing: what a resident caller under graph capture runs
                rc = lib.amcx_features18_c64_ex(*src, *dst)
            _lib.check(rc)
        if ws is not None:
            ws.record_stream(cur)                          # freed for reuse behind the launch, not before
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


def _pairs_on_device(iq, out, family: str, what: str, scale, frame_size, variant, feature_ids, chunk_frames=None):
    """:func:`features18_sc16` (``family`` "sc16") and :func:`features18_iq8` ("iq8"): their checks, in their order."""
    import torch

    mask = _lib.FEATURES_ALL if feature_ids is None else _lib.feature_mask(feature_ids)
    scale = _formats.check_scale(scale)
    fmt = _formats.by_plain(iq.dtype) if isinstance(iq, torch.Tensor) else None
    if fmt is None or fmt.family != family:
        raise TypeError(f"iq must be a {what} tensor")
    if iq.dim() < 2 or iq.shape[-1] != 2:
        raise TypeError("iq must have shape (..., L, 2): the last dimension is (I, Q)")
    L = iq.shape[-2]
    if iq.stride(-1) != 1 or (L > 1 and iq.stride(-2) != 2):
        raise ValueError("(I, Q) pairs must be interleaved in memory")
    if not iq.is_cuda:
        raise ValueError(f"iq must live in GPU memory (use features18_{family}_host for numpy input)")
    N = _frame_size(frame_size, L)
    if chunk_frames is not None and int(chunk_frames) < 1:
        raise ValueError("chunk_frames must be at least 1")
    return _features_on_device(iq, out, fmt, L, N, variant, mask, scale, chunk_frames)


def features18_sc16(iq, out=None, *, scale=_formats.get("sc16").scale, frame_size: int | None = None, variant="auto",
                    feature_ids=None):
    """The features of every frame of 16-bit integer IQ in GPU memory, read as it lies (amcx_features_sc16).

    iq    : torch.int16 tensor on a GPU, shape (..., L, 2): I then Q, interleaved (unit stride in the last dimension, 2
            in the one before it), frames uniformly strided as for :func:`features18`.
    scale : a finite float32 > 0.  The frame's value is complex64(float32(I) * scale, float32(Q) * scale), and the
            result is BIT-IDENTICAL to :func:`features18` (same variant and feature_ids) on that complex64 frame.
    out, frame_size, variant, feature_ids: as :func:`features18`.
    At 128 ... 4096 (wave / auto) kernels read the int16 themselves; every other size and variant widens the frames
    into a workspace from torch's allocator and runs the complex64 path."""
    return _pairs_on_device(iq, out, "sc16", "torch.int16", scale, frame_size, variant, feature_ids)


def features18_iq8(iq, out=None, *, scale=_formats.get("ci8").scale, frame_size: int | None = None, variant="auto",
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
    return _pairs_on_device(iq, out, "iq8", "torch.int8 (ci8) or torch.uint8 (cu8)", scale, frame_size, variant, feature_ids,
                            chunk_frames)


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


def _features_on_host(x: np.ndarray, tail: tuple, frame_size, device, variant, mask, fmt=None, scale=None) -> np.ndarray:
    """What the three host entries do once their arguments have passed: the frames (..., L) + tail, made contiguous, through
    this thread's context (at ``scale`` for the integer format ``fmt``) -> (..., 18) float32."""
    L = x.shape[x.ndim - 1 - len(tail)]
    N = _frame_size(frame_size, L)
    lead = x.shape[:x.ndim - 1 - len(tail)]
    x2 = np.ascontiguousarray(x.reshape((-1, L) + tail))
    ctx = _host_context(int(device))
    if fmt is not None:
        ctx.set_scale(fmt.name, scale)
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
    if x.dtype != np.complex128:                            # (MATLAB doubles alone go up as they are)
        x = x.astype(np.complex64, copy=False)
    return _features_on_host(x, (), frame_size, device, variant, mask)


def _pairs_on_host(frames, family: str, what: str, scale, frame_size, device, variant, feature_ids) -> np.ndarray:
    """:func:`features18_sc16_host` (``family`` "sc16") and :func:`features18_iq8_host` ("iq8"): their checks, in their order."""
    mask = _mask(feature_ids)
    scale = _formats.check_scale(scale)
    fmt = _formats.by_plain(frames.dtype) if isinstance(frames, np.ndarray) else None
    if fmt is None or fmt.family != family or frames.ndim < 2 or frames.shape[-1] != 2:
        raise TypeError(f"expected an {what} array whose last dimension is (I, Q)")
    return _features_on_host(frames, fmt.tail, frame_size, device, variant, mask, fmt, scale)


def features18_sc16_host(frames: np.ndarray, *, scale=_formats.get("sc16").scale, frame_size: int | None = None,
                         device: int = 0, variant="auto", feature_ids=None) -> np.ndarray:
    """numpy (..., L, 2) int16 (I, Q) pairs -> numpy (..., 18) float32 via the GPU.  The samples cross the link as
    they lie, 4 bytes each, and are never widened on the host; the result equals :func:`features18_sc16`'s."""
    return _pairs_on_host(frames, "sc16", "int16", scale, frame_size, device, variant, feature_ids)


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


def features18_iq8_host(frames: np.ndarray, *, scale=_formats.get("ci8").scale, frame_size: int | None = None,
                        device: int = 0, variant="auto", feature_ids=None) -> np.ndarray:
    """numpy (..., L, 2) int8 (ci8) / uint8 (cu8) (I, Q) pairs -> numpy (..., 18) float32 via the GPU.  The samples cross
    the link as they lie, 2 bytes each, and are widened by the device; the result equals :func:`features18_iq8`'s."""
    return _pairs_on_host(frames, "iq8", "int8 or uint8", scale, frame_size, device, variant, feature_ids)
