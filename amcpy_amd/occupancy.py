"""Occupancy detection on a (channel x frame) grid in GPU memory (include/amcx.h, ABI 14): which cells of a raster hold an
emitter, how far above the noise floor, and the features of those cells alone.

A CELL is one frame of N complex64 samples of one channel: row ``r = c * K + k`` of the ``(C * K, N)`` matrix the filter
bank's ``(C, M)`` output is cut into.

    power = row_power(frames)                      # (C * K,) float32, one read of the samples
    occ = detect(power.view(C, K))                 # floor per frame, mask, ascending row list, SNR per cell
    feats = occupied_features(frames_CKN, occ)     # (C, K, 18), NaN where nothing was detected
    segments(occ.mask.cpu().numpy())               # [(channel, first_frame, last_frame), ...]

WHAT THE DETECTOR ASSUMES.  The floor of frame k is a RANK STATISTIC across that frame's C channels: the element of rank
``floor_rank = int(floor_quantile * (C - 1))`` (ascending, NaN last) of their powers.  It is the noise floor only where at
least ``floor_rank + 1`` channels of every frame are free -- a raster whose channels are all occupied has no floor to find, and
everything in it reads as noise.  A cell is occupied where its power exceeds ``threshold`` times that floor (one float32
product, one comparison).  Nothing is smoothed over time and there is no hysteresis: a cell is judged on its own frame.

Every call is one C-ABI entry on the current torch stream; :func:`detect` reads the number of occupied rows back, its one
host synchronisation.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _lib, _stream

_TINY = float(np.finfo(np.float32).tiny)
Occupancy = namedtuple("Occupancy", "mask floor rows snr_db")
Occupancy.__doc__ = """``mask`` (C, K) bool, ``floor`` (K,) float32, ``rows`` (n,) int32 ascending (r = c * K + k), ``snr_db`` (C, K) float32."""


def floor_rank_of(channels: int, floor_quantile: float) -> int:
    """``int(floor_quantile * (C - 1))``: the rank (0-based, ascending) of the channel power that serves as a frame's floor."""
    q = float(floor_quantile)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"floor_quantile must lie in [0, 1], got {floor_quantile!r}")
    return int(q * (int(channels) - 1))


def threshold_of(threshold_db: float) -> np.float32:
    """``float32(10 ** (threshold_db / 10))``: the factor over the floor at which a cell counts as occupied."""
    with np.errstate(over="ignore"):
        t = np.float32(10.0 ** (float(threshold_db) / 10.0))
    if not (np.isfinite(t) and t > 0):
        raise ValueError(f"threshold_db {threshold_db!r} gives no finite float32 factor > 0")
    return t


def snr_db(power, floor, axis: int):
    """Ten times the decimal logarithm of ``max(power / floor - 1, tiny)`` in float32, tiny the smallest normal float32: how
    far a cell lies above its floor, -379 dB where it does not.  ``power`` float32, numpy or torch; ``floor`` of the same kind, one value per index of
    ``power``'s ``axis``."""
    shape = [1] * power.ndim
    shape[axis] = -1
    if isinstance(power, np.ndarray):
        log10, at_least = np.log10, np.maximum
    else:
        import torch
        log10, at_least = torch.log10, lambda v, least: torch.clamp(v, min=least)
    with np.errstate(all="ignore"):
        return 10.0 * log10(at_least(power / floor.reshape(shape) - 1.0, _TINY))


def _rows_of(frames, what: str):
    import torch
    return _stream.rows_of(frames, torch.complex64, what, "N", 2, narrow="rows of at least 2 samples")


def row_power(frames):
    """``power[r] = sum_n |frames[r, n]|^2`` in float32: complex64 ``(R, N)`` on the GPU, contiguous rows at a row stride >= N
    -> float32 ``(R,)``.  A row's bits depend on its N samples alone (include/amcx.h)."""
    import torch

    R, N, stride = _rows_of(frames, "frames")
    power = torch.empty((R,), dtype=torch.float32, device=frames.device)
    _stream.launch(frames, lambda lib, stream: lib.amcx_row_power_c64(
        frames.data_ptr() if R else None, R, N, stride, power.data_ptr() if R else None, stream))
    return power


def detect(power, *, floor_quantile: float = 0.25, threshold_db: float = 6.0) -> Occupancy:
    """``power``: float32 ``(C, K)`` on the GPU, contiguous, 2 <= C <= 256 -> :class:`Occupancy` (the module's docstring says
    what the detector assumes).  ``snr_db`` is :func:`snr_db` of every cell over its frame's floor, computed with torch: a label
    for the user, no part of the detection."""
    import torch

    if not isinstance(power, torch.Tensor) or power.dtype != torch.float32 or power.dim() != 2:
        raise TypeError("power must be a float32 (C, K) torch tensor")
    if not power.is_cuda or not power.is_contiguous():
        raise ValueError("power must be contiguous in GPU memory")
    C, K = int(power.shape[0]), int(power.shape[1])
    rank, thr = floor_rank_of(C, floor_quantile), threshold_of(threshold_db)
    lib = _lib.load()
    need = lib.amcx_occupancy_workspace_bytes(C, K)
    if need < 0:
        raise ValueError(f"a grid of {C} channels x {K} frames is outside 2 <= C <= 256, C K < 2^31")
    dev = power.device
    floor = torch.empty((K,), dtype=torch.float32, device=dev)
    mask = torch.empty((C, K), dtype=torch.uint8, device=dev)
    rows = torch.empty((C * K,), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(need, 4),), dtype=torch.uint8, device=dev)
    _stream.launch(power, lambda lib_, stream: lib_.amcx_occupancy_detect_f32(
        power.data_ptr() if K else None, C, K, rank, float(thr), floor.data_ptr() if K else None, mask.data_ptr() if K else None,
        rows.data_ptr() if K else None, count.data_ptr(), ws.data_ptr(), need, stream))
    snr = snr_db(power, floor, 1)
    n = int(count.item())                                   # the one host synchronisation
    return Occupancy(mask.bool(), floor, rows[:n], snr)


def gather_rows(frames, rows):
    """``frames[rows]`` as packed complex64 ``(n, N)``: frames complex64 ``(R, N)`` as :func:`row_power` takes it, ``rows``
    int32 ``(n,)`` on the same device.  A copy, bit for bit; an index outside ``[0, R)`` gives a row of NaN."""
    import torch

    R, N, stride = _rows_of(frames, "frames")
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.dim() != 1 or rows.device != frames.device:
        raise TypeError("rows must be a one-dimensional int32 tensor on frames' device")
    rows = rows.contiguous()
    n = int(rows.shape[0])
    out = torch.empty((n, N), dtype=torch.complex64, device=frames.device)
    _stream.launch(frames, lambda lib, stream: lib.amcx_gather_rows_c64(
        frames.data_ptr() if R else None, R, N, stride, rows.data_ptr() if n else None, n, out.data_ptr() if n else None, N, stream))
    return out


def occupied_features(frames_CKN, occ: Occupancy, feature_ids=None, recover=None, sample_rate=None):
    """The 18 features of the occupied cells alone: ``frames_CKN`` complex64 ``(C, K, N)`` (or the ``(C * K, N)`` matrix),
    contiguous -> float32 ``(C, K, 18)`` with NaN in every cell that is not occupied.  :func:`gather_rows`, then
    :func:`amcpy_amd.features.features18` on the packed rows -- the feature kernels are the ones every other path runs --,
    then a torch scatter.  ``recover`` (default None: the bits without the keyword): ``dict(order=M, search_hz=F,
    per="frame" | "emitter")`` -- the packed rows go through :func:`amcpy_amd.carrier.recover_frames` in front of the features;
    an emitter is a CHANNEL (row c of the mask), ``sample_rate`` the channels' own rate (for ``search_hz``)."""
    C, K = int(occ.mask.shape[0]), int(occ.mask.shape[1])
    flat = frames_CKN.reshape(C * K, frames_CKN.shape[-1]) if frames_CKN.dim() == 3 else frames_CKN
    if int(flat.shape[0]) != C * K:
        raise ValueError(f"frames of {C} x {K} cells expected, got {tuple(frames_CKN.shape)}")
    prepare = None
    if recover is not None:
        from . import carrier
        prepare = lambda packed, at: carrier.recover_frames(packed, recover, sample_rate, groups=at // K)[0]      # noqa: E731
    return _features_at(flat, occ.rows, feature_ids, prepare)[0].view(C, K, _lib.NUM_FEATURES)


def _features_at(flat, rows, feature_ids=None, prepare=None) -> tuple:
    """The gather -> features -> scatter step: ``flat`` complex64 ``(R, N)``, ``rows`` int32 ``(n,)`` -> ``(out, at, packed)``:
    ``out`` float32 ``(R, 18)`` with NaN in every row not listed, and -- None where no row is listed -- the int64 index ``at``
    and the ``packed`` ``(n, 18)`` features that were scattered by it (the survey scatters its labels by the same index).
    ``prepare(packed rows, at)``: what the gathered rows go through in front of the features."""
    import torch
    from .features import features18

    out = torch.full((int(flat.shape[0]), _lib.NUM_FEATURES), float("nan"), dtype=torch.float32, device=flat.device)
    if int(rows.shape[0]) == 0:
        return out, None, None
    at = rows.long()
    gathered = gather_rows(flat, rows)
    if prepare is not None:
        gathered = prepare(gathered, at)
    packed = features18(gathered, feature_ids=feature_ids).reshape(-1, _lib.NUM_FEATURES)
    out[at] = packed
    return out, at, packed


def segments(mask) -> list:
    """The runs of occupied frames per channel: ``mask`` (C, K) bool (numpy, or anything ``numpy.asarray`` takes) ->
    ``[(channel, first_frame, last_frame), ...]``, both ends inclusive, ordered by channel and then by time.  Host side."""
    m = np.asarray(mask).astype(bool)
    if m.ndim != 2:
        raise ValueError("mask must be (C, K)")
    out = []
    for c in range(m.shape[0]):
        edge = np.diff(np.concatenate(([0], m[c].astype(np.int8), [0])))
        first, past = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
        out.extend((c, int(a), int(b) - 1) for a, b in zip(first, past))
    return out
