"""SigMF recordings: ``X.sigmf-meta`` (JSON) beside ``X.sigmf-data`` (the samples).

Written from the field names of the SigMF specification with the stdlib ``json``; no dependency.  What is read:

    global   core:datatype        cf32_le, ci16_le, ci8, cu8 (every other datatype is a ValueError that names it)
             core:num_channels    1 (or absent)
             core:trailing_bytes  bytes at the end of the data file that are no samples
    captures core:sample_start    index of the segment's first sample, counted over the samples of the data file
             core:header_bytes    bytes in front of the segment's first sample that are no samples

A capture segment runs to the next one's ``core:sample_start`` (the last: to the end of the file).  Frames never straddle a
segment boundary: each segment is cut into consecutive frames and its partial tail is dropped, since whatever made the tool
begin a new capture -- a retune, a gap, a header -- lies between the two.  Archives (``.sigmf`` tar files), several channels,
real-valued, big-endian and the wider datatypes are out of scope.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Optional

import numpy as np

from . import _lib
from .features import CI8, CU8, SC16

# core:datatype -> (sample_format of extract_raw_stream, stored sample, default scale)
DATATYPES = {
    "cf32_le": ("cf32", np.dtype(np.complex64), 1.0),
    "ci16_le": ("sc16", SC16, _lib.SC16_SCALE),
    "ci8": ("ci8", CI8, _lib.IQ8_SCALE),
    "cu8": ("cu8", CU8, _lib.IQ8_SCALE),
}
META_SUFFIX, DATA_SUFFIX = ".sigmf-meta", ".sigmf-data"


def is_sigmf(path) -> bool:
    """True for ``X.sigmf-meta`` / ``X.sigmf-data``, or a stem both of which exist for."""
    p = str(path)
    return p.endswith((META_SUFFIX, DATA_SUFFIX)) or (Path(p + META_SUFFIX).exists() and Path(p + DATA_SUFFIX).exists())


def _stem(path) -> str:
    p = str(path)
    for suffix in (META_SUFFIX, DATA_SUFFIX):
        if p.endswith(suffix):
            return p[:-len(suffix)]
    return p


def read_meta(path) -> dict:
    """The recording ``path`` names (``X.sigmf-meta``, ``X.sigmf-data`` or the stem ``X``) ->

        {"meta": the parsed JSON, "data_path": Path, "datatype": str, "sample_format": "cf32" | "sc16" | "ci8" | "cu8",
         "store": numpy dtype of one sample, "scale": the default scale,
         "segments": [(sample_start, byte_offset, n_samples), ...]}

    ValueError for a meta file without ``core:datatype``, a datatype that is not read (named in the message), more than
    one channel, or captures that are not in ascending ``core:sample_start`` order."""
    stem = _stem(path)
    meta_path, data_path = Path(stem + META_SUFFIX), Path(stem + DATA_SUFFIX)
    with open(meta_path, "r", encoding="utf-8") as fh:
        meta = json.load(fh)
    glob = meta.get("global") if isinstance(meta, dict) else None
    if not isinstance(glob, dict) or "core:datatype" not in glob:
        raise ValueError(f"{meta_path}: no global core:datatype")
    datatype = str(glob["core:datatype"])
    if datatype not in DATATYPES:
        raise ValueError(f"{meta_path}: core:datatype {datatype!r} is not read (supported: {', '.join(DATATYPES)})")
    if int(glob.get("core:num_channels", 1)) != 1:
        raise ValueError(f"{meta_path}: core:num_channels {glob['core:num_channels']} is not read (one channel only)")
    sample_format, store, scale = DATATYPES[datatype]
    item = store.itemsize
    data_bytes = data_path.stat().st_size - int(glob.get("core:trailing_bytes", 0))
    captures = meta.get("captures") or [{}]
    starts, offsets, headers = [], [], 0
    for cap in captures:
        start = int(cap.get("core:sample_start", 0))
        if start < 0 or (starts and start < starts[-1]):
            raise ValueError(f"{meta_path}: captures must be in ascending core:sample_start order")
        headers += int(cap.get("core:header_bytes", 0))
        starts.append(start)
        offsets.append(headers + start * item)
    segments = []
    for j, (start, off) in enumerate(zip(starts, offsets)):
        n = starts[j + 1] - start if j + 1 < len(starts) else (data_bytes - off) // item
        segments.append((start, off, max(0, int(n))))
    return {"meta": meta, "data_path": data_path, "datatype": datatype, "sample_format": sample_format, "store": store,
            "scale": scale, "segments": segments}


def extract_sigmf(path, frame_size: int, *, device: Optional[int] = None, feature_ids=None, scale=None,
                  max_frames: Optional[int] = None, compute=None):
    """Features of a SigMF recording -> ``(features, frame_start)``: (F, 18) float32 and (F,) int64.

    Every capture segment is cut into consecutive ``frame_size``-sample frames (its partial tail is dropped: no frame
    straddles a capture boundary) and goes through the engine as ONE call over the data file itself, so the staging
    threads read it and the samples cross the link as they lie (8, 4 or 2 bytes each).  ``frame_start[k]`` is the
    sample index (``core:sample_start`` counting) of frame k's first sample.  ``scale``: what an integer component is
    multiplied by (default 2^-15 for ci16_le, 2^-7 for ci8 / cu8; cf32_le has none).  ``feature_ids``: only these (NaN in
    the other columns).  ``compute``: an injected engine (tests), which sees the widened complex64 frames."""
    from .feature_extraction import FileComplex, FrameRows, HipEngine, _subset, widen_integer_frames
    from .features import _sc16_scale
    feature_ids, compute = _subset(feature_ids, compute)
    N = int(frame_size)
    if N < 2:
        raise ValueError("frame_size must be >= 2")
    rec = read_meta(path)
    store, fmt = rec["store"], rec["sample_format"]
    scale = rec["scale"] if scale is None or fmt == "cf32" else _sc16_scale(scale)
    left = None if max_frames is None else max(0, int(max_frames))
    parts, starts = [], []
    engine = None
    try:
        for start, off, n_samples in rec["segments"]:
            n = n_samples // N if left is None else min(n_samples // N, left)
            if n == 0:
                continue
            if left is not None:
                left -= n
            if compute is None:
                if engine is None:
                    engine = HipEngine(N, device, feature_ids=feature_ids, sc16_scale=scale if fmt == "sc16" else _lib.SC16_SCALE,
                                       iq8_scale=scale if fmt in ("ci8", "cu8") else _lib.IQ8_SCALE)
                stream = FileComplex(rec["data_path"], store, (1, n, N), off, interleaved=True)
                try:
                    parts.append(np.asarray(engine(FrameRows(stream, 1, n)), dtype=np.float32))
                finally:
                    stream.release()
            else:
                frames = np.memmap(rec["data_path"], dtype=store, mode="r", offset=off, shape=(n, N))
                parts.append(np.asarray(compute(frames if fmt == "cf32" else widen_integer_frames(frames, scale)),
                                        dtype=np.float32))
            starts.append(start + N * np.arange(n, dtype=np.int64))
    finally:
        if engine is not None:
            engine.close()
    if not parts:
        return np.empty((0, 18), dtype=np.float32), np.empty((0,), dtype=np.int64)
    return np.concatenate(parts), np.concatenate(starts)
