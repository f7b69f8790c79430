"""SigMF recordings: ``X.sigmf-meta`` (JSON) beside ``X.sigmf-data`` (the samples).

Written from the field names of the SigMF specification with the stdlib ``json``; no dependency.  What is read:

    global   core:datatype        cf32_le, ci16_le, ci8, cu8 (every other datatype is a ValueError that names it)
             core:num_channels    1 (or absent)
             core:trailing_bytes  bytes at the end of the data file that are no samples
    captures core:sample_start    index of the segment's first sample, counted over the samples of the data file
             core:header_bytes    bytes in front of the segment's first sample that are no samples

With ``tune=`` (:func:`extract_sigmf`) also ``core:sample_rate``, a capture's ``core:frequency`` and an annotation's
``core:sample_start`` / ``core:freq_lower_edge`` / ``core:freq_upper_edge``: :func:`tune_from_annotation`.

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

from . import _formats

# core:datatype -> (sample_format of extract_raw_stream, stored sample, default scale)
DATATYPES = {f.sigmf: (f.name, f.store, f.scale) for f in _formats.TABLE}
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


def tune_from_annotation(meta: dict, k: int, oversample=2.0, rational: bool = False) -> tuple:
    """Where annotation ``k`` of the parsed meta file says its emitter is -> ``(shift_hz, decimate)`` for ``tune=``, or,
    ``rational=True``, ``(shift_hz, (L, D))`` with ``L / D = rational_ratio(oversample * bandwidth / fs, 255, 255)``
    (:func:`amcpy_amd.resample.rational_ratio`, exact arithmetic on the floats' values): the integer ``decimate`` delivers
    anything between ``oversample`` and twice that, the fraction what was asked for.  L and D stay within 255
    (``resample.DESIGN_MAX``): the largest for which :func:`amcpy_amd.resample.design_resample_lowpass`'s default,
    ``16 max(L, D) + 1`` taps, fits the kernel's 4096 -- so a filter exists for whatever comes back; the fraction is within
    ``1 / (2 * 255 * D)`` of the ratio wanted, 0.2 % of it at worst for ratios from 0.05 up (a host test sweeps them).
    ValueError for a ratio outside ``[1 / 255, 255]``: a band narrower than ``fs / (255 * oversample)`` wants a
    down-converter first.

    The annotation's band ``core:freq_lower_edge ... core:freq_upper_edge`` is set against the ``core:frequency`` of the
    capture that holds its ``core:sample_start`` (the last capture that starts at or before it) and the recording's
    ``core:sample_rate`` fs:  ``shift_hz = capture frequency - band centre`` (what moves the centre to 0 Hz) and
    ``decimate = max(1, floor(fs / (oversample * bandwidth)))``, 4096 at most.  Pure arithmetic on the JSON; ValueError
    names the field that is missing."""
    glob = meta.get("global") or {}
    anns = meta.get("annotations") or []
    if not 0 <= int(k) < len(anns):
        raise ValueError(f"annotation {k}: the recording has {len(anns)}")
    ann = anns[int(k)]
    for key in ("core:freq_lower_edge", "core:freq_upper_edge"):
        if key not in ann:
            raise ValueError(f"annotation {k} has no {key}")
    if "core:sample_rate" not in glob:
        raise ValueError("no global core:sample_rate")
    lo, hi, fs = float(ann["core:freq_lower_edge"]), float(ann["core:freq_upper_edge"]), float(glob["core:sample_rate"])
    r = float(oversample)
    if not (hi > lo and fs > 0.0 and r > 0.0):
        raise ValueError(f"annotation {k}: needs freq_upper_edge > freq_lower_edge, sample_rate > 0 and oversample > 0")
    at = int(ann.get("core:sample_start", 0))
    held = [c for c in (meta.get("captures") or []) if int(c.get("core:sample_start", 0)) <= at]
    if not held or "core:frequency" not in held[-1]:
        raise ValueError(f"annotation {k}: the capture that holds sample {at} has no core:frequency")
    shift_hz = float(held[-1]["core:frequency"]) - (lo + hi) / 2.0
    if rational:
        from fractions import Fraction
        from .resample import DESIGN_MAX, rational_ratio
        return shift_hz, rational_ratio(Fraction(r) * Fraction(hi - lo) / Fraction(fs), DESIGN_MAX, DESIGN_MAX)
    return shift_hz, int(min(4096, max(1, np.floor(fs / (r * (hi - lo))))))


def resolve_tune(meta: dict, tune: dict) -> tuple:
    """``tune`` of :func:`extract_sigmf` -> ``(shift in cycles per sample, decimate, float32 taps)``."""
    from fractions import Fraction
    from .ddc import design_lowpass
    known = {"shift_hz", "decimate", "taps", "annotation", "oversample"}
    if not isinstance(tune, dict) or set(tune) - known:
        raise ValueError(f"tune: a dict of {sorted(known)}")
    if "annotation" in tune:
        if "shift_hz" in tune or "decimate" in tune:
            raise ValueError("tune: either annotation (and oversample) or shift_hz and decimate")
        shift_hz, D = tune_from_annotation(meta, tune["annotation"], tune.get("oversample", 2.0))
    else:
        if "decimate" not in tune or "oversample" in tune:
            raise ValueError("tune: either annotation (and oversample) or shift_hz and decimate")
        shift_hz, D = float(tune.get("shift_hz", 0.0)), int(tune["decimate"])
    shift = Fraction(0)
    if shift_hz != 0.0:
        fs = (meta.get("global") or {}).get("core:sample_rate")
        if fs is None or float(fs) <= 0.0:
            raise ValueError("tune: a shift in Hz needs the global core:sample_rate")
        shift = Fraction(shift_hz) / Fraction(float(fs))
    taps = tune.get("taps")
    if taps is None or isinstance(taps, (int, np.integer)):
        taps = design_lowpass(D, taps)
    return shift, D, np.ascontiguousarray(np.asarray(taps, dtype=np.float32))


class ResolvedResample(tuple):
    """``(shift in cycles per sample, L, D, float32 taps)``: what :func:`resolve_resample` returns, and takes back unchanged
    as a ``tune`` of :func:`extract_sigmf` (a caller that needs L and D resolves once and passes the result on)."""
    __slots__ = ()


def resolve_resample(meta: dict, tune) -> ResolvedResample:
    """The rational forms of ``tune`` -- ``dict(annotation=k, oversample=r, rational=True, taps=None)`` or ``dict(shift_hz=F,
    resample=(L, D), taps=None)`` -- -> ``(shift in cycles per sample, L, D, float32 taps)``.  ``taps``: None for
    :func:`amcpy_amd.resample.design_resample_lowpass`'s default, a tap count, or the taps at the upsampled rate."""
    from fractions import Fraction
    from .resample import design_resample_lowpass, out_samples
    if isinstance(tune, ResolvedResample):
        return tune
    if "annotation" in tune:
        if set(tune) - {"annotation", "oversample", "rational", "taps"}:
            raise ValueError("tune: annotation, oversample, rational and taps, or shift_hz, resample and taps")
        shift_hz, (L, D) = tune_from_annotation(meta, tune["annotation"], tune.get("oversample", 2.0), rational=True)
    else:
        if set(tune) - {"shift_hz", "resample", "taps", "rational"} or "resample" not in tune:
            raise ValueError("tune: annotation, oversample, rational and taps, or shift_hz, resample and taps")
        shift_hz = float(tune.get("shift_hz", 0.0))
        L, D = (int(v) for v in tune["resample"])
    shift = Fraction(0)
    if shift_hz != 0.0:
        fs = (meta.get("global") or {}).get("core:sample_rate")
        if fs is None or float(fs) <= 0.0:
            raise ValueError("tune: a shift in Hz needs the global core:sample_rate")
        shift = Fraction(shift_hz) / Fraction(float(fs))
    taps = tune.get("taps")
    if taps is None or isinstance(taps, (int, np.integer)):
        taps = design_resample_lowpass(L, D, taps)
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float32))
    out_samples(0, taps.shape[0], L, D)                          # the limits
    return ResolvedResample((shift, L, D, taps))


def is_rational_tune(tune) -> bool:
    """Whether a ``tune`` asks for the rational resampler: a dict with ``resample=(L, D)`` or ``rational=True``, or what
    :func:`resolve_resample` made of one."""
    return isinstance(tune, ResolvedResample) or (isinstance(tune, dict) and ("resample" in tune or bool(tune.get("rational", False))))


def _walk(rec, make, device, on_gpu: bool, chunk_samples: int, axis: int = 0, enough=None):
    """The segment and chunk walk of every streaming path.  Each capture segment that has samples is memory-mapped and pushed
    in chunks of ``chunk_samples`` -- as torch tensors on the device (``on_gpu``), or as the numpy arrays they are -- through
    a streaming object that starts anew with the segment: ``make()``.  Yields ``(segment index, segment start, the outputs
    of the pushes, the streaming object)``.  ``enough(have)``, where given, is asked before a segment (have = 0: true ends the
    walk) and after every push (have: the outputs of this segment so far, counted along ``axis``; true ends the segment)."""
    fmt = _formats.get(rec["sample_format"])                # of one stored sample, for the chunks
    if on_gpu:
        import torch                                       # the streaming paths alone: the untuned one stays torch-free
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    for j, (start, off, n_samples) in enumerate(rec["segments"]):
        if enough is not None and enough(0):
            break
        if n_samples == 0:
            continue
        # (mode "c": private pages, never written -- torch.from_numpy wants a writable array, and "r+" would want a writable file)
        src = np.memmap(rec["data_path"], dtype=fmt.plain, mode="c", offset=off, shape=(n_samples,) + fmt.tail)
        obj = make()
        ys, have = [], 0
        for c0 in range(0, n_samples, chunk_samples):
            chunk = np.ascontiguousarray(src[c0:c0 + chunk_samples])
            ys.append(obj.push(torch.from_numpy(chunk).to(dev) if on_gpu else chunk))
            have += int(ys[-1].shape[axis])
            if enough is not None and enough(have):
                break
        yield j, start, ys, obj


def _extract_tuned(rec, N, tune, device, feature_ids, scale, left, compute, tune_compute, chunk_samples, recover=None):
    """The tuned path of :func:`extract_sigmf`: every segment through a :class:`amcpy_amd.ddc.Channelizer` -- or, a
    rational ``tune``, a :class:`amcpy_amd.resample.Resampler` -- in chunks.  ``recover``: the frames go through
    :func:`amcpy_amd.carrier.recover_frames` in front of the features, and a third value comes back: the carrier found per frame."""
    from .ddc import Channelizer
    fmt = rec["sample_format"]
    if is_rational_tune(tune):
        from .resample import Resampler
        shift, L, D, taps = resolve_resample(rec["meta"], tune)
        make = lambda: Resampler(taps, L, D, shift, fmt, scale, compute=tune_compute)      # noqa: E731
    else:
        if isinstance(tune, dict) and tune.get("rational", True) is False:
            tune = {k: v for k, v in tune.items() if k != "rational"}
        shift, D, taps = resolve_tune(rec["meta"], tune)
        L = 1
        make = lambda: Channelizer(taps, D, shift, fmt, scale, compute=tune_compute)       # noqa: E731
    on_gpu = tune_compute is None
    if on_gpu:
        import torch
        from .features import features18
    if recover is not None:
        if not on_gpu:
            raise ValueError("recover runs on the device: not beside an injected tune_compute")
        from . import carrier
        rate = rec["meta"].get("global", {}).get("core:sample_rate")
        rate = float(rate) * L / D if rate else None                       # the frames' own rate
        found = {"cycles": [], "phase": [], "quality": []}
    parts, starts = [], []
    for _, start, ys, _ in _walk(rec, make, device, on_gpu, chunk_samples,
                                 enough=lambda have: left is not None and have >= left * N):
        have = sum(int(y.shape[0]) for y in ys)
        n = have // N if left is None else min(have // N, left)
        if n == 0:
            continue
        if left is not None:
            left -= n
        if on_gpu:
            frames = torch.cat(ys)[:n * N].view(n, N)
            if recover is not None:
                frames, est = carrier.recover_frames(frames, recover, rate)
                for key in found:
                    found[key].append(getattr(est, key).cpu().numpy())
            if compute is None:
                parts.append(features18(frames, feature_ids=feature_ids).cpu().numpy())
            else:
                parts.append(np.asarray(compute(frames.cpu().numpy()), dtype=np.float32))
        else:
            parts.append(np.asarray(compute(np.concatenate(ys)[:n * N].reshape(n, N)), dtype=np.float32))
        starts.append(start + N * D * np.arange(n, dtype=np.int64) // L)
    if recover is not None:
        cat = {k: np.concatenate(v) if v else np.empty((0,), np.float64) for k, v in found.items()}
        carrier_of = {"carrier_hz": cat["cycles"] * (rate or 1.0), "carrier_phase": cat["phase"], "carrier_quality": cat["quality"]}
        if not parts:
            return np.empty((0, 18), dtype=np.float32), np.empty((0,), dtype=np.int64), carrier_of
        return np.concatenate(parts), np.concatenate(starts), carrier_of
    if not parts:
        return np.empty((0, 18), dtype=np.float32), np.empty((0,), dtype=np.int64)
    return np.concatenate(parts), np.concatenate(starts)


def resolve_channelize(meta: dict, channelize: dict) -> tuple:
    """``channelize`` of :func:`extract_sigmf` -> ``(shift in cycles per sample, channels, decim, float32 taps)``."""
    from fractions import Fraction
    from .bank import design_bank_lowpass
    known = {"channels", "oversample", "taps_per_channel", "taps", "shift_hz"}
    if not isinstance(channelize, dict) or set(channelize) - known or "channels" not in channelize:
        raise ValueError(f"channelize: a dict of {sorted(known)}, channels among them")
    C, over = int(channelize["channels"]), channelize.get("oversample", 1)
    if over not in (1, 2):
        raise ValueError(f"channelize: oversample is 1 (critically sampled) or 2, not {over!r}")
    shift_hz = float(channelize.get("shift_hz", 0.0))
    shift = Fraction(0)
    if shift_hz != 0.0:
        rate = meta.get("global", {}).get("core:sample_rate")
        if not rate:
            raise ValueError("channelize: a shift in Hz needs the global core:sample_rate")
        shift = Fraction(shift_hz) / Fraction(float(rate))
    taps = channelize.get("taps")
    if taps is None:
        taps = design_bank_lowpass(C, int(channelize.get("taps_per_channel", 16)))
    elif "taps_per_channel" in channelize:
        raise ValueError("channelize: either taps or taps_per_channel")
    return shift, C, C // int(over), np.ascontiguousarray(np.asarray(taps, dtype=np.float32))


def _walk_channelized(rec, N, channelize, device, scale, left, bank_compute, chunk_samples):
    """The segment and chunk walk of the filter-bank paths (:func:`extract_sigmf` with ``channelize``, :func:`survey_sigmf`):
    every segment through a :class:`amcpy_amd.bank.FilterBank` in chunks, its channels cut into frames.  Yields
    ``(segment start, n, frames)`` per segment that has frames: ``frames`` is the contiguous complex64 ``(C * n, N)`` matrix, row
    ``c * n + k`` channel c's frame k -- a torch tensor on the device, or, with an injected ``bank_compute``, a numpy array."""
    from .bank import FilterBank
    shift, C, D, taps = resolve_channelize(rec["meta"], channelize)
    fmt = rec["sample_format"]
    on_gpu = bank_compute is None
    if on_gpu:
        import torch
    for _, start, ys, _ in _walk(rec, lambda: FilterBank(taps, C, D, shift, fmt, scale, compute=bank_compute), device, on_gpu,
                                 chunk_samples, axis=1, enough=lambda have: left is not None and have >= left * N):
        have = sum(int(y.shape[1]) for y in ys)
        n = have // N if left is None else min(have // N, left)
        if n == 0:
            continue
        if left is not None:
            left -= n
        if on_gpu:
            frames = torch.cat(ys, dim=1)[:, :n * N].contiguous().view(C * n, N)          # row c * n + k: channel c, frame k
        else:
            frames = np.ascontiguousarray(np.concatenate(ys, axis=1)[:, :n * N]).reshape(C * n, N)
        yield start, n, frames


def _extract_channelized(rec, N, channelize, device, feature_ids, scale, left, compute, bank_compute, chunk_samples):
    """The filter-bank path of :func:`extract_sigmf`: the 18 features of every cell :func:`_walk_channelized` yields."""
    _, C, D, _ = resolve_channelize(rec["meta"], channelize)
    parts, starts = [], []
    for start, n, frames in _walk_channelized(rec, N, channelize, device, scale, left, bank_compute, chunk_samples):
        if bank_compute is None:
            if compute is None:
                from .features import features18
                got = features18(frames, feature_ids=feature_ids).cpu().numpy()
            else:
                got = np.asarray(compute(frames.cpu().numpy()), dtype=np.float32)
        else:
            got = np.asarray(compute(frames), dtype=np.float32)
        parts.append(got.reshape(C, n, 18))
        starts.append(start + N * D * np.arange(n, dtype=np.int64))
    if not parts:
        return np.empty((C, 0, 18), dtype=np.float32), np.empty((0,), dtype=np.int64)
    return np.concatenate(parts, axis=1), np.concatenate(starts)


def _survey_segment_gpu(frames, C, n, rank_q, thr_db, detect, model, cols, mean, scale_, feature_ids):
    """One segment of :func:`survey_sigmf` on the device -> (features, power, floor, mask, snr_db, labels) as numpy."""
    import torch
    from . import occupancy
    from .features import features18
    power = occupancy.row_power(frames).view(C, n)
    occ = occupancy.detect(power, floor_quantile=rank_q, threshold_db=thr_db)
    labels = None
    if detect is None:
        feats = features18(frames, feature_ids=feature_ids).reshape(C * n, 18)
        if model is not None:
            from .classifier import classify
            labels = classify(feats, model, cols=cols, mean=mean, scale=scale_).reshape(C, n)
    else:
        feats, at, packed = occupancy._features_at(frames, occ.rows, feature_ids)
        if model is not None:
            labels = torch.full((C * n,), -2, dtype=torch.int32, device=frames.device)
            if at is not None:
                from .classifier import classify
                labels[at] = classify(packed, model, cols=cols, mean=mean, scale=scale_).reshape(-1)
            labels = labels.view(C, n)
    host = lambda t: None if t is None else t.cpu().numpy()      # noqa: E731
    return (host(feats.view(C, n, 18)), host(power), host(occ.floor), host(occ.mask), host(occ.snr_db), host(labels))


def _survey_segment_injected(frames, C, n, rank, thr, detect, model, compute, occupancy_compute):
    """The same over numpy with injected computes (tests)."""
    from .occupancy import snr_db
    power, floor, mask = occupancy_compute(frames, C, n, rank, thr)
    power, floor, mask = np.asarray(power, np.float32).reshape(C, n), np.asarray(floor, np.float32), np.asarray(mask, bool).reshape(C, n)
    rows = np.flatnonzero(mask.reshape(-1)) if detect is not None else np.arange(C * n)
    feats = np.full((C * n, 18), np.nan, dtype=np.float32)
    labels = None if model is None else np.full((C * n,), -2, dtype=np.int32)
    if rows.size:
        got = np.asarray(compute(np.ascontiguousarray(frames[rows])), dtype=np.float32).reshape(-1, 18)
        feats[rows] = got
        if model is not None:
            labels[rows] = np.asarray(model(got), dtype=np.int32).reshape(-1)
    return feats.reshape(C, n, 18), power, floor, mask, snr_db(power, floor, 1), None if labels is None else labels.reshape(C, n)


def survey_sigmf(path, frame_size: int, *, channelize, detect=None, model=None, cols=None, mean=None, scale=None,
                 device: Optional[int] = None, feature_ids=None, scale_samples=None, chunk_samples: int = 1 << 24,
                 bank_compute=None, occupancy_compute=None, compute=None) -> dict:
    """Which channels of a wideband SigMF recording hold an emitter, when, how strong, and -- with ``model`` -- which
    modulation.  The recording goes through the filter bank exactly as ``extract_sigmf(channelize=...)`` takes it (the same
    segment and chunk walk, ``channelize`` as there); every cell's power and every frame's floor are computed on the device
    (:mod:`amcpy_amd.occupancy`), and, with ``detect``, only the occupied cells go through the feature kernels and the
    classifier.  Returns a dict:

        features (C, K, 18) float32     NaN in cells that are not occupied (without ``detect``: every cell's features)
        frame_start (K,) int64          as :func:`extract_sigmf`
        power (C, K), floor (K,)        float32
      with ``detect = dict(threshold_db=6.0, floor_quantile=0.25)`` (either key may be left out):
        occupied (C, K) bool, snr_db (C, K) float32, segments [(channel, first_frame, last_frame), ...]
      with ``model`` (an :class:`amcpy_amd.classifier.MlpModel`; ``cols``, ``mean``, ``scale`` as :func:`amcpy_amd.classifier.classify`):
        labels (C, K) int32             the classifier's label, -1 for a row without finite probabilities, -2 for a cell that
                                        is not occupied

    ``scale_samples``: what an integer component is multiplied by (``extract_sigmf``'s ``scale``; the name ``scale`` is the
    classifier's here).  What the detector assumes: :mod:`amcpy_amd.occupancy`.  Injected computes (tests, all numpy):
    ``bank_compute`` as :class:`amcpy_amd.bank.FilterBank`'s; ``occupancy_compute(frames (C n, N), C, n, floor_rank,
    threshold) -> (power, floor, mask)``; ``compute(rows) -> (rows, 18)``; ``model`` is then a callable ``(rows, 18) -> labels``.
    The three go together."""
    from . import occupancy
    from .feature_extraction import _subset
    injected = [bank_compute is not None, occupancy_compute is not None, compute is not None]
    if any(injected) and not all(injected):
        raise ValueError("bank_compute, occupancy_compute and compute are injected together")
    feature_ids, compute = _subset(feature_ids, compute)
    N = int(frame_size)
    if N < 2:
        raise ValueError("frame_size must be >= 2")
    if detect is not None and (not isinstance(detect, dict) or set(detect) - {"threshold_db", "floor_quantile"}):
        raise ValueError("detect: a dict of threshold_db and floor_quantile")
    if model is not None and cols is None and not any(injected):
        raise ValueError("model needs cols (and mean and scale, unless the model takes raw features)")
    thr_db = float((detect or {}).get("threshold_db", 6.0))
    quantile = float((detect or {}).get("floor_quantile", 0.25))
    rec = read_meta(path)
    _, C, D, _ = resolve_channelize(rec["meta"], channelize)
    rank, thr = occupancy.floor_rank_of(C, quantile), occupancy.threshold_of(thr_db)
    sample_scale = _formats.scale_of(rec["sample_format"], scale_samples)
    parts, starts = [], []
    for start, n, frames in _walk_channelized(rec, N, channelize, device, sample_scale, None, bank_compute,
                                              max(1, int(chunk_samples))):
        if any(injected):
            parts.append(_survey_segment_injected(frames, C, n, rank, thr, detect, model, compute, occupancy_compute))
        else:
            parts.append(_survey_segment_gpu(frames, C, n, quantile, thr_db, detect, model, cols, mean, scale, feature_ids))
        starts.append(start + N * D * np.arange(n, dtype=np.int64))
    if parts:
        feats, power, floor, mask, snr_db, labels = zip(*parts)           # frames are axis 1 of everything but the floor
        feats, power, mask, snr_db = (np.concatenate(v, axis=1) for v in (feats, power, mask, snr_db))
        labels = None if model is None else np.concatenate(labels, axis=1)
        floor, frame_start = np.concatenate(floor), np.concatenate(starts)
    else:
        feats, power, floor = np.empty((C, 0, 18), np.float32), np.empty((C, 0), np.float32), np.empty((0,), np.float32)
        mask, snr_db = np.zeros((C, 0), bool), np.empty((C, 0), np.float32)
        labels = None if model is None else np.empty((C, 0), np.int32)
        frame_start = np.empty((0,), np.int64)
    out = {"features": feats, "frame_start": frame_start, "power": power, "floor": floor}
    if detect is not None:
        out.update(occupied=mask, snr_db=snr_db, segments=occupancy.segments(mask))
    if model is not None:
        out["labels"] = labels
    return out


_SCAN_DETECT = {"threshold_db": 6.0, "floor_quantile": 0.25, "min_bins": 2, "merge_bins": 2, "min_rows": 1}


def scan_sigmf(path, *, nfft: int = 1024, hop=None, averages: int = 16, window="hann", detect=None,
               device: Optional[int] = None, scale_samples=None, chunk_samples: int = 1 << 24, psd_compute=None,
               detect_compute=None) -> dict:
    """Where the emitters of a SigMF recording of an unknown band are, with no channel raster: the Welch spectrogram of the
    raw stream on the device (:mod:`amcpy_amd.psd`), a noise floor and a mask per row, and the occupied bins joined into
    emitters -- time span and frequency edges, the input of ``tune_from_annotation``.  Returns a dict:

        psd (R, nfft) float32           sums of ``averages`` windowed periodograms in FFT order, not normalised
                                        (:func:`amcpy_amd.psd.power_scale`)
        row_start (R,) int64            the sample index (``core:sample_start`` counting) of each row's first sample
        row_samples                     ``(A - 1) hop + nfft``: the samples a row covers
        freq_hz (nfft,) float64         only where the meta gives ``core:sample_rate``: the bins' frequencies, offset by the
                                        first capture's ``core:frequency`` where it has one
      with ``detect = dict(threshold_db=6.0, floor_quantile=0.25, min_bins=2, merge_bins=2, min_rows=1)`` (any key may be left out):
        floor (R,) float32, occupied (R, nfft) bool, snr_db (R, nfft) float32
        emitters                        a list of dicts: ``sample_start``, ``sample_count``, ``freq_lower_edge``,
                                        ``freq_upper_edge`` (the outer edges of the emitter's first and last bin: bin centre
                                        -/+ half a bin, in Hz and offset by the ``core:frequency`` of the capture that holds
                                        the emitter; in cycles per sample where the meta gives no sample rate), ``snr_db``
                                        (the mean over the emitter's occupied cells), and ``rows`` / ``bins``, its
                                        ``(first, last)`` rows of ``psd`` and signed bins (:func:`amcpy_amd.psd.emitters`)

    Segments are walked as ``extract_sigmf(tune=...)`` walks them: every capture is read in chunks of ``chunk_samples``, copied
    to the device as it lies and pushed through a :class:`amcpy_amd.psd.Spectrogram` that starts anew with the capture -- no
    row straddles a capture, and no emitter does.  What the detector assumes: :mod:`amcpy_amd.psd`.  ``scale_samples``: what an
    integer component is multiplied by.  Injected computes (tests, numpy; the two go together): ``psd_compute`` as
    :class:`amcpy_amd.psd.Spectrogram`'s ``compute``; ``detect_compute(P (R, nfft), floor_rank, threshold) -> (floor, mask)``."""
    return scan_recording(read_meta(path), nfft=nfft, hop=hop, averages=averages, window=window, detect=detect, device=device,
                          scale_samples=scale_samples, chunk_samples=chunk_samples, psd_compute=psd_compute,
                          detect_compute=detect_compute)


def raw_recording(path, sample_format: str) -> dict:
    """What :func:`read_meta` returns, for a raw stream of ``sample_format`` samples: one capture from sample 0, an empty meta."""
    fmt = _formats.get(sample_format)
    data_path = Path(path)
    return {"meta": {"global": {}, "captures": [{}], "annotations": []}, "data_path": data_path, "datatype": fmt.sigmf,
            "sample_format": fmt.name, "store": fmt.store, "scale": fmt.scale,
            "segments": [(0, 0, data_path.stat().st_size // fmt.store.itemsize)]}


def _scan_detect(P, opt, rank: int, thr, detect_compute) -> tuple:
    """The detection of one capture's rows ``P`` -- on the device, or injected over numpy -> ``(floor, mask, snr_db)`` as numpy."""
    from . import occupancy, psd
    if detect_compute is None:
        det = psd.detect(P, floor_quantile=float(opt["floor_quantile"]), threshold_db=float(opt["threshold_db"]))
        return det.floor.cpu().numpy(), det.mask.cpu().numpy(), det.snr_db.cpu().numpy()
    floor, mask = detect_compute(P, rank, thr)
    floor, mask = np.asarray(floor, dtype=np.float32), np.asarray(mask).astype(bool)
    return floor, mask, occupancy.snr_db(np.asarray(P, np.float32), floor, 0)


def _scan_emitters(mask, snr, row_start, span: int, first_row: int, fs: float, fc: float, opt) -> list:
    """The emitters of one capture as :func:`scan_sigmf`'s dicts: ``row_start`` the first sample of each of its rows, ``span``
    the samples a row covers, ``first_row`` its first row in the whole recording's ``psd``; ``fs`` and ``fc`` scale and offset the
    bin edges."""
    from . import psd
    nfft = int(mask.shape[1])
    found = []
    for r0, r1, lo, hi in psd.emitters(mask, int(opt["min_bins"]), int(opt["merge_bins"]), int(opt["min_rows"])):
        cols = np.arange(lo, hi + 1) % nfft
        cells = mask[r0:r1 + 1][:, cols]
        found.append({"sample_start": int(row_start[r0]), "sample_count": int(row_start[r1] - row_start[r0]) + span,
                      "freq_lower_edge": fc + fs * (lo - 0.5) / nfft, "freq_upper_edge": fc + fs * (hi + 0.5) / nfft,
                      "snr_db": float(np.mean(snr[r0:r1 + 1][:, cols][cells])),
                      "rows": (first_row + r0, first_row + r1), "bins": (lo, hi)})
    return found


def _scan_result(nfft: int, span: int, parts, starts, freq_hz, detected, found) -> dict:
    """:func:`scan_sigmf`'s dict from the captures' pieces: ``detected`` is None, or the captures' ``(floor, mask, snr_db)``."""
    out = {"psd": np.concatenate(parts) if parts else np.empty((0, nfft), np.float32),
           "row_start": np.concatenate(starts) if starts else np.empty((0,), np.int64), "row_samples": span}
    if freq_hz is not None:
        out["freq_hz"] = freq_hz
    if detected is not None:
        none = (np.empty((0,), np.float32), np.zeros((0, nfft), bool), np.empty((0, nfft), np.float32))
        for k, key in enumerate(("floor", "occupied", "snr_db")):
            out[key] = np.concatenate([d[k] for d in detected]) if detected else none[k]
        out["emitters"] = found
    return out


def scan_recording(rec: dict, *, nfft: int = 1024, hop=None, averages: int = 16, window="hann", detect=None,
                   device: Optional[int] = None, scale_samples=None, chunk_samples: int = 1 << 24, psd_compute=None,
                   detect_compute=None) -> dict:
    """:func:`scan_sigmf` on what :func:`read_meta` (or :func:`raw_recording`) returned."""
    from . import occupancy, psd
    if (psd_compute is None) != (detect_compute is None):
        raise ValueError("psd_compute and detect_compute are injected together")
    if detect is not None and (not isinstance(detect, dict) or set(detect) - set(_SCAN_DETECT)):
        raise ValueError(f"detect: a dict of {sorted(_SCAN_DETECT)}")
    opt = {**_SCAN_DETECT, **(detect or {})}
    nfft = int(nfft)
    hop = nfft // 2 if hop is None else int(hop)
    A = int(averages)
    fmt = rec["sample_format"]
    scale = _formats.scale_of(fmt, scale_samples)
    win = psd._window_of(window, nfft)
    span, step = psd.row_samples(nfft, hop, A), A * hop
    rank, thr = occupancy.floor_rank_of(nfft, float(opt["floor_quantile"])), occupancy.threshold_of(float(opt["threshold_db"]))
    on_gpu = psd_compute is None
    if on_gpu:
        import torch
    rate = (rec["meta"].get("global") or {}).get("core:sample_rate")
    captures = rec["meta"].get("captures") or [{}]
    parts, starts, detected, found = [], [], [], []
    n_rows = 0
    for j, start, rows, sp in _walk(rec, lambda: psd.Spectrogram(nfft, hop, A, win, fmt, scale, compute=psd_compute), device, on_gpu,
                                    max(1, int(chunk_samples))):
        R = sp.rows_done
        if R == 0:
            continue
        P = torch.cat(rows) if on_gpu else np.concatenate(rows)
        row_start = start + step * np.arange(R, dtype=np.int64)
        if detect is not None:
            detected.append(_scan_detect(P, opt, rank, thr, detect_compute))
            fc = float(captures[j].get("core:frequency", 0.0)) if rate and j < len(captures) else 0.0
            found += _scan_emitters(detected[-1][1], detected[-1][2], row_start, span, n_rows, float(rate) if rate else 1.0, fc, opt)
        parts.append(P.cpu().numpy() if on_gpu else np.asarray(P, dtype=np.float32))
        starts.append(row_start)
        n_rows += R
    freq_hz = psd.bin_frequencies(nfft, float(rate), float(captures[0].get("core:frequency", 0.0))) if rate else None
    return _scan_result(nfft, span, parts, starts, freq_hz, None if detect is None else detected, found)


def extract_sigmf(path, frame_size: int, *, device: Optional[int] = None, feature_ids=None, scale=None,
                  max_frames: Optional[int] = None, compute=None, tune=None, tune_compute=None,
                  chunk_samples: int = 1 << 24, channelize=None, bank_compute=None):
    """Features of a SigMF recording -> ``(features, frame_start)``: (F, 18) float32 and (F,) int64.

    Every capture segment is cut into consecutive ``frame_size``-sample frames (its partial tail is dropped: no frame
    straddles a capture boundary) and goes through the engine as ONE call over the data file itself, so the staging
    threads read it and the samples cross the link as they lie (8, 4 or 2 bytes each).  ``frame_start[k]`` is the
    sample index (``core:sample_start`` counting) of frame k's first sample.  ``scale``: what an integer component is
    multiplied by (default 2^-15 for ci16_le, 2^-7 for ci8 / cu8; cf32_le has none).  ``feature_ids``: only these (NaN in
    the other columns).  ``compute``: an injected engine (tests), which sees the widened complex64 frames.

    ``tune``: the emitter is off centre and narrower than the recorded band -- ``dict(shift_hz=F, decimate=D, taps=None)``
    (add F Hz to every frequency -- an emitter at +f wants F = -f --, low-pass, keep every D-th sample; ``taps``: None
    for :func:`amcpy_amd.ddc.design_lowpass`'s default, a tap count, or the taps), or ``dict(annotation=k, oversample=r)``
    (:func:`tune_from_annotation`).  Every segment is then read in chunks of ``chunk_samples``, copied to the device as it
    lies and pushed through a :class:`amcpy_amd.ddc.Channelizer` (the phase starts at 0 with every segment); the
    decimated stream is cut into ``frame_size`` frames (its partial tail dropped, nothing straddles a capture) and the
    features are computed on the resident result.  ``frame_start[k]`` is ``segment start + k * frame_size * D``, the first
    input sample that contributes to frame k.  ``tune_compute``: an injected down-converter over numpy chunks (tests, as
    :class:`amcpy_amd.ddc.Channelizer`'s ``compute``); ``compute`` then sees the decimated complex64 frames.
    The RATIONAL forms, ``dict(annotation=k, oversample=r, rational=True)`` (L and D within 255, so that the default taps
    exist: :func:`tune_from_annotation`; it takes ``taps`` too) and ``dict(shift_hz=F, resample=(L, D),
    taps=None)`` (``taps``: None for :func:`amcpy_amd.resample.design_resample_lowpass`'s default, a tap count, or the taps at
    the upsampled rate), go through a :class:`amcpy_amd.resample.Resampler` instead -- L outputs for every D inputs, so the
    emitter comes out at the oversampling asked for, not at the next integer's: ``frame_start[k] = segment start +
    floor(k * frame_size * D / L)``; ``tune_compute`` is then that class's ``compute``.

    ``recover``, A KEY OF THE ``tune`` DICT in any of its forms (absent or None: every result is the bits it is without the key) --
    ``tune=dict(..., recover=dict(order=M, search_hz=F, per="frame" | "emitter"))``: tuning centres an emitter to within a scan bin, and the residual
    offset, the carrier's phase and the receiver's level move the features; every frame goes through
    :func:`amcpy_amd.carrier.recover_frames` (blind M-th-power carrier recovery: gain, frequency and phase taken out; the frame
    size must be a power of two of 64 ... 4096) in front of the features.  ``search_hz``: the largest residual looked for, in Hz
    at the frames' rate (needs ``core:sample_rate``; default: frame_size / 16 bins of x^M).  ``per="emitter"``: one frequency, the
    median, for all frames of a chunk.  A THIRD value is then returned: ``dict(carrier_hz, carrier_phase, carrier_quality)``,
    one float per frame (Hz at the frames' rate -- cycles per sample where the recording names no rate --, cycles, and the
    line's share of the M-th power's energy).

    ``channelize`` (not together with ``tune``): the recording holds emitters on a raster --
    ``dict(channels=C, oversample=1|2, taps_per_channel=16, taps=None, shift_hz=0.0)``.  Every segment is read in chunks and
    pushed through a :class:`amcpy_amd.bank.FilterBank` of C channels, D = C / oversample (the sample index starts at 0 with
    every segment); every channel's stream is cut into frames.  Returns ``(features (C, K, 18), frame_start (K,))`` with
    ``frame_start[k] = segment start + k * frame_size * D``; ``max_frames`` counts frames per channel.  ``bank_compute``: an
    injected bank over numpy chunks (tests, as :class:`amcpy_amd.bank.FilterBank`'s ``compute``); ``compute`` then sees
    the (C * n, frame_size) complex64 frames of a segment, channel-major."""
    from .feature_extraction import FileComplex, FrameRows, HipEngine, _subset, widen_integer_frames
    feature_ids, compute = _subset(feature_ids, compute)
    N = int(frame_size)
    if N < 2:
        raise ValueError("frame_size must be >= 2")
    rec = read_meta(path)
    store, fmt = rec["store"], rec["sample_format"]
    scale = _formats.scale_of(fmt, scale)
    left = None if max_frames is None else max(0, int(max_frames))
    if tune is not None and channelize is not None:
        raise ValueError("tune and channelize exclude each other: one emitter, or every channel of a raster")
    if channelize is not None:
        return _extract_channelized(rec, N, channelize, device, feature_ids, scale, left, compute, bank_compute,
                                    max(1, int(chunk_samples)))
    recover = None
    if isinstance(tune, dict) and "recover" in tune:                  # carried by the tune dict; the resolvers never see it
        recover = tune["recover"]
        tune = {k: v for k, v in tune.items() if k != "recover"}
    if tune is not None:
        return _extract_tuned(rec, N, tune, device, feature_ids, scale, left, compute, tune_compute, max(1, int(chunk_samples)),
                              recover)
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
                    engine = HipEngine(N, device, feature_ids=feature_ids, **_formats.scale_kw(fmt, scale))
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
