"""Batch feature extraction: the MI355X drop-in for the reference's
``run_extraction(cfg)`` (src/amcpy/feature_extraction.py:85-99).

Same call, same files: reads ``cfg.paths.mat_data / cfg.paths.mat_filename``
(one variable per modulation, ``cfg.signals.mat_info[mod]``, shaped
``(n_snr, n_frames, >= frame_size)`` complex; feature_extraction.py:46-48) and
writes ``cfg.paths.calculated_features / f"{mod}_features.mat"`` holding exactly
``"Modulation"`` and ``mat_info[mod]`` -> float32 ``(n_snr, n_frames, 18)``
(feature_extraction.py:56,77-81), so preprocessing / plotting / training code
that loads those files is untouched.

What is different underneath:
* every variable of the container is decoded ONCE, by one process, one
  modulation at a time (the reference decodes the whole file in each of its six
  child processes, feature_extraction.py:46-47), and the three stages overlap:
  a reader thread decodes modulation k+1 while modulation k is on the GPU and a
  writer thread saves k-1;
* there are no worker processes or threads on the compute side.  A modulation goes
  to the GPU AS IT LIES in host memory (``amcx_ctx_features18_strided_host``,
  include/amcx.h): ``scipy.io.loadmat`` hands back Fortran-ordered arrays, in which a
  frame's samples are ``n_snr * n_frames`` elements apart but a sample PLANE is
  contiguous, so planes are staged into pinned memory by a few host threads
  (``cfg.signals.num_threads``; doubles are rounded to float32 on the way, so PCIe
  carries 8 bytes per sample), uploaded while the next planes are staged, and
  transposed to frame-major by a device kernel.  No transposed copy of the
  container is ever made on the host and the ``[0:frame_size]`` slice of a frame
  (feature_extraction.py:68) is just the first ``frame_size`` planes;
* with several ranks (one process per GPU of one node, ``torch.distributed``
  initialised by the caller) a variable the fast reader can map (an
  uncompressed level-5 variable of doubles or singles) is mapped by every rank
  for itself -- the page cache is shared, nothing is decoded or copied; anything
  else is decoded by rank 0 alone, which publishes the part the configuration
  uses, in the order it lies in memory, as a memory-mapped file in shared
  memory.  Either way every rank uploads its own contiguous frame range over its
  own PCIe link, and rank 0 gathers the (F x 18) rows and writes the files
  (amcpy_amd/sharding.py).  No collective touches the IQ data;
* several GPUs need no launcher: ``run_extraction(cfg, devices=[0, 1, ...])`` (``python -m amcpy_amd extract
  --devices all``) drives one engine per device from one host thread each inside ONE process
  (:class:`DeviceFanOut`): every device takes its share of the frame axis, reads it from the file over its own
  staging threads and PCIe link, and writes its rows straight into the result -- no process group, no gather;
* a failure raises, on every rank: the reference's worker threads swallow
  exceptions and leave zero rows behind (feature_extraction.py:33-39), and its
  parent ignores the children's exit codes (:96-97).
"""
from __future__ import annotations

import functools
import json
import os
import socket
import tempfile
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from contextlib import closing
from pathlib import Path
from typing import Callable, List, Optional

import numpy as np

from . import _formats, _lib
from .config import Config
from .frame_sources import (FileComplex, FrameColumns, FrameRows, SplitComplex, _native_source,  # noqa: F401 (re-exported)
                            as_frame_rows)
from .sharding import FrameCut, collectives_forced, sharded_features


def _process_group_up() -> bool:
    try:
        import torch.distributed as dist
        return _lib.torch_wanted() and dist.is_available() and dist.is_initialized()
    except Exception:
        return False


def _rank_world():
    if not _lib.torch_wanted():          # a process that opted out of torch has no process group
        return 0, 1
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except Exception:
        pass
    return 0, 1


# ----------------------------------------------------------------------------
# host container -> HBM -> features: the native upload pipeline
# ----------------------------------------------------------------------------
class HipEngine:
    """``engine(frames) -> (F, 18) float32`` through device memory.

    ``frames`` is an (F, L) array / memmap -- complex, real, or sc16: (F, L) of ``features.SC16`` or (F, L, 2) int16
    (I, Q) pairs, which go up as they lie, 4 bytes per sample, and are multiplied by ``sc16_scale`` on the device
    (amcx_features_sc16), or 8-bit: (F, L) of ``features.CI8`` / ``CU8`` or (F, L, 2) int8 / uint8 pairs, 2 bytes per sample
    over the link, widened by the device and multiplied by ``iq8_scale`` (amcx_features_iq8) -- or a :class:`FrameRows` over an (n_snr, n_frames, L)
    container in any memory order (ndarray or :class:`SplitComplex`).  The container is read where it
    lies by ``amcx_ctx_features18_strided_host``: host threads stage contiguous runs -- sample planes
    of a Fortran-ordered container, rows of a C-ordered one -- into three pinned slots (rounding
    doubles to float32 on the way), the copy engine drains them, a device kernel transposes planes to
    frame-major, the feature kernel runs, the (F x 18) result comes back.  ``chunk_bytes`` is the size
    of one pinned slot, ``threads`` the staging threads (the reference's ``num_threads``).
    ``stats`` of the last call: frames, seconds, bytes over PCIe, source bytes, chunks, threads."""

    def __init__(self, frame_size: int, device: Optional[int] = None, chunk_bytes: int = 32 << 20,
                 threads: Optional[int] = None, round_on_device: bool = False, feature_ids=None,
                 sc16_scale: float = _formats.get("sc16").scale, iq8_scale: float = _formats.get("ci8").scale):
        self.N = int(frame_size)
        # what the context multiplies an integer component by, per format (cf32 has none)
        self.scales = {f.name: _formats.check_scale(sc16_scale if f.family == "sc16" else iq8_scale)
                       for f in _formats.TABLE if f.family is not None}
        # feature_ids: None (all 18) or the ids to compute; the result stays (F, 18), NaN outside the set (KeyError for an
        # unknown id, here, before anything is launched)
        self.feature_ids = _feature_ids(feature_ids)
        self.mask = _lib.FEATURES_ALL if self.feature_ids is None else _lib.feature_mask(self.feature_ids)
        if device is None:
            device = 0
            if _lib.torch_wanted():
                try:
                    import torch
                    if torch.cuda.is_available():
                        device = torch.cuda.current_device()
                except Exception:
                    pass
        self.device = int(device)
        self.chunk_bytes = int(chunk_bytes)
        self.threads = max(1, min(int(threads or 8), os.cpu_count() or 1))
        self.round_on_device = bool(round_on_device)
        self._ctx: Optional[_lib.HostContext] = None
        self.stats = {}

    def _context(self) -> "_lib.HostContext":
        if self._ctx is None:
            self._ctx = _lib.HostContext(self.device)
            self._ctx.configure(self.threads, self.chunk_bytes, int(self.round_on_device))
            self._ctx.set_feature_mask(self.mask)
            for fmt, scale in self.scales.items():
                self._ctx.set_scale(fmt, scale)
        return self._ctx

    sc16_scale = property(lambda self: self.scales["sc16"])
    iq8_scale = property(lambda self: self.scales["ci8"])

    def _run_block(self, src, base_elems: int, n_snr: int, n_frames: int, strides, out: np.ndarray) -> None:
        keep, re_ptr, im_ptr, kind, _, item, fd = src
        if fd is not None:
            # a file is read run by run (one pread each): worth it for whole planes or rows, not for the few snr
            # values per sample that a shard cut across the snr axis leaves of a column-major plane
            ss, sk, sn = strides
            if sn == 1:
                run = self.N * (n_frames if sk == self.N else 1)       # rows that follow each other are one read
            elif sk == 1 and n_frames > 1:
                run = n_snr * n_frames if ss == n_frames else n_frames
            else:
                run = n_snr * n_frames if sk == n_snr else n_snr
            if run * item < (8 << 10):
                src = _native_source(keep._mapped())
                keep, re_ptr, im_ptr, kind, _, item, fd = src
        ctx = self._context()
        run = ctx.run_strided if fd is None else functools.partial(ctx.run_file, fd)
        run(re_ptr + base_elems * item, None if im_ptr is None else im_ptr + base_elems * item,
            kind, n_snr, n_frames, self.N, strides, out)
        st = ctx.upload_stats()
        for k in ("frames", "source_bytes", "pcie_bytes", "chunks", "seconds_staging", "seconds_waiting",
                  "seconds_prepare", "seconds_tail", "seconds"):
            self.stats[k] = self.stats.get(k, 0) + st[k]
        self.stats["gather_threads"], self.stats["plane_major"] = st["threads"], st["plane_major"]
        self.stats["from_file"] = max(self.stats.get("from_file", 0), st["from_file"])

    def __call__(self, frames) -> np.ndarray:
        rows = as_frame_rows(frames)
        F, L = rows.shape
        if L < self.N:
            raise ValueError(f"rows of {L} samples are shorter than frame_size {self.N}")
        if F == 0:
            return np.empty((0, 18), dtype=np.float32)
        t0 = time.perf_counter()
        self.stats = {}
        parsed = rows.parsed
        src = _native_source(parsed)
        if src is not None:
            st = src[4]
            unit = [st[2] == 1, st[1] == 1 and rows.n_frames > 1, st[0] == 1 or rows.n_snr == 1]
            if not any(unit):
                src = None
        if src is None:
            # integer / half / exotic dtypes, negative or sub-element strides, no contiguous axis: one
            # C-ordered copy of the part that is used, then the row path
            # (sc16 stays sc16, 8-bit stays 8-bit: the library takes their row layouts only)
            block = np.ascontiguousarray(rows.to_array(),
                                         dtype=rows.dtype if _formats.by_store(rows.dtype) else np.complex128)
            rows = FrameRows(block[None], 1, F)
            src = _native_source(rows.parsed)
        ss, sk, sn = src[4]
        out = np.empty((F, 18), dtype=np.float32)
        row = 0
        for s0, s1, k0, k1 in rows.blocks():
            n = (s1 - s0) * (k1 - k0)
            self._run_block(src, s0 * ss + k0 * sk, s1 - s0, k1 - k0, (ss, sk, sn), out[row:row + n])
            row += n
        self.stats["seconds_native"] = self.stats.pop("seconds", 0.0)
        self.stats["seconds"] = time.perf_counter() - t0
        self.stats["bytes_uploaded"] = self.stats.get("pcie_bytes", 0)
        return out

    def close(self) -> None:
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None


_ENGINES = {}


def default_engine(frame_size: int, device: Optional[int] = None, threads: Optional[int] = None,
                   feature_ids=None) -> HipEngine:
    """The process's engine for (frame_size, device, threads), created on first use and kept: a context is two
    streams, three pinned slots and device scratch (~10 ms to set up, ~8 ms to tear down -- as long as a whole
    BASELINE configs[0] run takes).  :func:`release_engines` frees them."""
    probe = HipEngine(frame_size, device, threads=threads, feature_ids=feature_ids)
    key = (probe.N, probe.device, probe.threads) + ((probe.mask,) if probe.feature_ids is not None else ())
    eng = _ENGINES.get(key)
    if eng is None:
        eng = _ENGINES[key] = probe
    return eng


def release_engines() -> None:
    """Free the contexts :func:`default_engine` keeps (pinned host memory, device scratch, staging threads)."""
    while _ENGINES:
        _ENGINES.popitem()[1].close()


def staging_threads_per_device(places, want: Optional[int] = None, allowed=None):
    """Staging threads for each engine of a one-process fan-out.  ``places[i] = (numa node, [cpus local to device i])``
    (``_lib.numa_place``; node -1: unknown).  An engine whose device has a known node shares that node's CPUs -- those
    of them this process may run on (``allowed``, default ``os.sched_getaffinity(0)``) -- with the other engines on the
    node; the rest share all allowed CPUs evenly, as before round 5.  At most ``want`` (default 8) and at least 1 each."""
    allowed = set(os.sched_getaffinity(0)) if allowed is None else set(allowed)
    want = max(1, int(want or 8))
    on_node = {}
    for node, _ in places:
        on_node[node] = on_node.get(node, 0) + 1
    out = []
    for node, cpus in places:
        local = len(allowed.intersection(cpus)) if node >= 0 else 0
        share = local // on_node[node] if local else len(allowed) // len(places)
        out.append(max(1, min(want, share)))
    return out


class DeviceFanOut:
    """``engine(rows) -> (F, 18) float32`` over SEVERAL devices from one process: one :class:`HipEngine` (context,
    streams, pinned slots, staging threads) per entry of ``devices`` and one host thread each -- the native call
    releases the GIL, ``hipSetDevice`` is per thread (the C ABI's host entries take the device index).  Where the
    reference forks a process per modulation and threads inside it (feature_extraction.py:58-61,89-97), this cuts
    every modulation over the devices: along its FRAME axis when that balances (``sharding.shard_by_frames`` -- one
    contiguous run per sample plane of a column-major .mat), along the snr-major flattening otherwise.  Each device's
    rows land directly in the result; no process group and no gather are involved.  A device may be listed twice
    (two contexts on it: how the one-GPU test box exercises the path).  ``frames`` is whatever one :class:`HipEngine`
    takes (``as_frame_rows``), a :class:`SplitComplex`, (F, L, 2) int16 pairs -- at the engines' default
    ``sc16_scale`` -- and int8 / uint8 pairs -- at ``iq8_scale`` -- included."""

    def __init__(self, frame_size: int, devices, threads: Optional[int] = None, chunk_bytes: int = 32 << 20,
                 feature_ids=None, iq8_scale: float = _formats.get("ci8").scale):
        devices = [int(d) for d in devices]
        feature_ids = _feature_ids(feature_ids)
        if feature_ids is not None:
            _lib.feature_mask(feature_ids)                  # KeyError for an unknown id before any device is touched
        if not devices:
            raise ValueError("DeviceFanOut needs at least one device")
        have = _lib.load().amcx_device_count()
        bad = [d for d in devices if d < 0 or (have > 0 and d >= have)]
        if bad:
            raise ValueError(f"device index {bad[0]} out of range: {have} gfx950 device(s) visible")
        self.N, self.devices = int(frame_size), devices
        # the staging threads of all devices share the host's cores: a device's engine gets its share of the CPUs LOCAL to
        # it (the socket it hangs off: _lib.numa_place reads the kernel's PCI tree; the context binds its threads and
        # pinned slots there by itself), or of all CPUs when the platform does not say
        self.places = [self._place(d) for d in devices]
        per_dev = staging_threads_per_device(self.places, threads)
        self.engines = []
        try:
            for d, n in zip(devices, per_dev):
                self.engines.append(HipEngine(frame_size, d, chunk_bytes, threads=n, feature_ids=feature_ids,
                                              iq8_scale=iq8_scale))
        except BaseException:
            for e in self.engines:                          # a later device failed: the earlier ones' contexts, pinned slots
                e.close()                                   # and staging threads are released, not leaked
            raise
        self.threads = min(per_dev)
        self._pool = ThreadPoolExecutor(max_workers=len(devices), thread_name_prefix="amcx-device")
        self.stats = {}

    @staticmethod
    def _place(device: int):
        """(numa node, [local cpus]) of a device, (-1, []) if unknown or switched off (AMCX_NUMA=0)."""
        if os.environ.get("AMCX_NUMA", "1")[:1] == "0":
            return -1, []
        try:
            return _lib.numa_place(_lib.device_pci_bus_id(device), os.environ.get("AMCX_SYSFS_ROOT", ""))
        except Exception:
            return -1, []

    def placement(self):
        """What each engine's context bound itself to (amcx_ctx_placement), in device order."""
        return [e._context().placement() for e in self.engines]

    def __call__(self, frames) -> np.ndarray:
        rows = as_frame_rows(frames)
        F = rows.shape[0]
        out = np.empty((F, 18), dtype=np.float32)
        if F == 0:
            return out
        t0 = time.perf_counter()
        cut = _frame_cut(rows, len(self.engines))
        shares = [_share(rows, cut, i) for i in range(cut.world)]
        futs = [self._pool.submit(_features_of, e, part) for e, part in zip(self.engines, shares)]
        failures = []
        for i, fut in enumerate(futs):                      # every device finishes (or fails) before anything is raised
            try:
                blk = fut.result()
            except Exception as exc:
                failures.append(f"device {self.devices[i]}: {type(exc).__name__}: {exc}")
                continue
            cut.place(out, i, blk)
        if failures:
            raise RuntimeError("feature extraction failed on " + "; ".join(failures))
        self.stats = {"seconds": time.perf_counter() - t0, "devices": list(self.devices),
                      "frames_per_device": [part.shape[0] for part in shares],
                      "bytes_uploaded": sum(e.stats.get("bytes_uploaded", 0) for e in self.engines),
                      "source_bytes": sum(e.stats.get("source_bytes", 0) for e in self.engines)}
        return out

    def close(self) -> None:
        self._pool.shutdown(wait=True)
        for e in self.engines:
            getattr(e, "close", lambda: None)()


def default_fanout(frame_size: int, devices, threads: Optional[int] = None, feature_ids=None) -> DeviceFanOut:
    """The process's :class:`DeviceFanOut` for (frame_size, devices, threads), kept like :func:`default_engine`'s."""
    ids = _feature_ids(feature_ids)
    key = (int(frame_size), tuple(int(d) for d in devices), max(1, int(threads or 8))) + \
        ((_lib.feature_mask(ids),) if ids is not None else ())
    eng = _ENGINES.get(key)
    if eng is None:
        eng = _ENGINES[key] = DeviceFanOut(frame_size, devices, threads, feature_ids=ids)
    return eng


def _feature_ids(feature_ids):
    """None (all 18) or the sorted distinct ids of a subset; all 18 given explicitly is None too (the 18-feature path)."""
    if feature_ids is None:
        return None
    ids = list(feature_ids)
    _lib.feature_mask(ids)                                  # KeyError for an unknown id, ValueError for none
    ids = tuple(sorted({int(f) for f in ids}))
    return None if ids == tuple(range(1, 19)) else ids


def _masked_compute(compute, feature_ids):
    """An injected engine (tests: a CPU stand-in) under a feature subset: its (F, 18) result with NaN outside the set, the
    file layout the native engine produces."""
    if feature_ids is None:
        return compute
    drop = np.array([j for j in range(18) if j + 1 not in feature_ids], dtype=np.int64)

    def run(block):
        mat = np.array(compute(block), dtype=np.float32, copy=True)
        mat[..., drop] = np.nan
        return mat
    return run


def _subset(feature_ids, compute):
    """The prologue of every entry point: ``(_feature_ids(feature_ids), the injected engine masked to them or None)``."""
    feature_ids = _feature_ids(feature_ids)
    return feature_ids, (None if compute is None else _masked_compute(compute, feature_ids))


def _frame_cut(rows: FrameRows, world: int) -> FrameCut:
    """The cut of ``rows`` over ``world`` workers: a whole container's, or the flat one of any other range."""
    if type(rows) is FrameRows and rows.lo == 0 and rows.hi == rows.n_snr * rows.n_frames:
        return FrameCut(rows.n_snr, rows.n_frames, world)
    return FrameCut.flat(rows.shape[0], world)


def _share(rows: FrameRows, cut: FrameCut, rank: int) -> FrameRows:
    """Worker ``rank``'s source under ``cut``: its frames of every snr row, or its range of the flattening."""
    lo, hi = cut.range(rank)
    if cut.by_frames:
        return FrameColumns(rows.parsed, rows.n_snr, rows.n_frames, lo, hi)
    return rows.slice(lo, hi)


def _features_of(engine, part: FrameRows) -> np.ndarray:
    """``engine(part)`` as float32; an empty share does not reach the engine."""
    if part.shape[0] == 0:
        return np.empty((0, 18), dtype=np.float32)
    return np.asarray(engine(part), dtype=np.float32)


def _file_stream_features(path, store, offset: int, n_frames: int, N: int, device, feature_ids,
                          scale=None) -> np.ndarray:
    """An interleaved stream ``offset`` bytes into a file: the staging threads read it themselves, part by part."""
    stream = FileComplex(path, store, (1, n_frames, N), offset, interleaved=True)
    try:
        engine = HipEngine(N, device, feature_ids=feature_ids, **_formats.scale_kw(_formats.by_store(store).name, scale))
        return np.asarray(engine(FrameRows(stream, 1, n_frames)), dtype=np.float32)
    finally:
        stream.release()


def _check_container(parsed, cfg: Config):
    n_snr = len(cfg.signals.snr_values)
    n_frames = cfg.signals.num_frames
    N = cfg.signals.frame_size
    if len(cfg.features.all_features) != 18:
        raise ValueError("the extraction engine always produces the 18 features of FeatureConfig.all_features")
    if parsed.ndim != 3 or parsed.shape[0] < n_snr or parsed.shape[1] < n_frames or parsed.shape[2] < N:
        raise ValueError(f"container array has shape {parsed.shape}, config needs "
                         f"(>={n_snr}, >={n_frames}, >={N})")
    return n_snr, n_frames, N


def extract_modulation(parsed: np.ndarray, cfg: Config, *, compute=None, device: Optional[int] = None,
                       group=None, feature_ids=None) -> Optional[np.ndarray]:
    """All 18 features of one modulation's ``(n_snr, n_frames, L)`` array, which every rank
    holds (``run_extraction`` itself decodes on rank 0 only).  Returns float32
    ``(n_snr, n_frames, 18)`` on rank 0 (None on other ranks).  ``feature_ids``: only these (NaN in the other columns)."""
    feature_ids, compute = _subset(feature_ids, compute)
    n_snr, n_frames, N = _check_container(parsed, cfg)
    rank, world = _rank_world()
    rows = FrameRows(parsed, n_snr, n_frames)
    if compute is None:
        engine = HipEngine(N, device, threads=cfg.signals.num_threads, feature_ids=feature_ids)
        cut = _frame_cut(rows, world)
        mat = cut.gather(_features_of(engine, _share(rows, cut, rank)), rank, group)
    else:                           # injected engine (tests): plain (F, L) arrays
        mat = sharded_features(rows.to_array(), N, compute, rank, world, group)
    return None if mat is None else mat.reshape(n_snr, n_frames, 18)


def extract_raw_stream(path, frame_size: int, *, skip_samples: int = 0, max_frames: Optional[int] = None,
                       compute=None, device: Optional[int] = None, feature_ids=None, sample_format: str = "cf32",
                       scale: float = _formats.get("sc16").scale, scale8: float = _formats.get("ci8").scale) -> np.ndarray:
    """Features of a raw complex64 sample stream on disk (GNU Radio file sink: interleaved
    float32 I/Q, no header -- what the reference's legacy reader takes with
    ``np.fromfile(..., dtype=np.complex64)`` and a fixed number of leading samples dropped,
    old/read_binary_stream.py:28,48,54-56), or, ``sample_format="sc16"``, of a stream of int16 (I, Q) pairs (UHD sc16,
    SigMF ci16_le), each component multiplied by ``scale`` on the device, or, ``"ci8"`` / ``"cu8"``, of a stream of int8 /
    uint8 (I, Q) pairs (HackRF / RTL-SDR recordings; cu8: zero level 128), each component multiplied by ``scale8``.  The file is memory-mapped and cut into
    consecutive ``frame_size``-sample frames (a trailing partial frame is dropped); the staging
    threads read the file slot by slot, so it never has to fit in host memory.
    Returns ``(n_frames, 18)`` float32 (``feature_ids``: only these, NaN in the other columns)."""
    feature_ids, compute = _subset(feature_ids, compute)
    if frame_size < 2:
        raise ValueError("frame_size must be >= 2")
    if skip_samples < 0:
        raise ValueError("skip_samples must be >= 0")
    if sample_format not in _formats.NAMES:
        raise ValueError("sample_format is 'cf32', 'sc16', 'ci8' or 'cu8'")
    store = _formats.get(sample_format).store
    # the one of the two keywords that is this format's (the other is not read)
    scale = _formats.scale_of(sample_format, scale if sample_format == "sc16" else scale8)
    n_total = Path(path).stat().st_size // store.itemsize - skip_samples
    n_frames = max(0, n_total // frame_size)
    if max_frames is not None:
        n_frames = min(n_frames, int(max_frames))
    if n_frames == 0:
        return np.empty((0, 18), dtype=np.float32)
    if compute is None:
        return _file_stream_features(path, store, store.itemsize * skip_samples, n_frames, frame_size, device,
                                     feature_ids, scale)
    frames = np.memmap(path, dtype=store, mode="r", offset=store.itemsize * skip_samples,
                       shape=(n_frames, frame_size))
    if sample_format != "cf32":         # an injected engine (tests) sees the complex64 frames the device computes on
        frames = widen_integer_frames(frames, scale)
    return np.asarray(compute(frames), dtype=np.float32)


def widen_integer_frames(frames: np.ndarray, scale: float) -> np.ndarray:
    """(..., L) ``SC16`` / ``CI8`` / ``CU8`` samples -> the complex64 frames the device computes on (host copy: tests and
    injected engines): complex64(float32(i) * scale, float32(q) * scale), cu8 components around the zero level 128."""
    zero = _formats.by_store(frames.dtype).zero
    wide = np.empty(frames.shape, dtype=np.complex64)
    for part, name in ((wide.real, "i"), (wide.imag, "q")):
        part[...] = (frames[name].astype(np.int16) - zero).astype(np.float32) * np.float32(scale)
    return wide


def _pairs_as_complex(block: np.ndarray) -> np.ndarray:
    """(g, L, 2) float32 -> (g, L) complex64 view (bit-identical layouts); copies only if the pairs
    are not interleaved in memory."""
    if block.strides[-1] != 4 or block.strides[-2] != 8:
        block = np.ascontiguousarray(block)
    return block.view(np.complex64)[..., 0]


def extract_iq_pairs(dataset, frame_size: Optional[int] = None, *, first_frame: int = 0,
                     max_frames: Optional[int] = None, compute=None, device: Optional[int] = None,
                     chunk_frames: Optional[int] = None, feature_ids=None) -> np.ndarray:
    """Features of frames stored as float32 (I, Q) pairs, ``dataset[f, n] = (I, Q)`` -- RadioML's
    ``(F, 1024, 2)`` layout (reference old/dataset.py:50-56, old/dataset_analysis.py:22).  ``dataset``
    is anything sliceable with ``.shape`` and ``.dtype``.  A numpy array or memmap is re-viewed as
    complex64 and goes up in one native call; any other dataset (an ``h5py.Dataset``, which decodes
    chunks from the file as they are sliced) is read ``chunk_frames`` at a time by a reader thread one
    chunk ahead of the upload, so the set never has to fit in host memory.  Returns ``(n_frames, 18)``
    float32 (``feature_ids``: only these, NaN in the other columns)."""
    feature_ids, compute = _subset(feature_ids, compute)
    shape = tuple(dataset.shape)
    if len(shape) != 3 or shape[2] != 2:
        raise ValueError(f"expected an (F, L, 2) dataset of (I, Q) pairs, got shape {shape}")
    if np.dtype(dataset.dtype) != np.float32:
        raise TypeError(f"(I, Q) pairs must be float32, got {dataset.dtype}")
    F, L = int(shape[0]), int(shape[1])
    N = L if frame_size is None else int(frame_size)
    if N < 2 or N > L:
        raise ValueError(f"frame_size {N} outside 2 .. {L}")
    lo = min(max(0, int(first_frame)), F)
    hi = F if max_frames is None else min(F, lo + int(max_frames))
    if hi <= lo:
        return np.empty((0, 18), dtype=np.float32)
    if compute is not None:                       # injected engine (tests): plain (F, N) arrays
        block = np.ascontiguousarray(_pairs_as_complex(np.asarray(dataset[lo:hi]))[:, :N])
        return np.asarray(compute(block), dtype=np.float32)
    from . import hdf5_min
    if (isinstance(dataset, hdf5_min.Dataset) and N == L and dataset.file_offset is not None and dataset.little_endian):
        # a contiguous dataset is a raw interleaved complex64 stream at a known place in the file: the staging threads
        # read it themselves, slot by slot (as extract_raw_stream does), and libhdf5 is not on the data path at all
        return _file_stream_features(dataset.file_path, np.complex64, dataset.file_offset + lo * L * 8, hi - lo, N, device,
                                     feature_ids)
    engine = HipEngine(N, device, feature_ids=feature_ids)
    if isinstance(dataset, np.ndarray):
        return engine(_pairs_as_complex(dataset[lo:hi]))
    step = int(chunk_frames or max(1, (256 << 20) // (L * 8)))
    spans = [(a, min(hi, a + step)) for a in range(lo, hi, step)]
    out = np.empty((hi - lo, 18), dtype=np.float32)
    for (a, b), fut in _prefetched(spans, lambda ab: _pairs_as_complex(np.asarray(dataset[ab[0]:ab[1]]))):
        out[a - lo:b - lo] = engine(fut.result())
    return out


def extract_radioml_hdf5(path, *, key: str = "X", frame_size: Optional[int] = None, first_frame: int = 0,
                         max_frames: Optional[int] = None, device: Optional[int] = None, compute=None,
                         chunk_frames: Optional[int] = None, feature_ids=None) -> np.ndarray:
    """``extract_iq_pairs`` on dataset ``key`` of a RadioML-style HDF5 file (``GOLD_XYZ_OSC.0001_1024.hdf5``:
    ``X`` float32 (2 555 904, 1024, 2), reference old/dataset.py:43-56).  The file is opened with the HDF5 C library
    through ``amcpy_amd.hdf5_min`` (ctypes) where one is found, otherwise with ``h5py``, which the reference lists for
    its legacy scripts (this image ships libhdf5 1.10.6 but no h5py for its interpreter).  A CONTIGUOUS ``X`` at its full
    frame length is then a raw complex64 stream at a known file offset and the engine's staging threads read it
    themselves; a chunked or compressed one is decoded by the library ``chunk_frames`` rows at a time on a reader thread
    ahead of the upload.  Neither library there: ImportError that says so."""
    from . import hdf5_min
    kw = dict(first_frame=first_frame, max_frames=max_frames, device=device, compute=compute, chunk_frames=chunk_frames,
              feature_ids=feature_ids)
    if hdf5_min.available():                      # the C library itself: a contiguous X then bypasses it altogether
        with hdf5_min.File(path) as fh:
            return extract_iq_pairs(fh[key], frame_size, **kw)
    try:
        import h5py
    except ImportError as exc:                    # not a silent fallback: say what is missing
        raise ImportError("extract_radioml_hdf5 needs an HDF5 C library >= 1.10 (AMCX_LIBHDF5=/path/to/libhdf5.so) or h5py "
                          "(pip install h5py); any sliceable (F, L, 2) float32 dataset can be passed to extract_iq_pairs "
                          "instead") from exc
    with h5py.File(str(path), "r") as fh:
        return extract_iq_pairs(fh[key], frame_size, **kw)


# ----------------------------------------------------------------------------
# run_extraction
# ----------------------------------------------------------------------------
def _prefetched(items: List, fn: Callable, depth: int = 3):
    """``(item, future)`` pairs with ``fn(item)`` running on reader threads up to ``depth`` items ahead of the
    consumer: while the caller works on item k, items k+1 .. k+depth are being read / decoded (a memory-mapped
    variable costs nothing to "read"; a compressed one is a zlib inflate of hundreds of megabytes, which
    releases the GIL -- MATLAB's default `save` compresses).  At most ``depth + 1`` items are alive."""
    depth = max(1, int(depth))
    with ThreadPoolExecutor(max_workers=depth, thread_name_prefix="amcx-reader") as ex:
        futs = [ex.submit(fn, it) for it in items[:depth]]
        for i, it in enumerate(items):
            cur = futs[i]
            if i + depth < len(items):
                futs.append(ex.submit(fn, items[i + depth]))
            yield it, cur
            futs[i] = None                                  # drop the reference: the consumer is done with it


def _shared_dir(need_bytes: int) -> Path:
    """Where rank 0 publishes a modulation for the other ranks of the node: /dev/shm (page cache, no
    disk) when it has room, the temp dir otherwise.  Writing a sparse tmpfs file past the mount's
    capacity raises SIGBUS, not an exception, so room is checked BEFORE the file is mapped (a
    container's default /dev/shm is 64 MB; a configs[1] modulation is 3.5 GB)."""
    for cand in (Path("/dev/shm"), Path(tempfile.gettempdir())):
        try:
            if cand.is_dir() and os.access(cand, os.W_OK):
                st = os.statvfs(cand)
                if st.f_bavail * st.f_frsize >= need_bytes + (64 << 20):
                    return cand
        except OSError:
            continue
    raise OSError(f"neither /dev/shm nor {tempfile.gettempdir()} has {need_bytes / 1e9:.2f} GB free to publish a "
                  "modulation to the other ranks")


def _copy_parallel(dst: np.ndarray, src, threads: int) -> None:
    """dst <- src over host threads, split along the slowest axis of dst (numpy releases the GIL in copyto)."""
    axis = int(np.argmax(dst.strides))
    n = dst.shape[axis]
    threads = max(1, min(threads, n))
    idx = [slice(None)] * dst.ndim

    def part(a, b):
        sl = list(idx)
        sl[axis] = slice(a, b)
        np.copyto(dst[tuple(sl)], src[tuple(sl)], casting="same_kind")

    if threads == 1:
        part(0, n)
        return
    per = -(-n // threads)
    with ThreadPoolExecutor(max_workers=threads, thread_name_prefix="amcx-publish") as ex:
        for f in [ex.submit(part, a, min(n, a + per)) for a in range(0, n, per)]:
            f.result()


def _publish_container(parsed, n_snr: int, n_frames: int, N: int, threads: int) -> Path:
    """Rank 0: the part of the container the configuration uses -> an .npy in shared memory, IN THE
    MEMORY ORDER IT HAS (Fortran for what loadmat returns: the copy is a run of contiguous planes,
    no transposition), source dtype kept."""
    used = parsed[:n_snr, :n_frames, :N]                 # a view (ndarray) or the assembled part (SplitComplex)
    dtype = used.dtype if used.dtype in (np.complex64, np.complex128) else np.dtype(np.complex128)
    fortran = used.strides[0] < used.strides[2]
    need = n_snr * n_frames * N * dtype.itemsize
    fd, name = tempfile.mkstemp(prefix="amcx_frames_", suffix=".npy", dir=str(_shared_dir(need)))
    os.close(fd)
    try:
        mm = np.lib.format.open_memmap(name, mode="w+", dtype=dtype, shape=(n_snr, n_frames, N), fortran_order=fortran)
        _copy_parallel(mm, used, threads)
        mm.flush()
        del mm
    except BaseException:
        Path(name).unlink(missing_ok=True)
        raise
    return Path(name)


def _load_variable(mat_path: Path, key: str, pool=None, direct: bool = False):
    from .matfile import load_variable
    return load_variable(mat_path, key, pool, direct)


def _read_ahead(inflated_bytes: int, n_variables: int) -> int:
    """How many variables the reader threads decode ahead of the GPU.  An uncompressed container: 1 (it is only
    located, or read at link rate).  A compressed one is inflate-bound, one deflate stream per variable, so every
    variable ahead is a core at work (2.2 / 0.9 / 0.62 s for the 2.6 GB container at 1 / 3 / 6,
    profiles/r3_extract_ab_readahead.txt): up to six, as many as fit twice over in a quarter of the memory the host
    has available.  AMCX_READ_AHEAD overrides."""
    if "AMCX_READ_AHEAD" in os.environ:
        return max(1, int(os.environ["AMCX_READ_AHEAD"]))
    if inflated_bytes <= 0:
        return 1
    avail = 0
    try:
        with open("/proc/meminfo") as fh:
            for line in fh:
                if line.startswith("MemAvailable:"):
                    avail = int(line.split()[1]) * 1024
                    break
    except OSError:
        pass
    fit = (avail // 4) // (2 * inflated_bytes) if avail else 3
    return int(max(1, min(6, n_variables, (os.cpu_count() or 2) - 1, fit)))


def _placement(world: int, device: Optional[int]) -> bool:
    """One all-gather of (host name, device index) per run: True when every rank is on one host (rank 0 then decodes
    for all).  Two ranks on the SAME device of the same host -- a launcher whose ranks never called
    ``set_device(LOCAL_RANK)`` -- would be silently correct and ``world`` times slow: that raises on every rank
    unless AMCX_SHARE_GPU=1 says it is meant (rehearsals on a one-GPU box).  ``device`` None: an injected engine."""
    import torch.distributed as dist
    where = [None] * world
    dist.all_gather_object(where, (socket.gethostname(), device))
    if device is not None and os.environ.get("AMCX_SHARE_GPU", "0") != "1":
        seen = {}
        for r, hd in enumerate(where):
            if hd[1] is not None and hd in seen:
                raise RuntimeError(f"ranks {seen[hd]} and {r} both compute on device {hd[1]} of {hd[0]}: give every rank "
                                   f"its own GPU (torch.cuda.set_device(LOCAL_RANK) before run_extraction, or device=), "
                                   f"or set AMCX_SHARE_GPU=1 if sharing is intended")
            seen[hd] = r
    return len({h for h, _ in where}) == 1


def _provenance(cfg: Config, mat_path: Path, key: str, feature_ids=None) -> dict:
    """What a feature file was computed FROM and FOR: the shape (n_snr, n_frames, 18) says neither the frame size nor
    which SNR labels or which input container -- a file written for another ``--frame-size``, or for a container that
    has since been replaced, has the right shape and stale numbers."""
    try:
        st = Path(mat_path).stat()
        src = {"input_size": st.st_size, "input_mtime_ns": st.st_mtime_ns}
    except OSError:
        src = {"input_size": None, "input_mtime_ns": None}
    rec = {"frame_size": int(cfg.signals.frame_size), "num_frames": int(cfg.signals.num_frames),
           "snr_values": [[int(k), str(v)] for k, v in cfg.signals.snr_values.items()],
           "input": str(Path(mat_path).name), "variable": key, **src}
    if feature_ids is not None:                             # a subset run only: a full run's record is what it always was
        rec["features"] = [int(f) for f in feature_ids]
    return rec


def _provenance_path(out_path: Path) -> Path:
    """Beside the feature file, not inside it: the .mat keeps exactly the two variables the reference writes
    (feature_extraction.py:77-81), which is what its downstream loaders see."""
    return out_path.with_name(out_path.stem + ".provenance.json")


def _already_extracted(out_path: Path, key: str, shape, provenance: Optional[dict] = None) -> bool:
    """True if ``out_path`` is a complete feature file for this configuration: it holds ``key`` as a float32 array
    of ``shape`` (and the ``Modulation`` string) -- only the variable headers are read (``scipy.io.whosmat``) -- AND the
    provenance record written beside it equals ``provenance`` (frame size, SNR labels, frame count, the input
    container's name, size and modification time).  A file that is cut short, was written for another frame size / SNR
    grid / container, or has no record (written before records existed, or by the reference) does not qualify; nor does one
    computed for a feature subset that does not cover the one asked for (no "features" in a record: all 18)."""
    import scipy.io
    try:
        seen = {name: (tuple(shp), cls) for name, shp, cls in scipy.io.whosmat(str(out_path))}
        if seen.get(key) != (tuple(shape), "single") or "Modulation" not in seen:
            return False
        size = out_path.stat().st_size
        if size < 4 * int(np.prod(shape)):                  # the array's bytes are really there
            return False
        if provenance is None:
            return True
        # the features: a record without the key holds all 18; a file serves a request whose ids its record covers
        have = json.loads(_provenance_path(out_path).read_text())
        want = dict(provenance)
        have_ids, want_ids = have.pop("features", None), want.pop("features", None)
        have.pop("channel", None)                           # how `synth --channel` made the IQ, not what the file was computed for
        have.pop("cpm", None)                               # ... and the pulse of a continuous-phase name
        have.pop("recover", None)                           # ... and the carrier recovery `synth --features-only --recover M` put in front
        covers = have_ids is None or (want_ids is not None and set(want_ids) <= set(have_ids))
        return have == want and covers
    except Exception:
        return False


def _extraction_engine(cfg: Config, world: int, compute, device, devices, feature_ids):
    """``engine(FrameRows) -> (F, 18)``: the injected ``compute`` over plain arrays, a fan-out over ``devices``, or one engine."""
    N, threads = cfg.signals.frame_size, max(1, int(cfg.signals.num_threads))
    if devices is not None:
        devices = [int(d) for d in devices]
        if compute is not None or device is not None:
            raise ValueError("devices= stands in for device= / compute=")
        if world > 1:
            raise ValueError("devices= drives several GPUs from one process; with a process group of several ranks "
                             "every rank takes its one device=")
        if len(devices) == 1:
            device, devices = devices[0], None
    if compute is not None:
        return lambda rows: compute(rows.to_array())
    if devices:
        return default_fanout(N, devices, threads, feature_ids)
    return default_engine(N, device, threads, feature_ids)


def _modulations_to_do(cfg: Config, mat_path: Path, rank: int, world: int, resume: bool, feature_ids, verbose: bool):
    """The configuration's modulations, less (``resume``) those rank 0 finds done; every rank gets rank 0's answer."""
    mods = list(cfg.signals.modulations_with_noise)
    if not resume:
        return mods
    todo = mods
    if rank == 0:
        shape = (len(cfg.signals.snr_values), cfg.signals.num_frames, 18)
        todo = [m for m in mods if not _already_extracted(
            cfg.paths.calculated_features / f"{m}_features.mat", cfg.signals.mat_info[m], shape,
            _provenance(cfg, mat_path, cfg.signals.mat_info[m], feature_ids))]
        if verbose and len(todo) < len(mods):
            print(f"resume: {len(mods) - len(todo)} of {len(mods)} feature files are complete, computing {todo}")
    if world > 1:
        import torch.distributed as dist
        box = [todo]
        dist.broadcast_object_list(box, src=0)
        todo = box[0]
    return todo


class _FeatureWriter:
    """Rank 0's one writer thread, and what each file is computed from -- taken here, BEFORE the container is read: a
    container replaced mid-run leaves a record that no longer matches it."""

    def __init__(self, cfg: Config, mat_path: Path, mods, feature_ids, rank: int, verbose: bool):
        import scipy.io
        self.cfg, self.verbose, self._savemat = cfg, verbose, scipy.io.savemat
        self.provenance = {m: _provenance(cfg, mat_path, cfg.signals.mat_info[m], feature_ids) for m in mods}
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="amcx-writer") if rank == 0 else None
        self._writes = []

    def submit(self, mod: str, feats: np.ndarray, t0: float) -> None:
        self._writes.append(self._pool.submit(self._save, mod, feats, t0))

    def _save(self, mod: str, feats: np.ndarray, t0: float) -> None:
        out_path = self.cfg.paths.calculated_features / f"{mod}_features.mat"
        # written aside and renamed: an interrupted run never leaves a partial file under the final name (what
        # resume= and every downstream loader look at)
        tmp_path = out_path.with_name(f"{out_path.stem}.{os.getpid()}.tmp.mat")
        record = _provenance_path(out_path)
        try:
            record.unlink(missing_ok=True)                  # never a fresh record beside an old file, or an old one beside a new
            self._savemat(str(tmp_path), {"Modulation": mod, self.cfg.signals.mat_info[mod]: feats})
            os.replace(tmp_path, out_path)
            record.write_text(json.dumps(self.provenance[mod]) + "\n")
        finally:
            tmp_path.unlink(missing_ok=True)
        if self.verbose:
            print(f"[{mod}] {feats.shape[0] * feats.shape[1]} frames in "
                  f"{time.perf_counter() - t0:.2f}s -> {out_path}")

    def close(self, reraise: bool = True) -> None:
        if self._pool is not None:
            self._pool.shutdown(wait=True)
        for w in self._writes if reraise else ():
            w.result()                                      # a failed savemat raises here


def _single_process_loop(cfg: Config, mat_path: Path, mods, direct: bool, engine, writer: _FeatureWriter) -> None:
    """One process, no collectives: reader threads ahead of the GPU, the writer thread behind it."""
    from .matfile import BufferPool, compressed_variable_bytes
    # A compressed container is inflate-bound: three reader threads run ahead (zlib releases the GIL).  An
    # uncompressed variable is only LOCATED here: the native engine's staging threads read it from the file
    # on their way to the pinned slots.  With an injected engine (tests) it is read with preadv into two
    # pairs of buffers that take turns: reading is faster than first-touching fresh pages, mapped or allocated.
    pool = BufferPool()
    depth = _read_ahead(compressed_variable_bytes(mat_path), len(mods))
    with closing(_prefetched(mods, lambda m: _load_variable(mat_path, cfg.signals.mat_info[m], pool, direct), depth)) as feed:
        for mod, fut in feed:
            t0 = time.perf_counter()
            parsed = fut.result()                           # the reader threads are up to `depth` variables ahead
            try:
                n_snr, n_frames, _ = _check_container(parsed, cfg)
                feats = _features_of(engine, FrameRows(parsed, n_snr, n_frames)).reshape(n_snr, n_frames, 18)
            finally:
                getattr(parsed, "release", lambda: None)()
            del parsed
            writer.submit(mod, feats, t0)


# What the steps of the rank loop share.  mapped: variables rank 0's reader thread has already mapped; published: rank
# 0's shared files not yet removed (run_extraction's list: it removes what a failure leaves behind)
_RankRun = namedtuple("_RankRun", "cfg mat_path direct rank world engine shared_host mapped published")


def decode_locally(run: _RankRun, mod: str):
    """Reader of ranks on different hosts: each decodes for itself, as the reference's children do."""
    parsed = _load_variable(run.mat_path, run.cfg.signals.mat_info[mod], None, run.direct)
    return (parsed,) + _check_container(parsed, run.cfg)[:2]


def decode_and_publish(run: _RankRun, mod: str):
    """Rank 0's reader when all ranks share its host -> ``(path of the published copy or "", n_snr, n_frames)``."""
    parsed, n_snr, n_frames = decode_locally(run, mod)
    if getattr(parsed, "source", None) in ("mapped", "file"):
        run.mapped[mod] = parsed                            # every rank reads / maps the variable itself: nothing to publish
        return "", n_snr, n_frames
    sig = run.cfg.signals
    path = _publish_container(parsed, n_snr, n_frames, sig.frame_size, max(1, int(sig.num_threads)))
    run.published.append(path)                              # (several reader threads publish at once: the path stays local)
    return str(path), n_snr, n_frames


def _rank_reader(run: _RankRun):
    """What this rank's reader thread does ahead of its GPU; on a shared host only rank 0 has one (None elsewhere)."""
    return decode_locally if not run.shared_host else decode_and_publish if run.rank == 0 else None


def _announce(run: _RankRun, mod: str, fut):
    """Step 1, shared host only (else None): every rank learns ``(published path or "", n_snr, n_frames)``, or that rank
    0 could not read the modulation -- then all raise."""
    if not run.shared_host:
        return None
    import torch.distributed as dist
    meta = [None]
    if run.rank == 0:
        try:
            meta = [("ok",) + fut.result()]
        except Exception as exc:                            # every rank must leave the collective
            meta = [("error", repr(exc), 0, 0)]
    dist.broadcast_object_list(meta, src=0)
    status, shared, n_snr, n_frames = meta[0]
    if status != "ok":
        raise RuntimeError(f"rank 0 could not read {run.cfg.signals.mat_info[mod]!r} from {run.mat_path}: {shared}")
    return shared, n_snr, n_frames


def _compute_share(run: _RankRun, mod: str, fut, where):
    """Step 2: this rank's share -> ``(cut, local rows, failure)``.  Nothing raises: a failure is kept, as a string, until
    every rank has reported.  The container is let go of on return, so nobody maps a shared file past step 3."""
    cut = local = None
    try:
        if where is None:
            parsed, n_snr, n_frames = fut.result()
        else:
            shared, n_snr, n_frames = where
            if shared:
                parsed = np.load(shared, mmap_mode="r")
            else:                                           # mapped straight from the container, by every rank
                parsed = run.mapped.pop(mod, None) if run.rank == 0 else None
                if parsed is None:
                    parsed = _load_variable(run.mat_path, run.cfg.signals.mat_info[mod], None, run.direct)
                _check_container(parsed, run.cfg)
        cut = FrameCut(n_snr, n_frames, run.world)          # the same answer on every rank
        local = _features_of(run.engine, _share(FrameRows(parsed, n_snr, n_frames), cut, run.rank))
        # a wrong row count would raise inside the gather on THIS rank only and leave the others in the
        # collective: it is reported with the status word instead
        if local.shape != (cut.rows(run.rank), 18):
            raise RuntimeError(f"engine returned {local.shape} for {cut.rows(run.rank)} frames")
    except Exception as exc:
        return cut, local, f"{type(exc).__name__}: {exc}"
    return cut, local, None


def _agree_and_gather(run: _RankRun, mod: str, where, cut, local, failure):
    """Step 3: one status word per rank BEFORE the data collective -- all ranks raise together, or all gather.  The
    all-gather is also the point after which nobody maps the shared file any more: rank 0 removes it."""
    import torch.distributed as dist
    statuses = [None] * run.world
    dist.all_gather_object(statuses, failure)
    if where is not None and run.rank == 0 and where[0]:
        Path(where[0]).unlink(missing_ok=True)
        run.published.remove(Path(where[0]))
    bad = [(r, s) for r, s in enumerate(statuses) if s is not None]
    if bad:
        raise RuntimeError(f"feature extraction of {mod!r} failed on " + "; ".join(f"rank {r}: {s}" for r, s in bad))
    return cut.gather(local, run.rank)


def _rank_loop(run: _RankRun, mods, writer: _FeatureWriter) -> None:
    """Several ranks (or one, under ``collectives_forced``): the three steps per modulation; rank 0 writes."""
    reader = _rank_reader(run)
    feed = ((m, None) for m in mods) if reader is None else _prefetched(mods, functools.partial(reader, run))
    with closing(feed):                                     # waits for a decode / publish still in flight
        for mod, fut in feed:
            t0 = time.perf_counter()
            where = _announce(run, mod, fut)
            cut, local, failure = _compute_share(run, mod, fut, where)
            mat = _agree_and_gather(run, mod, where, cut, local, failure)
            if run.rank == 0:
                writer.submit(mod, mat.reshape(cut.n_snr, cut.n_frames, 18), t0)


def run_extraction(cfg: Config, *, compute=None, device: Optional[int] = None, devices=None,
                   verbose: bool = True, resume: bool = False, feature_ids=None) -> None:
    """Drop-in for the reference's ``run_extraction(cfg)``: writes one
    ``{mod}_features.mat`` per entry of ``cfg.signals.modulations_with_noise``.
    ``devices``: several GPU indices driven from THIS process (:class:`DeviceFanOut`; not together with a process
    group of several ranks, where every rank has its one ``device``).
    ``resume``: modulations whose feature file is already there, complete, of this configuration's shape AND recorded
    (``{mod}_features.provenance.json`` beside it) as computed for this frame size, these SNR labels and this very input
    container (name, size, modification time) are skipped -- the per-modulation file is the path's natural resume unit (the reference recomputes everything,
    all-or-nothing per file; a file is written by ONE savemat call at the end of its modulation, here as there).
    ``feature_ids``: only these features (KeyError for an unknown id, before anything runs); the files keep the
    reference's ``(n_snr, n_frames, 18)`` float32 layout with NaN in the other columns, and the record beside each file
    lists them (``"features"``) -- a full run's record does not change.  ``resume`` trusts a file whose recorded set
    covers the one asked for."""
    native = compute is None
    feature_ids, compute = _subset(feature_ids, compute)
    rank, world = _rank_world()
    cfg.paths.ensure_dirs()
    mat_path = cfg.paths.mat_data / cfg.paths.mat_filename
    engine = _extraction_engine(cfg, world, compute, device, devices, feature_ids)
    mods = _modulations_to_do(cfg, mat_path, rank, world, resume, feature_ids, verbose)
    t_start = time.perf_counter()
    # uncompressed variables go from the file to the pinned slots inside the native engine (AMCX_DIRECT_FILE=0: read /
    # map them in Python first, the round-3 path kept for A/B runs); an injected engine gets arrays
    direct = native and os.environ.get("AMCX_DIRECT_FILE", "1") != "0"
    writer = _FeatureWriter(cfg, mat_path, mods, feature_ids, rank, verbose)
    published: List[Path] = []
    try:
        if world == 1 and not (collectives_forced() and _process_group_up()):
            _single_process_loop(cfg, mat_path, mods, direct, engine, writer)
        else:
            shared_host = _placement(world, getattr(engine, "device", None))
            _rank_loop(_RankRun(cfg, mat_path, direct, rank, world, engine, shared_host, {}, published), mods, writer)
        writer.close()                                      # a failed savemat raises here
    finally:
        writer.close(reraise=False)
        for path in list(published):
            Path(path).unlink(missing_ok=True)
    if verbose and rank == 0:
        print(f"All feature calculations complete! ({time.perf_counter() - t_start:.2f}s)")
