"""Frame sources: rows of the C-order flattening (snr-major) of a container array, wherever it lies -- an ndarray or
memmap in any memory order, two real arrays, or still in its file.  No engine and no process group in here."""
from __future__ import annotations

import os
import threading
from pathlib import Path
from typing import Iterator, Optional, Tuple

import numpy as np

from . import _formats, _lib

# the element kinds of a container that are no sample formats of the table: doubles, and real arrays (two of them: a split container)
_OTHER_KINDS = {np.dtype(np.complex128): _lib.SRC_C128, np.dtype(np.float32): _lib.SRC_F32_SPLIT,
                np.dtype(np.float64): _lib.SRC_F64_SPLIT}


def _kind_of(dtype):
    """The ``AMCX_SRC_*`` kind of a container of ``dtype`` elements, or None where the library reads none such."""
    fmt = _formats.by_store(dtype)
    return _OTHER_KINDS.get(np.dtype(dtype)) if fmt is None else fmt.kind


class SplitComplex:
    """A complex ``(n_snr, n_frames, L)`` container held as two real arrays of equal shape, strides
    and dtype (float32 / float64) -- how a MATLAB v5 file stores a complex variable, so a
    memory-mapped .mat goes to the GPU without a complex array being built (amcpy_amd/matfile.py).
    ``imag`` may be None (a real signal).  Indexing returns an ordinary complex ndarray."""

    def __init__(self, real: np.ndarray, imag: Optional[np.ndarray]):
        if imag is not None and (imag.shape != real.shape or imag.strides != real.strides or imag.dtype != real.dtype):
            raise ValueError("real and imaginary parts must agree in shape, strides and dtype")
        if real.dtype not in (np.float32, np.float64):
            raise TypeError(f"split containers hold float32 or float64, got {real.dtype}")
        self.real, self.imag = real, imag
        self.source = None            # "mapped": views of a memory-mapped file every process can map for itself
        self.shape, self.ndim = real.shape, real.ndim
        self.dtype = np.dtype(np.complex64 if real.dtype == np.float32 else np.complex128)

    def __getitem__(self, idx) -> np.ndarray:
        out = np.asarray(self.real[idx]).astype(self.dtype)
        if self.imag is not None:
            out.imag = self.imag[idx]
        return out


class FileComplex:
    """A complex ``(n_snr, n_frames, L)`` container that is still in its FILE: the byte offsets of its real and
    imaginary arrays (column-major float32 / float64, how a level-5 .mat stores an uncompressed complex variable;
    ``imag_offset`` None: a real signal), or of ONE interleaved complex array (``interleaved=True``: a raw
    complex64 / complex128 stream, or a stream of sc16 samples -- ``store_dtype=features.SC16``, int16 (I, Q) pairs -- or of
    8-bit samples -- ``features.CI8`` / ``features.CU8`` -- C-ordered; with ``order="F"`` the {real, imag} compound dataset of a MATLAB -v7.3
    file, whose bytes are the column-major variable).  Nothing is read or mapped here: the engine's staging threads pread
    the file block by block on their way to the pinned slots (``amcx_ctx_features18_strided_file``), so the
    variable never exists in host memory outside the page cache.  Indexing (tests, injected engines) goes
    through a memory mapping.  ``release()`` closes the descriptor."""

    def __init__(self, path, store_dtype, shape, real_offset: int, imag_offset: Optional[int] = None, *,
                 interleaved: bool = False, order: Optional[str] = None):
        self.path = Path(path)
        self.store = np.dtype(store_dtype)
        self.interleaved = bool(interleaved)
        if not self.interleaved and self.store not in (np.float32, np.float64):
            raise TypeError(f"split containers hold float32 or float64, got {self.store}")
        if self.interleaved and self.store != np.complex128 and _formats.by_store(self.store) is None:
            raise TypeError(f"interleaved containers hold complex64, complex128, sc16, ci8 or cu8, got {self.store}")
        self.shape, self.ndim = tuple(int(x) for x in shape), len(shape)
        self.real_offset, self.imag_offset = int(real_offset), (None if imag_offset is None else int(imag_offset))
        self.dtype = self.store if self.interleaved else \
            np.dtype(np.complex64 if self.store == np.float32 else np.complex128)
        # element strides: column-major for the split arrays of a .mat (and a -v7.3 compound), row-major for a raw stream
        self.order = order if order is not None else ("C" if self.interleaved else "F")
        if self.order not in ("C", "F"):
            raise ValueError("order is 'C' or 'F'")
        st, acc = [], 1
        for n in (self.shape if self.order == "F" else self.shape[::-1]):
            st.append(acc)
            acc *= n
        self.strides_elems = tuple(st if self.order == "F" else st[::-1])
        self.source = "file"
        self._fd, self._view, self._lock = None, None, threading.Lock()

    def fileno(self) -> int:
        with self._lock:
            if self._fd is None:
                self._fd = os.open(str(self.path), os.O_RDONLY)
            return self._fd

    def release(self) -> None:
        with self._lock:
            if self._fd is not None:
                os.close(self._fd)
                self._fd = None
            self._view = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def _mapped(self):
        if self._view is None:
            re = np.memmap(self.path, dtype=self.store, mode="r", offset=self.real_offset, shape=self.shape, order=self.order)
            if self.interleaved:
                self._view = re
            else:
                im = None if self.imag_offset is None else \
                    np.memmap(self.path, dtype=self.store, mode="r", offset=self.imag_offset, shape=self.shape, order=self.order)
                self._view = SplitComplex(re, im)
        return self._view

    def __getitem__(self, idx) -> np.ndarray:
        return np.asarray(self._mapped()[idx])


class FrameRows:
    """Frames ``[lo, hi)`` of ``parsed[:n_snr, :n_frames]`` flattened snr-major
    (frame g = snr * n_frames + k, the order feature_extraction.py:64-72 enqueues
    them in), WITHOUT materialising the flattening: for the Fortran-ordered arrays
    ``loadmat`` returns, ``reshape`` would be a full transposing copy."""

    def __init__(self, parsed, n_snr: int, n_frames: int, lo: int = 0, hi: Optional[int] = None):
        self.parsed, self.n_snr, self.n_frames = parsed, n_snr, n_frames
        self.lo = lo
        self.hi = n_snr * n_frames if hi is None else hi
        self.dtype = parsed.dtype

    @property
    def shape(self):
        return (self.hi - self.lo, self.parsed.shape[2])

    def slice(self, lo: int, hi: int) -> "FrameRows":
        return FrameRows(self.parsed, self.n_snr, self.n_frames, self.lo + lo, self.lo + hi)

    def blocks(self) -> Iterator[Tuple[int, int, int, int]]:
        """``(s0, s1, k0, k1)`` rectangles of the (snr, frame) grid that tile ``[lo, hi)`` in order:
        at most a partial first snr row, a run of whole rows, a partial last row."""
        a = self.lo
        while a < self.hi:
            s, k = divmod(a, self.n_frames)
            if k == 0 and self.hi - a >= self.n_frames:
                m = (self.hi - a) // self.n_frames
                yield s, s + m, 0, self.n_frames
                a += m * self.n_frames
            else:
                take = min(self.hi - a, self.n_frames - k)
                yield s, s + 1, k, k + take
                a += take

    def gather(self, dst: np.ndarray, g0: int, g1: int, n: int) -> None:
        """dst[(g1-g0), n] <- the first n samples of frames [g0, g1) of this range (host copy:
        tests and injected engines; the production engine never calls it)."""
        row = 0
        for s0, s1, k0, k1 in self.slice(g0, g1).blocks():
            for s in range(s0, s1):
                np.copyto(dst[row:row + k1 - k0], self.parsed[s, k0:k1, :n], casting="same_kind")
                row += k1 - k0

    def to_array(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=self.dtype)
        self.gather(out, 0, self.shape[0], self.shape[1])
        return out


class FrameColumns(FrameRows):
    """Frames ``[k_lo, k_hi)`` of EVERY snr row of ``parsed[:n_snr, :n_frames]``, snr-major (row
    ``s * (k_hi - k_lo) + (k - k_lo)``): a rank's share when a container is cut along its frame axis
    (``sharding.shard_by_frames``).  In a column-major container that is one contiguous run of every sample
    plane -- what the staging threads read from the file or copy at full rate."""

    def __init__(self, parsed, n_snr: int, n_frames: int, k_lo: int, k_hi: int):
        super().__init__(parsed, n_snr, n_frames, 0, n_snr * max(0, k_hi - k_lo))
        self.k_lo, self.k_hi = k_lo, max(k_lo, k_hi)

    def slice(self, lo: int, hi: int) -> "FrameRows":
        if (lo, hi) != (0, self.hi):
            raise NotImplementedError("a frame-axis share is taken whole")
        return self

    def blocks(self) -> Iterator[Tuple[int, int, int, int]]:
        if self.k_hi > self.k_lo and self.n_snr:
            yield 0, self.n_snr, self.k_lo, self.k_hi

    def gather(self, dst: np.ndarray, g0: int, g1: int, n: int) -> None:
        w = self.k_hi - self.k_lo
        for g in range(g0, g1):                           # host copy: tests and injected engines only
            s, k = divmod(g, w)
            np.copyto(dst[g - g0], self.parsed[s, self.k_lo + k, :n], casting="same_kind")


def _native_source(arr):
    """(keepalive, re_ptr, im_ptr, kind, element strides, bytes per element, fd) of a container the
    native engine can read in place -- pointers, or byte offsets into the file ``fd`` -- or None if it has to be
    copied first."""
    if isinstance(arr, FileComplex):
        return arr, arr.real_offset, arr.imag_offset, _kind_of(arr.store), list(arr.strides_elems), arr.store.itemsize, arr.fileno()
    if isinstance(arr, SplitComplex):
        re, im = arr.real, arr.imag
    elif isinstance(arr, np.ndarray) and _kind_of(arr.dtype) is not None:
        re, im = arr, None
    else:
        return None
    item = re.itemsize
    if any(st < 0 or st % item for st in re.strides):
        return None
    return (re, im), re.ctypes.data, (None if im is None else im.ctypes.data), _kind_of(re.dtype), [st // item for st in re.strides], item, None


def as_frame_rows(frames) -> FrameRows:
    """What a caller may hand an engine, as :class:`FrameRows`, without a copy: one passes through; an (F, L) array,
    memmap or :class:`SplitComplex` -- (F, L, 2) int16 / int8 / uint8 pairs re-viewed as ``SC16`` / ``CI8`` / ``CU8`` -- becomes
    a one-snr container."""
    if isinstance(frames, FrameRows):
        return frames
    arr = frames if isinstance(frames, SplitComplex) else np.asarray(frames)
    family = None if isinstance(arr, SplitComplex) else getattr(_formats.by_plain(arr.dtype), "family", None)
    if family is not None:                                   # (F, L, 2) integer pairs -> (F, L) stored samples, no copy
        arr = (_formats.sc16_view if family == "sc16" else _formats.iq8_view)(arr)
    if arr.ndim != 2:
        raise ValueError(f"expected (F, L) frames, got shape {arr.shape}")
    if isinstance(arr, SplitComplex):
        return FrameRows(SplitComplex(arr.real[None], None if arr.imag is None else arr.imag[None]), 1, arr.shape[0])
    return FrameRows(arr[None], 1, arr.shape[0])
