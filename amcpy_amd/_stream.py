"""What the stream operations -- the down-converter (:mod:`amcpy_amd.ddc`), the filter bank (:mod:`amcpy_amd.bank`), the
resampler (:mod:`amcpy_amd.resample`) and the spectrogram (:mod:`amcpy_amd.psd`) -- share on the host: the sample formats, the
phase step, the tap design, the front of a one-shot call, the check of a matrix of rows (:mod:`amcpy_amd.occupancy` too) and
the bookkeeping of the streaming classes.  Private: those modules are the interface."""
from __future__ import annotations

from collections import namedtuple
from fractions import Fraction

import numpy as np

from . import _formats, _lib

FORMATS = _formats.NAMES
_MASK64 = (1 << 64) - 1


def phase_step_of(shift) -> int:
    """``round(shift * 2^64) mod 2^64`` in Python integers.  ``shift``: cycles per input sample, a float (taken at its
    exact value) or a ``fractions.Fraction`` -- ``Fraction(k, 2**64)`` is the step k itself.  To move a signal at +f Hz
    to 0 Hz: ``shift = -f / fs``."""
    if isinstance(shift, float) and not np.isfinite(shift):
        raise ValueError(f"shift must be finite, got {shift!r}")
    return int(round(Fraction(shift) * (1 << 64))) & _MASK64


def _format_of(x) -> str:
    """The sample format a tensor's or array's dtype and shape name: complex64 (S,), or int16 / int8 / uint8 (S, 2)."""
    fmt = _formats.by_plain(x.dtype)
    if fmt is None:
        name = str(x.dtype).replace("torch.", "")
        raise TypeError(f"samples must be complex64 (S,) or int16 / int8 / uint8 (S, 2), not {name}")
    if x.ndim < 1 or tuple(x.shape[1:]) != fmt.tail:
        raise TypeError("complex64 samples must have shape (S,)" if not fmt.tail else
                        f"{fmt.plain.name} samples must have shape (S, 2): the last dimension is (I, Q)")
    return fmt.name


def windowed_sinc(n_taps: int, cutoff: float, gain=1) -> np.ndarray:
    """``n_taps`` float32 taps of a Hamming-windowed sinc with its -6 dB edge at ``cutoff`` cycles per sample: symmetric to
    the bit, computed in float64, normalised to a DC gain of ``gain`` and then rounded."""
    T, fc = n_taps, cutoff
    n = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
    h = 2.0 * fc * np.sinc(2.0 * fc * n)
    if T > 1:
        h *= 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(T, dtype=np.float64) / (T - 1))
    h = (h + h[::-1]) / 2.0                                   # symmetric to the bit
    return (h / h.sum() * gain).astype(np.float32)            # (times 1 changes no bit)


Front = namedtuple("Front", "kind scale taps S T M step index0 phase0")


def source(x, scale) -> tuple:
    """The checks every one-shot call opens with on its samples, in their order -> the format's name, the source kind the C
    entry takes, the scale and the S samples."""
    import torch

    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch tensor (complex64 (S,), or int16 / int8 / uint8 (S, 2))")
    fmt = _format_of(x)
    scale = _formats.scale_of(fmt, scale)
    if not x.is_cuda:
        raise ValueError("x must live in GPU memory")
    if not x.is_contiguous():
        raise ValueError("x must be one contiguous stream")
    return fmt, _formats.get(fmt).kind, scale, int(x.shape[0])


def front(x, taps, scale, shift, sample_index0, count) -> Front:
    """What a one-shot call of a tap filter opens with: :func:`source`'s checks, then the taps on x's device, the S samples, T
    taps and ``M = count(S, T)`` outputs (the caller's ``out_samples``, which refuses what is outside its kernel's limits), the
    phase step, and ``sample_index0`` and the phase there mod 2^64."""
    import torch

    _, kind, scale, S = source(x, scale)
    if not isinstance(taps, torch.Tensor):
        taps = torch.from_numpy(np.ascontiguousarray(np.asarray(taps, dtype=np.float32))).to(x.device)
    if taps.dtype != torch.float32 or taps.dim() != 1 or taps.device != x.device:
        raise TypeError("taps must be a one-dimensional float32 tensor on x's device")
    taps = taps.contiguous()
    T = int(taps.shape[0])
    M = count(S, T)
    step = phase_step_of(shift)
    index0 = int(sample_index0) & _MASK64
    return Front(kind, scale, taps, S, T, M, step, index0, (index0 * step) & _MASK64)


def rows_of(t, dtype, name, cols, min_cols, max_cols=None, *, narrow, used=None, min_rows=0, device=None, kind=None,
            layout=None) -> tuple:
    """``t`` as a matrix of rows in GPU memory -> ``(R, n, row stride)``: a two-dimensional torch tensor of ``dtype`` (on
    ``device``, where given) with ``min_rows`` rows or more of ``min_cols ... max_cols`` elements, each row contiguous, at a row
    stride that holds the ``used`` elements of a row the kernel touches (all n of them unless given).  One row, or none, has
    no stride of its own: n.  ``name`` and ``cols`` (what the caller calls n) word the messages; ``kind``, ``narrow`` (which
    takes n) and ``layout`` are the caller's own TypeError, shape and layout texts."""
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 2 or (device is not None and t.device != device):
        raise TypeError(kind or f"{name} must be a {str(dtype).replace('torch.', '')} (R, {cols}) torch tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must live in GPU memory")
    R, n = int(t.shape[0]), int(t.shape[1])
    if R < min_rows or n < min_cols or (max_cols is not None and n > max_cols):
        raise ValueError(narrow.format(n))
    if t.stride(1) != 1 or (R > 1 and t.stride(0) < (n if used is None else used)):
        raise ValueError(layout or f"{name} must have contiguous rows at a row stride >= {cols}")
    return R, n, int(t.stride(0)) if R > 1 else n


def launch(x, call) -> None:
    """``call(lib, stream)`` -- one C entry -- on x's device and the current torch stream there; its status checked."""
    import torch

    _lib.require_torch_runtime()
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(call(lib, torch.cuda.current_stream(x.device).cuda_stream))


class Chunked:
    """The bookkeeping of a streaming class: the unconsumed tail of the input, the absolute index of the sample the next
    output's window begins at, and -- where that lies ahead of the data -- how many samples are still to be dropped.

    A subclass supplies ``_NOUN``, ``_outputs(S)`` (the outputs S samples complete), ``_run(buf, M)`` (those M outputs; over
    numpy with the injected ``self._compute``) and ``_consumed(M)`` (the samples M outputs move the next window on by)."""

    def __init__(self, fmt, compute):
        if fmt not in FORMATS:
            raise ValueError(f"fmt must be one of {FORMATS}, not {fmt!r}")
        self.fmt = fmt
        self.index = 0                 # absolute index of the sample the next output's window begins at
        self._tail = None              # the samples from there on that have arrived ...
        self._skip = 0                 # ... or, the next window beginning beyond them, how many are still to be dropped before it
        self._compute = compute

    def push(self, chunk):
        """The new outputs (possibly none) of the stream extended by ``chunk``."""
        if _format_of(chunk) != self.fmt:
            raise TypeError(f"this {self._NOUN} takes {self.fmt} chunks")
        if self._skip:                                               # samples between two windows, never read
            drop = min(self._skip, int(chunk.shape[0]))
            chunk, self._skip = chunk[drop:], self._skip - drop
        if self._tail is None or self._tail.shape[0] == 0:
            buf = chunk
        elif chunk.shape[0] == 0:
            buf = self._tail
        elif isinstance(chunk, np.ndarray):
            buf = np.concatenate([self._tail, chunk])
        else:
            import torch
            buf = torch.cat([self._tail, chunk])
        S = int(buf.shape[0])
        M = self._outputs(S)
        y = self._run(buf, M)
        used = self._consumed(M)                                     # where the next output's window begins
        self._skip += max(0, used - S)                               # (a skip still pending left buf empty: used == 0)
        tail = buf[min(used, S):]                                    # short: a copy, not a view that keeps the chunk alive
        self._tail = tail.copy() if isinstance(tail, np.ndarray) else tail.clone()
        self.index += used
        return y


class Stream(Chunked):
    """A streaming tap filter: :class:`Chunked` with the taps, uploaded once per device, and the frequency shift.

    A subclass names its shape (``__init__``'s keywords, kept as int attributes) and supplies ``_NOUN``, ``_one_shot``,
    ``_limits()``, ``_args()``, ``_outputs(S)`` and ``_consumed(M)``."""

    def __init__(self, taps, shift, fmt, scale, compute, **shape):
        super().__init__(fmt, compute)
        self.taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float32))
        if self.taps.ndim != 1:
            raise ValueError("taps must be one-dimensional")
        for name, value in shape.items():
            setattr(self, name, int(value))
        self.shift = shift
        self._limits()                 # ValueError outside the kernel's
        phase_step_of(shift)
        self.scale = _formats.scale_of(fmt, scale)
        self._taps_dev = None

    def _kw(self) -> dict:
        return dict(shift=self.shift, sample_index0=self.index, scale=self.scale)

    def _run(self, buf, M):
        """The M outputs ``buf`` completes: the injected ``compute`` over numpy, or the one-shot call with the taps uploaded once."""
        if self._compute is not None:
            return self._compute(buf, self.taps, *self._args(), **self._kw())
        import torch
        if self._taps_dev is None or self._taps_dev.device != buf.device:
            self._taps_dev = torch.from_numpy(self.taps).to(buf.device)
        return self._one_shot(buf, self._taps_dev, *self._args(), **self._kw())
