"""What the three stream operations -- the down-converter (:mod:`amcpy_amd.ddc`), the filter bank (:mod:`amcpy_amd.bank`) and
the resampler (:mod:`amcpy_amd.resample`) -- share on the host: the sample formats, the phase step, the tap design, the front
of a one-shot call and the bookkeeping of the streaming classes.  Private: the three modules are the interface."""
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


def front(x, taps, scale, shift, sample_index0, count) -> Front:
    """The checks every one-shot call opens with, in their order, and what it goes on with: the source kind and scale the C
    entry takes, the taps on x's device, the S samples, T taps and ``M = count(S, T)`` outputs (the caller's ``out_samples``,
    which refuses what is outside its kernel's limits), the phase step, and ``sample_index0`` and the phase there mod 2^64."""
    import torch

    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch tensor (complex64 (S,), or int16 / int8 / uint8 (S, 2))")
    fmt = _format_of(x)
    scale = _formats.scale_of(fmt, scale)
    if not x.is_cuda:
        raise ValueError("x must live in GPU memory")
    if not x.is_contiguous():
        raise ValueError("x must be one contiguous stream")
    if not isinstance(taps, torch.Tensor):
        taps = torch.from_numpy(np.ascontiguousarray(np.asarray(taps, dtype=np.float32))).to(x.device)
    if taps.dtype != torch.float32 or taps.dim() != 1 or taps.device != x.device:
        raise TypeError("taps must be a one-dimensional float32 tensor on x's device")
    taps = taps.contiguous()
    S, T = int(x.shape[0]), int(taps.shape[0])
    M = count(S, T)
    step = phase_step_of(shift)
    index0 = int(sample_index0) & _MASK64
    return Front(_formats.get(fmt).kind, scale, taps, S, T, M, step, index0, (index0 * step) & _MASK64)


def launch(x, call) -> None:
    """``call(lib, stream)`` -- one C entry -- on x's device and the current torch stream there; its status checked."""
    import torch

    _lib.require_torch_runtime()
    lib = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(call(lib, torch.cuda.current_stream(x.device).cuda_stream))


class Stream:
    """The bookkeeping of a streaming class: the unconsumed tail of the input, the absolute index of the sample the next
    output's window begins at, and -- where that lies ahead of the data -- how many samples are still to be dropped.

    A subclass names its shape (``__init__``'s keywords, kept as int attributes) and supplies ``_NOUN``, ``_one_shot``,
    ``_limits()``, ``_args()``, ``_outputs(S)`` and ``_consumed(M)``."""

    def __init__(self, taps, shift, fmt, scale, compute, **shape):
        if fmt not in FORMATS:
            raise ValueError(f"fmt must be one of {FORMATS}, not {fmt!r}")
        self.taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float32))
        if self.taps.ndim != 1:
            raise ValueError("taps must be one-dimensional")
        for name, value in shape.items():
            setattr(self, name, int(value))
        self.shift, self.fmt = shift, fmt
        self._limits()                 # ValueError outside the kernel's
        phase_step_of(shift)
        self.scale = _formats.scale_of(fmt, scale)
        self.index = 0                 # absolute index of the sample the next output's window begins at
        self._tail = None              # the samples from there on that have arrived ...
        self._skip = 0                 # ... or, the next window beginning beyond them, how many are still to be dropped before it
        self._compute = compute
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

    def push(self, chunk):
        """The new outputs (complex64, possibly none) of the stream extended by ``chunk``."""
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
