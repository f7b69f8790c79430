"""The digital down-converter: tune, low-pass and decimate samples where they lie (amcx_tune_decimate, include/amcx.h ABI 11).

A receiver records a band several times wider than the emitter, and the emitter sits off centre; the 18 features want it at
0 Hz and filling its band.  :func:`tune_decimate` is one launch over a resident stream -- complex64, or the raw sc16 / ci8 /
cu8 a recording holds -- that mixes, filters with real taps and keeps every ``decim``-th output, packed complex64:

    phi(n) = (phase0 + n * phase_step) mod 2^64       phase_step = round(shift * 2^64) mod 2^64, shift in cycles per sample
    v[n]   = x[n] * exp(+2 pi j phi(n) / 2^64)
    y[m]   = sum_k taps[k] * v[m * decim + T - 1 - k]  = numpy.convolve(v, taps, "valid")[::decim]

:func:`design_lowpass` makes the taps on the host, :class:`Channelizer` is the streaming form.  The bits of an output depend
only on its T input samples, the taps and the phase there, so a stream pushed in chunks equals one call over the whole.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import _lib

MAX_TAPS, MAX_DECIM = 2048, 4096
FORMATS = ("cf32", "sc16", "ci8", "cu8")
_KINDS = {"cf32": _lib.SRC_C64, "sc16": _lib.SRC_SC16, "ci8": _lib.SRC_CI8, "cu8": _lib.SRC_CU8}
_DEFAULT_SCALE = {"cf32": 1.0, "sc16": _lib.SC16_SCALE, "ci8": _lib.IQ8_SCALE, "cu8": _lib.IQ8_SCALE}
_NUMPY = {"cf32": np.complex64, "sc16": np.int16, "ci8": np.int8, "cu8": np.uint8}
_MASK64 = (1 << 64) - 1


def phase_step_of(shift) -> int:
    """``round(shift * 2^64) mod 2^64`` in Python integers.  ``shift``: cycles per input sample, a float (taken at its
    exact value) or a ``fractions.Fraction`` -- ``Fraction(k, 2**64)`` is the step k itself.  To move a signal at +f Hz
    to 0 Hz: ``shift = -f / fs``."""
    if isinstance(shift, float) and not np.isfinite(shift):
        raise ValueError(f"shift must be finite, got {shift!r}")
    return int(round(Fraction(shift) * (1 << 64))) & _MASK64


def out_samples(n_samples: int, n_taps: int, decim: int) -> int:
    """M of a call over ``n_samples`` inputs: 0 below ``n_taps``, else ``(n_samples - n_taps) // decim + 1``.  ValueError
    outside 1 <= n_taps <= 2048, 1 <= decim <= 4096, 0 <= n_samples < 2^40 (the limits of amcx_tune_decimate)."""
    S, T, D = int(n_samples), int(n_taps), int(decim)
    if not (1 <= T <= MAX_TAPS and 1 <= D <= MAX_DECIM and 0 <= S < 1 << 40):
        raise ValueError(f"outside the down-converter's limits: n_samples {S}, n_taps {T}, decim {D}")
    return 0 if S < T else (S - T) // D + 1


def design_lowpass(decim: int, n_taps=None, cutoff=None) -> np.ndarray:
    """A Hamming-windowed sinc for a decimation by ``decim``: float32 taps, symmetric, unit DC gain.

    n_taps : default ``16 * decim + 1``.
    cutoff : the -6 dB edge in cycles per INPUT sample, default 0.8 of the output Nyquist, ``0.4 / decim``.
    Computed in float64, normalised to a DC gain of 1 and then rounded to float32."""
    D = int(decim)
    T = 16 * D + 1 if n_taps is None else int(n_taps)
    if not (1 <= D <= MAX_DECIM and 1 <= T <= MAX_TAPS):
        raise ValueError(f"design_lowpass: decim {D} with {T} taps is outside 1 ... {MAX_DECIM} / 1 ... {MAX_TAPS}")
    fc = 0.4 / D if cutoff is None else float(cutoff)
    if not 0.0 < fc <= 0.5:
        raise ValueError(f"cutoff must lie in (0, 0.5] cycles per sample, got {cutoff!r}")
    n = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
    h = 2.0 * fc * np.sinc(2.0 * fc * n)
    if T > 1:
        h *= 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(T, dtype=np.float64) / (T - 1))
    h = (h + h[::-1]) / 2.0                                   # symmetric to the bit
    return (h / h.sum()).astype(np.float32)


def _format_of(x) -> str:
    """The sample format a tensor's or array's dtype and shape name: complex64 (S,), or int16 / int8 / uint8 (S, 2)."""
    name = str(x.dtype).replace("torch.", "")
    if name == "complex64":
        if x.ndim != 1:
            raise TypeError("complex64 samples must have shape (S,)")
        return "cf32"
    fmt = {"int16": "sc16", "int8": "ci8", "uint8": "cu8"}.get(name)
    if fmt is None:
        raise TypeError(f"samples must be complex64 (S,) or int16 / int8 / uint8 (S, 2), not {name}")
    if x.ndim != 2 or x.shape[1] != 2:
        raise TypeError(f"{name} samples must have shape (S, 2): the last dimension is (I, Q)")
    return fmt


def _scale_of(fmt: str, scale) -> float:
    from .features import _sc16_scale
    return _DEFAULT_SCALE[fmt] if scale is None or fmt == "cf32" else _sc16_scale(scale)


def tune_decimate(x, taps, decim: int, *, shift=0.0, sample_index0: int = 0, scale=None, out=None):
    """Mix, filter and decimate a stream in GPU memory: one launch of amcx_tune_decimate on the current torch stream.

    x     : torch tensor on a GPU, contiguous: complex64 (S,), or int16 (sc16) / int8 (ci8) / uint8 (cu8: zero level 128) of
            shape (S, 2), I then Q.  The dtype picks the format; a sample's value is what :func:`features18_sc16` /
            :func:`features18_iq8` define, ``float32(i) * scale``.
    taps  : T real taps, 1 <= T <= 2048: a float32 tensor on the same device, or anything ``numpy.asarray`` takes.
    decim : 1 ... 4096.
    shift : cycles per input sample (float or Fraction, :func:`phase_step_of`); a signal at +f Hz goes to 0 with -f / fs.
    sample_index0 : the index of x[0] in the stream this call continues: ``phase0 = sample_index0 * phase_step mod 2^64``.
    scale : integer formats only, default 2^-15 / 2^-7.
    out   : optional complex64 tensor with room for the M outputs.
    Returns complex64 (M,), M = :func:`out_samples`."""
    import torch

    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch tensor (complex64 (S,), or int16 / int8 / uint8 (S, 2))")
    fmt = _format_of(x)
    scale = _scale_of(fmt, scale)
    if not x.is_cuda:
        raise ValueError("x must live in GPU memory")
    if not x.is_contiguous():
        raise ValueError("x must be one contiguous stream")
    if not isinstance(taps, torch.Tensor):
        taps = torch.from_numpy(np.ascontiguousarray(np.asarray(taps, dtype=np.float32))).to(x.device)
    if taps.dtype != torch.float32 or taps.dim() != 1 or taps.device != x.device:
        raise TypeError("taps must be a one-dimensional float32 tensor on x's device")
    taps = taps.contiguous()
    S, T, D = int(x.shape[0]), int(taps.shape[0]), int(decim)
    M = out_samples(S, T, D)
    step = phase_step_of(shift)
    phase0 = (int(sample_index0) * step) & _MASK64
    if out is None:
        out = torch.empty((M,), dtype=torch.complex64, device=x.device)
    elif out.dtype != torch.complex64 or out.device != x.device or out.dim() != 1 or not out.is_contiguous() or out.shape[0] < M:
        raise ValueError(f"out must be a contiguous complex64 tensor of at least {M} samples on x's device")
    _lib.require_torch_runtime()
    lib = _lib.load()
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(lib.amcx_tune_decimate(x.data_ptr() if S else None, _KINDS[fmt], S, scale, phase0, step, taps.data_ptr(), T, D,
                                          out.data_ptr() if M else None, int(out.shape[0]), stream))
    return out[:M]


class Channelizer:
    """The streaming form of :func:`tune_decimate`: ``push(chunk)`` returns the outputs the stream so far completes.

    Keeps the unconsumed tail of the input (fewer than ``T - 1 + decim`` samples) and the absolute index of the sample the
    next window begins at (with ``decim > T`` that may lie ahead of the data: the samples up to it are dropped); every call advances the phase accordingly, so the concatenated results equal ONE call over the whole stream
    bit for bit, however it is cut.  ``fmt``: "cf32", "sc16", "ci8" or "cu8" -- what every chunk must be.  ``compute``:
    an injected ``f(x, taps, decim, shift=..., sample_index0=..., scale=...)`` over numpy chunks (tests); the default is
    :func:`tune_decimate` over GPU tensors, with the taps uploaded once."""

    def __init__(self, taps, decim: int, shift=0.0, fmt: str = "cf32", scale=None, *, compute=None):
        if fmt not in FORMATS:
            raise ValueError(f"fmt must be one of {FORMATS}, not {fmt!r}")
        self.taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float32))
        if self.taps.ndim != 1:
            raise ValueError("taps must be one-dimensional")
        self.decim, self.shift, self.fmt = int(decim), shift, fmt
        out_samples(0, self.taps.shape[0], self.decim)                  # the limits
        phase_step_of(shift)
        self.scale = _scale_of(fmt, scale)
        self.index = 0                 # absolute index of the sample the next output's window begins at
        self._tail = None              # the samples from there on that have arrived ...
        self._skip = 0                 # ... or, decim > T, how many are still to be dropped before it
        self._compute = compute
        self._taps_dev = None

    def _run(self, buf):
        if self._compute is not None:
            return self._compute(buf, self.taps, self.decim, shift=self.shift, sample_index0=self.index, scale=self.scale)
        import torch
        if self._taps_dev is None or self._taps_dev.device != buf.device:
            self._taps_dev = torch.from_numpy(self.taps).to(buf.device)
        return tune_decimate(buf, self._taps_dev, self.decim, shift=self.shift, sample_index0=self.index, scale=self.scale)

    def push(self, chunk):
        """The new outputs (complex64, possibly none) of the stream extended by ``chunk``."""
        if _format_of(chunk) != self.fmt:
            raise TypeError(f"this channelizer takes {self.fmt} chunks")
        if self._skip:                                               # decim > T: samples between two windows, never read
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
        y = self._run(buf)
        used = out_samples(S, self.taps.shape[0], self.decim) * self.decim      # where the next output's window begins
        self._skip += max(0, used - S)                               # (a skip still pending left buf empty: used == 0)
        tail = buf[min(used, S):]                                    # short: a copy, not a view that keeps the chunk alive
        self._tail = tail.copy() if isinstance(tail, np.ndarray) else tail.clone()
        self.index += used
        return y
