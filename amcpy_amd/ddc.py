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

import numpy as np

from . import _stream
from ._formats import _DEFAULT_SCALE, _KINDS, _NUMPY, scale_of as _scale_of  # noqa: F401
from ._stream import FORMATS, _MASK64, _format_of, phase_step_of  # noqa: F401

MAX_TAPS, MAX_DECIM = 2048, 4096


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
    return _stream.windowed_sinc(T, fc)


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

    f = _stream.front(x, taps, scale, shift, sample_index0, lambda S, T: out_samples(S, T, decim))
    D = int(decim)
    if out is None:
        out = torch.empty((f.M,), dtype=torch.complex64, device=x.device)
    elif out.dtype != torch.complex64 or out.device != x.device or out.dim() != 1 or not out.is_contiguous() or out.shape[0] < f.M:
        raise ValueError(f"out must be a contiguous complex64 tensor of at least {f.M} samples on x's device")
    _stream.launch(x, lambda lib, stream: lib.amcx_tune_decimate(
        x.data_ptr() if f.S else None, f.kind, f.S, f.scale, f.phase0, f.step, f.taps.data_ptr(), f.T, D,
        out.data_ptr() if f.M else None, int(out.shape[0]), stream))
    return out[:f.M]


class Channelizer(_stream.Stream):
    """The streaming form of :func:`tune_decimate`: ``push(chunk)`` returns the outputs the stream so far completes.

    Keeps the unconsumed tail of the input (fewer than ``T - 1 + decim`` samples) and the absolute index of the sample the
    next window begins at (with ``decim > T`` that may lie ahead of the data: the samples up to it are dropped); every call advances the phase accordingly, so the concatenated results equal ONE call over the whole stream
    bit for bit, however it is cut.  ``fmt``: "cf32", "sc16", "ci8" or "cu8" -- what every chunk must be.  ``compute``:
    an injected ``f(x, taps, decim, shift=..., sample_index0=..., scale=...)`` over numpy chunks (tests); the default is
    :func:`tune_decimate` over GPU tensors, with the taps uploaded once."""

    _NOUN, _one_shot = "channelizer", staticmethod(tune_decimate)

    def __init__(self, taps, decim: int, shift=0.0, fmt: str = "cf32", scale=None, *, compute=None):
        super().__init__(taps, shift, fmt, scale, compute, decim=decim)

    def _limits(self):
        out_samples(0, self.taps.shape[0], self.decim)

    def _args(self):
        return (self.decim,)

    def _outputs(self, S):
        return out_samples(S, self.taps.shape[0], self.decim)

    def _consumed(self, M):
        return M * self.decim
