"""The polyphase analysis filter bank: every channel of a raster from one pass (amcx_filter_bank, include/amcx.h ABI 12).

A wideband recording holds many emitters on a channel raster.  :func:`amcpy_amd.ddc.tune_decimate` tunes to one of them per
pass; :func:`filter_bank` is one launch that gives all ``C`` channels, packed complex64 ``(C, M)``:

    phi(n)  = (phase0 + n * phase_step) mod 2^64        phase_step = round(shift * 2^64) mod 2^64, shift in cycles per sample
    v[n]    = x[n] * exp(+2 pi j phi(n) / 2^64)
    y[c,m]  = sum_k taps[k] * v[n_m - k] * exp(-2 pi j c ((sample_index0 + n_m - k) mod C) / C),   n_m = m * decim + T - 1

Channel c is centred at +c / C cycles per sample of the pre-mixed stream (FFT order: c > C / 2 are negative frequencies) and
equals ``tune_decimate`` with ``shift - c / C``.  :func:`design_bank_lowpass` makes the prototype filter,
:func:`channel_frequencies` names the channels, :class:`FilterBank` is the streaming form.  The bits of an output depend only
on its T input samples, the taps, the phase there and the absolute sample index mod C, so a stream pushed in chunks equals one
call over the whole.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import _stream

MAX_TAPS, MAX_CHANNELS = 4096, 256


def _check_shape(n_taps: int, channels: int, decim: int) -> None:
    T, C, D = int(n_taps), int(channels), int(decim)
    if not (2 <= C <= MAX_CHANNELS and C & (C - 1) == 0 and 1 <= T <= MAX_TAPS and 1 <= D <= C):
        raise ValueError(f"outside the filter bank's limits: channels {C} (a power of two, 2 ... {MAX_CHANNELS}), "
                         f"n_taps {T} (1 ... {MAX_TAPS}), decim {D} (1 ... channels)")


def out_samples(n_samples: int, n_taps: int, channels: int, decim: int) -> int:
    """M of a call over ``n_samples`` inputs: 0 below ``n_taps``, else ``(n_samples - n_taps) // decim + 1``.  ValueError
    outside the limits of amcx_filter_bank."""
    _check_shape(n_taps, channels, decim)
    S = int(n_samples)
    if not 0 <= S < 1 << 40:
        raise ValueError(f"outside the filter bank's limits: n_samples {S}")
    return 0 if S < int(n_taps) else (S - int(n_taps)) // int(decim) + 1


def design_bank_lowpass(channels: int, taps_per_channel: int = 16, decim=None) -> np.ndarray:
    """The prototype low-pass of a bank of ``channels``: ``channels * taps_per_channel`` float32 taps, a Hamming-windowed sinc
    with its -6 dB edge at half the channel spacing, ``0.5 / channels`` cycles per sample; symmetric, unit DC gain.  Computed
    in float64, normalised and then rounded.  ``decim`` (default ``channels``) is only checked: the prototype depends on the
    raster, not on the output rate."""
    C, P = int(channels), int(taps_per_channel)
    if P < 1:
        raise ValueError(f"taps_per_channel must be at least 1, got {taps_per_channel!r}")
    T = C * P
    _check_shape(T, C, C if decim is None else decim)
    return _stream.windowed_sinc(T, 0.5 / C)


def channel_frequencies(channels: int, sample_rate: float = 1.0, center: float = 0.0, shift=0.0) -> np.ndarray:
    """The input frequency at the centre of every channel, float64 ``(C,)`` in the bank's (FFT) order.  ``shift``: what
    :func:`filter_bank` is given, in cycles per sample -- the pre-mixer moves the input up by it, so channel c holds what was
    at ``c / C - shift``, taken into [-0.5, 0.5) cycles per sample; times ``sample_rate``, plus ``center``."""
    C = int(channels)
    _check_shape(1, C, 1)
    f = [Fraction(c, C) - Fraction(shift) for c in range(C)]
    f = [float(v - (v + Fraction(1, 2)).__floor__()) for v in f]
    return float(center) + float(sample_rate) * np.array(f, dtype=np.float64)


def filter_bank(x, taps, channels: int, decim: int, *, shift=0.0, sample_index0: int = 0, scale=None, out=None):
    """All ``channels`` channels of a stream in GPU memory: one launch of amcx_filter_bank on the current torch stream.

    x     : as :func:`amcpy_amd.ddc.tune_decimate` takes it: complex64 (S,), or int16 / int8 / uint8 (S, 2).
    taps  : T real taps, 1 <= T <= 4096: a float32 tensor on the same device, or anything ``numpy.asarray`` takes.
    channels : C, a power of two 2 ... 256.  decim : 1 ... C (C: critically sampled, C / 2: 2x oversampled).
    shift : the pre-mixer, cycles per input sample (float or Fraction); it offsets the whole raster.
    sample_index0 : the absolute index of x[0] in the stream: it sets the mixer's phase and the channels' phases.
    out   : optional complex64 (C, >= M) tensor, rows contiguous.
    Returns complex64 (C, M), M = :func:`out_samples`."""
    import torch

    f = _stream.front(x, taps, scale, shift, sample_index0, lambda S, T: out_samples(S, T, channels, decim))
    C, D, M = int(channels), int(decim), f.M
    if out is None:
        out = torch.empty((C, M), dtype=torch.complex64, device=x.device)
    elif (out.dtype != torch.complex64 or out.device != x.device or out.dim() != 2 or out.shape[0] != C or out.shape[1] < M
          or (out.shape[1] > 1 and out.stride(1) != 1) or out.stride(0) < out.shape[1]):
        raise ValueError(f"out must be a complex64 ({C}, >= {M}) tensor on x's device with contiguous rows")
    stride = int(out.stride(0)) if C > 1 and out.shape[1] > 0 else M
    _stream.launch(x, lambda lib, stream: lib.amcx_filter_bank(
        x.data_ptr() if f.S else None, f.kind, f.S, f.scale, f.phase0, f.step, f.index0, f.taps.data_ptr(), f.T, C, D,
        out.data_ptr() if M else None, stride, (C - 1) * stride + M, stream))
    return out[:, :M]


class FilterBank(_stream.Stream):
    """The streaming form of :func:`filter_bank`: ``push(chunk)`` returns the ``(C, new)`` outputs the stream so far completes.

    Keeps the unconsumed tail of the input and the absolute index of the sample the next window begins at, as
    :class:`amcpy_amd.ddc.Channelizer` does (with ``decim > T`` that index may lie ahead of the data: the samples up to it are
    dropped); every call passes that index on, so the results, concatenated along the second axis, equal ONE call over the
    whole stream bit for bit, however it is cut.  ``compute``: an injected ``f(x, taps, channels, decim, shift=...,
    sample_index0=..., scale=...)`` over numpy chunks (tests); the default is :func:`filter_bank` over GPU tensors, with the
    taps uploaded once."""

    _NOUN, _one_shot = "filter bank", staticmethod(filter_bank)

    def __init__(self, taps, channels: int, decim: int, shift=0.0, fmt: str = "cf32", scale=None, *, compute=None):
        super().__init__(taps, shift, fmt, scale, compute, channels=channels, decim=decim)

    def _limits(self):
        _check_shape(self.taps.shape[0], self.channels, self.decim)

    def _args(self):
        return self.channels, self.decim

    def _outputs(self, S):
        return out_samples(S, self.taps.shape[0], self.channels, self.decim)

    def _consumed(self, M):
        return M * self.decim
