"""The rational resampler: tune, low-pass and change the sample rate by L / D where samples lie (amcx_resample, include/amcx.h
ABI 13).

The down-converter (:mod:`amcpy_amd.ddc`) changes the rate by an integer only, so an emitter comes out anywhere between r and
2 r times oversampled -- and the 18 features change with that ratio.  :func:`resample` is one launch over a resident stream
(complex64, or the raw sc16 / ci8 / cu8 a recording holds) that mixes, filters with real taps GIVEN AT THE UPSAMPLED RATE and
delivers L outputs for every D inputs, packed complex64.  With T taps, L = interp, D = decim, tau0 = phase_index0:

    phi(n) = (phase0 + n * phase_step) mod 2^64         phase_step = round(shift * 2^64) mod 2^64, shift in cycles per INPUT sample
    v[n]   = x[n] * exp(+2 pi j phi(n) / 2^64)
    P      = ceil(T / L)
    t_m    = m D + tau0,   p_m = t_m mod L,   n_m = (P - 1) + t_m // L
    y[m]   = sum_{q >= 0, p_m + q L < T} taps[p_m + q L] * v[n_m - q]

i.e. ``numpy.convolve(zero_stuff(v, L), taps)[(P - 1) L + tau0 :: D]`` as far as whole windows reach.  No gain is applied:
:func:`design_resample_lowpass` returns taps with DC gain L, which keeps a signal's amplitude.  :func:`rational_ratio` finds
L / D for a wanted rate, :class:`Resampler` is the streaming form.  The bits of an output depend only on its samples, the taps,
the phase there and p_m, so a stream pushed in chunks equals one call over the whole.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import _stream

MAX_TAPS, MAX_INTERP, MAX_DECIM = 4096, 256, 4096
DESIGN_MAX = (MAX_TAPS - 1) // 16      # 255: the largest interp or decim whose default design, 16 max(L, D) + 1 taps, fits MAX_TAPS


def out_samples(n_samples: int, n_taps: int, interp: int, decim: int, phase_index0: int = 0) -> int:
    """M of a call over ``n_samples`` inputs: the outputs m whose newest sample ``n_m = (P - 1) + (m D + tau0) // L`` exists.
    ValueError outside 1 <= n_taps <= 4096, 1 <= interp <= 256, 1 <= decim <= 4096, 0 <= n_samples < 2^40,
    0 <= phase_index0 < interp (the limits of amcx_resample)."""
    S, T, L, D, tau0 = int(n_samples), int(n_taps), int(interp), int(decim), int(phase_index0)
    if not (1 <= T <= MAX_TAPS and 1 <= L <= MAX_INTERP and 1 <= D <= MAX_DECIM and 0 <= S < 1 << 40 and 0 <= tau0 < L):
        raise ValueError(f"outside the resampler's limits: n_samples {S}, n_taps {T}, interp {L}, decim {D}, phase_index0 {tau0}")
    P = -(-T // L)
    last = (S - P + 1) * L - 1 - tau0                      # the largest m D the data reaches
    return 0 if S < P or last < 0 else last // D + 1


def design_resample_lowpass(interp: int, decim: int, n_taps=None, cutoff=None) -> np.ndarray:
    """A Hamming-windowed sinc for a rate change by ``interp / decim``: float32 taps at the upsampled rate, symmetric,
    DC gain ``interp`` (every phase then sums to about 1: the output keeps the input's amplitude).

    n_taps : default ``16 * max(interp, decim) + 1`` -- 16 taps per phase or per decimated sample, whichever is more;
             ValueError above 4096, so the default exists up to ``max(interp, decim) = 255`` (``DESIGN_MAX``): search a
             ratio with ``rational_ratio(ratio, 255, 255)``, or give a count beyond that (fewer taps per phase).
    cutoff : the -6 dB edge in cycles per UPSAMPLED sample, default ``0.4 / max(interp, decim)``: 0.8 of the narrower of
             the input's and the output's Nyquist.
    Computed in float64, normalised to a DC gain of ``interp`` and then rounded to float32."""
    L, D = int(interp), int(decim)
    if not (1 <= L <= MAX_INTERP and 1 <= D <= MAX_DECIM):
        raise ValueError(f"design_resample_lowpass: interp {L} / decim {D} is outside 1 ... {MAX_INTERP} / 1 ... {MAX_DECIM}")
    T = 16 * max(L, D) + 1 if n_taps is None else int(n_taps)
    if not 1 <= T <= MAX_TAPS:
        raise ValueError(f"design_resample_lowpass: {T} taps for {L} / {D} is outside 1 ... {MAX_TAPS}"
                         + (f" (the default, 16 max(L, D) + 1, exists up to {DESIGN_MAX}: rational_ratio(ratio, {DESIGN_MAX}, "
                            f"{DESIGN_MAX}), or pass n_taps)" if n_taps is None else ""))
    fc = 0.4 / max(L, D) if cutoff is None else float(cutoff)
    if not 0.0 < fc <= 0.5:
        raise ValueError(f"cutoff must lie in (0, 0.5] cycles per upsampled sample, got {cutoff!r}")
    return _stream.windowed_sinc(T, fc, gain=L)


def rational_ratio(ratio, max_interp: int = MAX_INTERP, max_decim: int = MAX_DECIM) -> tuple:
    """``(L, D)``: the fraction L / D in lowest terms, 1 <= L <= max_interp, 1 <= D <= max_decim, closest to ``ratio`` --
    output rate over input rate, a float (taken at its exact value), an int or a ``Fraction``.  Exact ``Fraction``
    arithmetic throughout; of two equally close fractions the one with the smaller L.  The defaults are the kernel's limits;
    ``design_resample_lowpass``'s default taps exist only up to 255 either way (``DESIGN_MAX``): pass 255, 255 for those.  ValueError when there is none: a ratio
    that is not finite and positive, or one outside ``[1 / max_decim, max_interp]``, which no L / D within the limits spans."""
    if isinstance(ratio, float) and not np.isfinite(ratio):
        raise ValueError(f"ratio must be finite, got {ratio!r}")
    r = Fraction(ratio)
    Lmax, Dmax = int(max_interp), int(max_decim)
    if Lmax < 1 or Dmax < 1:
        raise ValueError("max_interp and max_decim must be at least 1")
    if r <= 0 or r < Fraction(1, Dmax) or r > Lmax:
        raise ValueError(f"no L / D with L <= {Lmax}, D <= {Dmax} spans the ratio {ratio!r}")
    best = None
    for L in range(1, Lmax + 1):
        d = L / r                                           # the exact D; its two neighbours are the candidates
        for D in sorted({max(1, min(Dmax, d.numerator // d.denominator)), max(1, min(Dmax, -(-d.numerator // d.denominator)))}):
            err = abs(Fraction(L, D) - r)
            if best is None or err < best[0]:
                best = (err, Fraction(L, D))
    return best[1].numerator, best[1].denominator


def resample(x, taps, interp: int, decim: int, *, shift=0.0, sample_index0: int = 0, phase_index0: int = 0, scale=None,
             out=None):
    """Mix, filter and resample a stream in GPU memory: one launch of amcx_resample on the current torch stream.

    x      : torch tensor on a GPU, contiguous: complex64 (S,), or int16 (sc16) / int8 (ci8) / uint8 (cu8: zero level 128) of
             shape (S, 2), I then Q, as :func:`amcpy_amd.ddc.tune_decimate` takes them.
    taps   : T real taps at the upsampled rate, 1 <= T <= 4096: a float32 tensor on the same device, or anything
             ``numpy.asarray`` takes.  They carry the gain (:func:`design_resample_lowpass`: DC gain ``interp``).
    interp, decim : L in 1 ... 256, D in 1 ... 4096: L outputs for every D inputs.
    shift  : cycles per input sample (float or Fraction); a signal at +f Hz goes to 0 with -f / fs.
    sample_index0 : the index of x[0] in the stream this call continues: ``phase0 = sample_index0 * phase_step mod 2^64``.
    phase_index0  : tau0, the polyphase index of the first output, 0 <= tau0 < L (a continuation's ``(M D + tau0) mod L``).
    scale  : integer formats only, default 2^-15 / 2^-7.
    out    : optional complex64 tensor with room for the M outputs.
    Returns complex64 (M,), M = :func:`out_samples`."""
    import torch

    f = _stream.front(x, taps, scale, shift, sample_index0, lambda S, T: out_samples(S, T, interp, decim, phase_index0))
    L, D, tau0 = int(interp), int(decim), int(phase_index0)
    if out is None:
        out = torch.empty((f.M,), dtype=torch.complex64, device=x.device)
    elif out.dtype != torch.complex64 or out.device != x.device or out.dim() != 1 or not out.is_contiguous() or out.shape[0] < f.M:
        raise ValueError(f"out must be a contiguous complex64 tensor of at least {f.M} samples on x's device")
    _stream.launch(x, lambda lib, stream: lib.amcx_resample(
        x.data_ptr() if f.S else None, f.kind, f.S, f.scale, f.phase0, f.step, f.taps.data_ptr(), f.T, L, D, tau0,
        out.data_ptr() if f.M else None, int(out.shape[0]), stream))
    return out[:f.M]


class Resampler(_stream.Stream):
    """The streaming form of :func:`resample`: ``push(chunk)`` returns the outputs the stream so far completes.

    Keeps the unconsumed tail of the input, ``index`` -- the absolute index of the sample the next output's window begins
    at, ``floor(outputs * decim / interp)`` -- and ``phase_index`` -- that output's polyphase index,
    ``outputs * decim mod interp``.  Where ``decim > P * interp`` the next window may begin beyond the data: the samples up
    to it are dropped as they arrive (a pending skip, as in :class:`amcpy_amd.ddc.Channelizer`).  Every call advances the
    phase accordingly, so the concatenated results equal ONE call over the whole stream bit for bit, however it is cut.
    ``fmt``: "cf32", "sc16", "ci8" or "cu8" -- what every chunk must be.  ``compute``: an injected
    ``f(x, taps, interp, decim, shift=..., sample_index0=..., phase_index0=..., scale=...)`` over numpy chunks (tests); the
    default is :func:`resample` over GPU tensors, with the taps uploaded once."""

    _NOUN, _one_shot = "resampler", staticmethod(resample)

    def __init__(self, taps, interp: int, decim: int, shift=0.0, fmt: str = "cf32", scale=None, *, compute=None):
        self.phase_index = 0           # tau0 of the next output
        super().__init__(taps, shift, fmt, scale, compute, interp=interp, decim=decim)

    def _limits(self):
        out_samples(0, self.taps.shape[0], self.interp, self.decim)

    def _args(self):
        return self.interp, self.decim

    def _kw(self):
        return dict(super()._kw(), phase_index0=self.phase_index)

    def _outputs(self, S):
        return out_samples(S, self.taps.shape[0], self.interp, self.decim, self.phase_index)

    def _run(self, buf, M):
        if M:
            return super()._run(buf, M)
        if isinstance(buf, np.ndarray):                              # nothing completes (a skip pending, fewer than P samples): no launch
            return np.empty(0, np.complex64)
        import torch
        return torch.empty(0, dtype=torch.complex64, device=buf.device)

    def _consumed(self, M):
        used, self.phase_index = divmod(M * self.decim + self.phase_index, self.interp)      # ... and the next output's phase
        return used
