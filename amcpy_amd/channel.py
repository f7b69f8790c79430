"""The fading multipath channel: rows of IQ through a time-varying tapped delay line (amcx_channel_c64, include/amcx.h ABI 16.2.1).

One launch takes rows of complex64 in GPU memory -- generated (:mod:`amcpy_amd.waveform`) or recorded -- through ``L`` paths.
A path has a delay in whole samples and a gain that is a sum of ``S`` sinusoids with uniform arrival angles and phases (a
Rayleigh process with the Jakes Doppler spectrum) plus an optional line-of-sight term (Rician); optionally the launch adds the
generator's white noise.  Every random integer is fixed by the header's contract and a sample is named by its absolute row and
absolute index, so rows cut into calls, or a stream cut into chunks of any length, equal one call bit for bit;
tests/channel_ref.py restates it in numpy.

    Profile                      delays and powers, normalised to unit total power; ``records(S)`` are the entry's path records
    rayleigh / rician / exponential / two_ray / static       the builders
    default_interp_log2          the node spacing a Doppler allows
    apply                        one launch: (R, S + H) complex64 -> (R, S)
    Fader                        one row as a stream, ``push(chunk)``

A row of the input holds ``H = max delay`` samples of history in front of the first output: output i reads inputs
``i + H - delay``, the down-converter's convention.  Not built: named standard profiles, fractional delays, correlated paths,
shadowing, sc16 / 8-bit input (widen first), a path table on the device.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from . import _lib, _stream

MAX_PATHS, MAX_SINUSOIDS, MAX_DELAY, MAX_INTERP_LOG2 = _lib.CHANNEL_MAX_PATHS, _lib.CHANNEL_MAX_SINUSOIDS, _lib.CHANNEL_MAX_DELAY, 16
RECORD = np.dtype([("delay", "<i4"), ("diffuse_gain", "<f4"), ("los_gain", "<f4"), ("los_doppler_q31", "<i4")])
_MASK64 = (1 << 64) - 1
_tensor = lambda t: hasattr(t, "data_ptr")                                 # noqa: E731  (a torch tensor, without importing torch)


class Profile:
    """``L`` paths: ``delays`` in samples (0 ... 1024), the power of each path's diffuse (Rayleigh) part and of its line of
    sight, and the line of sight's Doppler as a fraction (-1 ... 1, the cosine of its arrival angle) of the maximum Doppler.
    The powers are normalised to a total of 1, so an ``snr_db`` keeps its meaning on average."""

    def __init__(self, delays, diffuse_power, los_power=0, los_doppler=0):
        d = np.atleast_1d(np.asarray(delays))
        if d.ndim != 1 or not 1 <= d.shape[0] <= MAX_PATHS or not np.all(d == np.round(d)) or d.min() < 0 or d.max() > MAX_DELAY:
            raise ValueError(f"1 ... {MAX_PATHS} paths with whole delays in 0 ... {MAX_DELAY} samples, got {delays!r}")
        L = d.shape[0]
        dp, lp, ld = (np.broadcast_to(np.asarray(v, dtype=np.float64), (L,)).copy() for v in (diffuse_power, los_power, los_doppler))
        total = float(dp.sum() + lp.sum())
        if not (np.all(np.isfinite(dp)) and np.all(np.isfinite(lp)) and dp.min() >= 0 and lp.min() >= 0 and total > 0):
            raise ValueError("the powers must be finite, none negative and not all zero")
        if not np.all(np.abs(ld) <= 1.0):
            raise ValueError("los_doppler is a fraction of the maximum Doppler: -1 ... 1")
        self.delays = d.astype(np.int64)
        self.diffuse_gain, self.los_gain, self.los_doppler = np.sqrt(dp / total), np.sqrt(lp / total), ld

    @classmethod
    def of_gains(cls, delays, diffuse_gain, los_gain, los_doppler=0) -> "Profile":
        """The paths with their GAINS as given: nothing is normalised, and a gain may be negative."""
        p = cls(delays, 1.0)
        L = p.delays.shape[0]
        p.diffuse_gain, p.los_gain, p.los_doppler = (np.broadcast_to(np.asarray(v, dtype=np.float64), (L,)).copy()
                                                     for v in (diffuse_gain, los_gain, los_doppler))
        return p

    @property
    def history(self) -> int:
        """H: the samples of input in front of the first output"""
        return int(self.delays.max())

    @property
    def power(self) -> float:
        return float((self.diffuse_gain ** 2).sum() + (self.los_gain ** 2).sum())

    def records(self, sinusoids: int) -> np.ndarray:
        """The entry's 16-byte path records for sums of ``sinusoids`` sinusoids: ``1 / sqrt(S)`` folded into ``diffuse_gain``."""
        S = int(sinusoids)
        if not 1 <= S <= MAX_SINUSOIDS:
            raise ValueError(f"sinusoids {S} is outside 1 ... {MAX_SINUSOIDS}")
        rec = np.zeros(self.delays.shape[0], RECORD)
        rec["delay"] = self.delays
        rec["diffuse_gain"] = self.diffuse_gain / math.sqrt(S)
        rec["los_gain"] = self.los_gain
        rec["los_doppler_q31"] = np.clip(np.rint(self.los_doppler * 2.0 ** 31), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
        return rec


def rayleigh() -> Profile:
    """One path, no line of sight: flat Rayleigh fading."""
    return Profile([0], [1.0])


def rician(k_db: float, los_doppler: float = 0.0) -> Profile:
    """One path with a line of sight ``k_db`` dB above its diffuse part (the Rician K factor)."""
    k = 10.0 ** (float(k_db) / 10.0)
    return Profile([0], [1.0], [k], [los_doppler])


def exponential(n_paths: int, spacing: int, decay_db: float) -> Profile:
    """``n_paths`` Rayleigh paths ``spacing`` samples apart, each ``decay_db`` dB below the one before."""
    l = np.arange(int(n_paths))
    return Profile(l * int(spacing), 10.0 ** (-float(decay_db) * l / 10.0))


def two_ray(delay: int, rel_db: float) -> Profile:
    """Two Rayleigh paths: at 0 and, ``rel_db`` dB relative to it, at ``delay`` samples."""
    return Profile([0, int(delay)], [1.0, 10.0 ** (float(rel_db) / 10.0)])


def static(delays, gains) -> Profile:
    """Line-of-sight terms only, with the GAINS as given (not normalised), in ascending delay.  Applied with
    ``random_phase=False`` and no Doppler it is the sparse FIR filter ``h[delay_l] = gain_l``."""
    d = np.atleast_1d(np.asarray(delays))
    g = np.broadcast_to(np.asarray(gains, dtype=np.float64), d.shape)
    order = np.argsort(d, kind="stable")
    return Profile.of_gains(d[order], 0.0, g[order])


def parse_profile(text: str) -> Profile:
    """``rayleigh`` | ``rician:K_DB`` | ``exp:N:SPACING:DECAY_DB`` | ``tworay:DELAY:DB`` (the `synth` command's --channel) ->
    the builder's profile, with the text kept as ``spec``."""
    name, *args = str(text).split(":")
    try:
        if name == "rayleigh" and not args:
            p = rayleigh()
        elif name == "rician" and len(args) == 1:
            p = rician(float(args[0]))
        elif name == "exp" and len(args) == 3:
            p = exponential(int(args[0]), int(args[1]), float(args[2]))
        elif name == "tworay" and len(args) == 2:
            p = two_ray(int(args[0]), float(args[1]))
        else:
            raise ValueError("no such profile")
    except ValueError as e:
        raise ValueError(f"--channel: rayleigh | rician:K_DB | exp:N:SPACING:DECAY_DB | tworay:DELAY:DB, got {text!r} ({e})")
    p.spec = str(text)
    return p


def doppler_max_of(doppler) -> int:
    """The maximum Doppler, cycles per sample -> the entry's units of 2^-33 cycles per sample."""
    c = int(round(Fraction(doppler) * (1 << 33)))
    if not 0 <= c < 1 << 32:
        raise ValueError(f"doppler must lie in [0, 0.5) cycles per sample, got {doppler!r}")
    return c


def default_interp_log2(doppler) -> int:
    """The largest b <= 16 with ``doppler * 2^b <= 1 / 64``: nodes at most 1 / 64 of the fastest sinusoid's period apart
    (0 where even one sample is more)."""
    f, b = Fraction(doppler), MAX_INTERP_LOG2
    while b > 0 and f * (1 << b) > Fraction(1, 64):
        b -= 1
    return b


def _plan(profile, doppler, sinusoids, interp_log2, random_phase) -> tuple:
    if not isinstance(profile, Profile):
        raise TypeError("profile must be a channel.Profile (rayleigh(), rician(k_db), exponential(...), two_ray(...), static(...))")
    S = int(sinusoids)
    b = default_interp_log2(doppler) if interp_log2 is None else int(interp_log2)
    if not 0 <= b <= MAX_INTERP_LOG2:
        raise ValueError(f"interp_log2 {b} is outside 0 ... {MAX_INTERP_LOG2}")
    return profile.records(S), S, b, doppler_max_of(doppler), _lib.CHANNEL_RANDOM_PHASE if random_phase else 0


def apply(x, profile, *, doppler=0.0, sinusoids: int = 16, interp_log2=None, seed: int = 0, row_index0: int = 0,
          sample_index0: int = 0, snr_db=None, sigma=None, frames_per_group=None, random_phase: bool = True, out=None, compute=None):
    """One launch of amcx_channel_c64 on the current torch stream -> complex64 ``(R, S)`` in GPU memory.

    x        : complex64 ``(R, S + H)`` on the GPU, possibly a strided view with contiguous rows; ``H = profile.history``
               samples of every row stand in front of its first output.
    profile  : a :class:`Profile`.  ``doppler``: the maximum Doppler in cycles per sample, [0, 0.5).  ``sinusoids``: 1 ... 32
               per path.  ``interp_log2``: the gains are computed every 2^b samples and interpolated linearly between
               (default :func:`default_interp_log2`; 0: the closed form at every sample).
    seed, row_index0, sample_index0 : the key and where the call begins; rows ``row_index0 ...`` and output samples
               ``sample_index0 ...`` of the same seed see the same channel in whatever call they pass it.
    snr_db / sigma : the generator's noise added in the same launch, a scalar or one value per group of ``frames_per_group``
               rows (default: the rows spread evenly over the values); neither: no noise.  ``sigma`` may be a float32 tensor
               on the device: with it and ``out`` given the call is the launch alone and can be captured in a graph.
    random_phase : the lines of sight start at a drawn phase; else at 0.
    out      : a complex64 tensor ``(R, S)`` to write, possibly a strided view with contiguous rows; it must not overlap x.
    compute  : tests only -- ``f(x, records, S, interp_log2, doppler_max, flags, sigma, frames_per_group, seed=...,
               row_index0=..., sample_index0=...)`` over numpy (tests/channel_ref.numpy_apply)."""
    rec, S, b, doppler_max, flags = _plan(profile, doppler, sinusoids, interp_log2, random_phase)
    H = profile.history
    if snr_db is not None and sigma is not None:
        raise ValueError("either snr_db or sigma")
    if snr_db is not None:
        sigma = (10.0 ** (-np.atleast_1d(np.asarray(snr_db, dtype=np.float64)) / 20.0)).astype(np.float32)
    if sigma is not None and not _tensor(sigma):
        sigma = np.ascontiguousarray(np.atleast_1d(np.asarray(sigma, dtype=np.float32)))
        if sigma.ndim != 1 or not np.all(np.isfinite(sigma)) or np.any(sigma < 0):
            raise ValueError("every sigma must be a finite float32 >= 0")
    if x.ndim != 2 or int(x.shape[1]) <= H:
        raise ValueError(f"x must be (R, S + H) with S >= 1 and H = {H} samples of history")
    R, count = int(x.shape[0]), int(x.shape[1]) - H
    G = 1 if sigma is None else int(sigma.shape[0])
    fpg = max(1, -(-R // G)) if frames_per_group is None else int(frames_per_group)
    if fpg < 1 or (sigma is not None and R > 0 and -(-R // fpg) > G):
        raise ValueError(f"{R} rows in groups of {fpg} need {-(-R // max(fpg, 1))} sigmas, {G} given")
    if not 0 <= int(sample_index0) or int(sample_index0) + count >= 1 << 40:
        raise ValueError(f"sample_index0 {sample_index0} with {count} samples is outside 0 ... 2^40")
    where = dict(seed=int(seed) & _MASK64, row_index0=int(row_index0) & _MASK64, sample_index0=int(sample_index0))
    if compute is not None:
        if _tensor(x) or _tensor(sigma) or out is not None:
            raise TypeError("an injected compute takes host arrays and returns its own output")
        return compute(np.asarray(x, dtype=np.complex64), rec, S, b, doppler_max, flags, sigma, fpg, **where)

    import torch
    _, _, in_stride = _stream.rows_of(x, torch.complex64, "x", "S + H", H + 1, narrow="x must have S + H > " + str(H) + " columns, not {}")
    if out is None:
        out = torch.empty((R, count), dtype=torch.complex64, device=x.device)
        out_stride = count
    else:
        _, _, out_stride = _stream.rows_of(out, torch.complex64, "out", "S", count, count, narrow="out must have S = " + str(count) +
                                           " columns, not {}", min_rows=R, device=x.device)
        if int(out.shape[0]) != R:
            raise ValueError(f"out has {int(out.shape[0])} rows, the call makes {R}")
    if sigma is not None and not isinstance(sigma, torch.Tensor):
        sigma = torch.from_numpy(sigma).to(x.device)
    if sigma is not None and (sigma.dtype != torch.float32 or sigma.device != x.device or sigma.dim() != 1 or not sigma.is_contiguous()):
        raise TypeError("sigma must be a contiguous one-dimensional float32 tensor on x's device")
    _stream.launch(x, lambda lib, stream: lib.amcx_channel_c64(
        where["seed"], where["row_index0"], where["sample_index0"], R, count, x.data_ptr() if R else None, in_stride,
        rec.ctypes.data, int(rec.shape[0]), S, b, doppler_max, flags, None if sigma is None else sigma.data_ptr(), fpg,
        out.data_ptr() if R else None, out_stride, stream))
    return out


class Fader(_stream.Chunked):
    """One row through a channel as a stream: ``push(chunk)`` returns the outputs the chunk completes -- as many as it has
    samples -- bit for bit those of one :func:`apply` over the whole stream.  The stream starts with ``H`` zeros of history.
    The keywords are :func:`apply`'s (``sigma`` / ``snr_db``: one value); ``row`` is the absolute row."""

    _NOUN = "fader"

    def __init__(self, profile, *, row: int = 0, compute=None, **kw):
        for bad in ("row_index0", "sample_index0", "out", "frames_per_group"):
            if bad in kw:
                raise ValueError(f"Fader: {bad} is the stream's own")
        super().__init__("cf32", compute)
        _plan(profile, kw.get("doppler", 0.0), kw.get("sinusoids", 16), kw.get("interp_log2"), kw.get("random_phase", True))
        self.profile, self.row, self._kw, self._sigma = profile, int(row), dict(kw), None

    def push(self, chunk):
        if self._tail is None and self.profile.history:                    # the H zeros in front of the stream
            H = self.profile.history
            self._tail = np.zeros(H, np.complex64) if isinstance(chunk, np.ndarray) else chunk.new_zeros(H)
        return super().push(chunk)

    def _outputs(self, S):
        return max(0, S - self.profile.history)

    def _consumed(self, M):
        return M

    def _run(self, buf, M):
        if M == 0:
            return buf[:0]
        kw = self._kw
        if self._compute is None and (kw.get("sigma") is not None or kw.get("snr_db") is not None):
            if self._sigma is None or self._sigma.device != buf.device:    # sigma goes to the device once
                import torch
                s = kw["sigma"] if kw.get("sigma") is not None else 10.0 ** (-float(kw["snr_db"]) / 20.0)
                self._sigma = s if _tensor(s) else torch.full((1,), float(s), dtype=torch.float32, device=buf.device)
            kw = dict(kw, sigma=self._sigma, snr_db=None)
        return apply(buf[None, :], self.profile, row_index0=self.row, sample_index0=self.index, compute=self._compute, **kw)[0]
