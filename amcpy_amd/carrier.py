"""Blind carrier recovery on the device (include/amcx.h, ABI 16.2.3; amcpy_amd/csrc/amcx_carrier_kernel.h): per row of N
complex64 samples the power, the gain that makes it 1, the carrier's offset and phase from the M-th-power spectrum, and the row
with all three taken out -- one launch of ``amcx_carrier_c64`` on the current torch stream.

    y, est = carrier.recover(frames, order=4)          # (R, N) complex64 on the GPU -> the recovered rows and the records
    est = carrier.estimate(frames, order=4)             # the records alone
    y = carrier.apply(frames, carrier.combine(est, groups))     # one frequency per emitter, each frame's own phase

``order`` M is 1 (a bare carrier), 2 (BPSK), 4 (QPSK, and what the QAMs mostly answer to) or 8 (8PSK).  The phase is one of
the M equivalent ones (the header's M-FOLD AMBIGUITY).  N is a power of two of 64 ... 4096.  The records are 32 bytes each
(:data:`amcpy_amd._lib.CARRIER_RECORD`); :class:`Estimates` reads their fields."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import _lib, _stream

ORDERS = (1, 2, 4, 8)
MIN_N, MAX_N = 64, 4096
RECORD_BYTES = 32
RECORD = np.dtype(_lib.CARRIER_RECORD)
assert RECORD.itemsize == RECORD_BYTES


def _check_shape(N: int, order: int) -> None:
    if N < MIN_N or N > MAX_N or N & (N - 1):
        raise ValueError(f"rows must hold a power of two of {MIN_N} ... {MAX_N} samples, not {N}")
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, not {order!r}")


def search_bins(N: int, order: int = 4, search=None) -> int:
    """The entry's ``search_bins``: ``search`` is the largest carrier offset looked for, in cycles per sample OF x (a float or a
    Fraction); its line in x^M stands at M * search * N bins, rounded up and kept inside 0 ... N / 2 - 1.  None: N / 16 bins."""
    N, order = int(N), int(order)
    _check_shape(N, order)
    if search is None:
        return N // 16
    s = Fraction(search)
    if s < 0:
        raise ValueError(f"search must be >= 0 cycles per sample, got {search!r}")
    b = s * order * N
    return int(min(-(-b.numerator // b.denominator), N // 2 - 1))


class Estimates:
    """The records of R rows: ``raw`` is a uint8 ``(R, 32)`` torch tensor (on the device the estimate ran on, or on the host);
    ``n`` and ``order`` are what they were estimated with.  Fields come out as torch tensors of R elements."""

    def __init__(self, raw, n: int, order: int):
        import torch
        if not isinstance(raw, torch.Tensor) or raw.dtype != torch.uint8 or raw.dim() != 2 or int(raw.shape[1]) != RECORD_BYTES \
                or not raw.is_contiguous():
            raise TypeError("raw must be a contiguous uint8 (R, 32) torch tensor")
        _check_shape(int(n), int(order))
        self.raw, self.n, self.order = raw, int(n), int(order)

    @classmethod
    def from_numpy(cls, records, n: int, order: int, device=None) -> "Estimates":
        """From a numpy array of :data:`RECORD` (hand-made or smoothed on the host)."""
        import torch
        rec = np.ascontiguousarray(np.asarray(records, dtype=RECORD).reshape(-1))
        raw = torch.from_numpy(rec.view(np.uint8).reshape(-1, RECORD_BYTES).copy())
        return cls(raw if device is None else raw.to(device), n, order)

    def __len__(self) -> int:
        return int(self.raw.shape[0])

    def numpy(self) -> np.ndarray:
        """The records as a numpy array of :data:`RECORD` (a copy on the host)."""
        return self.raw.cpu().numpy().reshape(-1).view(RECORD).copy()

    def _i64(self):
        import torch
        return self.raw.view(torch.int64)

    def _i32(self):
        import torch
        return self.raw.view(torch.int32)

    def _f32(self):
        import torch
        return self.raw.view(torch.float32)

    phase_step = property(lambda self: self._i64()[:, 0], doc="int64: the offset in 2^-64 cycle per sample")
    phase0 = property(lambda self: self._i32()[:, 2].long() & 0xFFFFFFFF, doc="int64 holding the uint32: the phase in 2^-32 cycle")
    bin = property(lambda self: self._i32()[:, 3], doc="int32: the signed bin of the M-th power's line")
    frac = property(lambda self: self._f32()[:, 4], doc="float32: the interpolated part of a bin, -0.5 ... 0.5")
    power = property(lambda self: self._f32()[:, 5], doc="float32: the row's mean |x|^2")
    gain = property(lambda self: self._f32()[:, 6], doc="float32: 1 / sqrt(power), 0 for a row without a finite power > 0")
    quality = property(lambda self: self._f32()[:, 7], doc="float32: the line's share of the M-th power's energy, 1 for a tone")

    @property
    def cycles(self):
        """float64: the carrier's offset in cycles per sample of x (``* sample_rate`` = Hz)."""
        return self.phase_step.double() * 2.0 ** -64

    @property
    def phase(self):
        """float64: phase0 in cycles, 0 ... 1 / order."""
        return self.phase0.double() * 2.0 ** -32


def _rows(rows, name="rows"):
    import torch
    R, N, stride = _stream.rows_of(rows, torch.complex64, name, "N", MIN_N, MAX_N,
                                   narrow="rows must hold a power of two of 64 ... 4096 samples, not {}")
    return R, N, stride


def _out(out, R, N, like):
    import torch
    if out is None:
        return torch.empty((R, N), dtype=torch.complex64, device=like.device), N
    _, _, stride = _stream.rows_of(out, torch.complex64, "out", "N", N, N, narrow="out must have N = " + str(N) + " columns, not {}",
                                   min_rows=R, device=like.device)
    if int(out.shape[0]) != R:
        raise ValueError(f"out has {int(out.shape[0])} rows, the call makes {R}")
    return out, stride


def _flags(gain: bool, freq: bool, phase: bool) -> int:
    return (_lib.CARRIER_GAIN if gain else 0) | (_lib.CARRIER_FREQ if freq else 0) | (_lib.CARRIER_PHASE if phase else 0)


def _run(rows, order, sb, flags, est_raw, out, out_stride) -> None:
    R, N, stride = _rows(rows)
    _stream.launch(rows, lambda lib, stream: lib.amcx_carrier_c64(
        rows.data_ptr() if R else None, R, N, stride, int(order), int(sb), int(flags), est_raw.data_ptr() if R else None,
        None if out is None or not R else out.data_ptr(), int(out_stride), stream))


def estimate(rows, order: int = 4, search=None, *, search_bins_: int | None = None) -> Estimates:
    """The records of ``rows`` complex64 ``(R, N)`` on the GPU (a strided view with contiguous rows will do): estimate only.
    ``search``: :func:`search_bins`' (cycles per sample of x; default N / 16 bins); ``search_bins_`` gives the bins themselves."""
    import torch
    R, N, _ = _rows(rows)
    _check_shape(N, int(order))
    sb = search_bins(N, order, search) if search_bins_ is None else int(search_bins_)
    raw = torch.empty((R, RECORD_BYTES), dtype=torch.uint8, device=rows.device)
    _run(rows, order, sb, 0, raw, None, 0)
    return Estimates(raw, N, int(order))


def recover(rows, order: int = 4, search=None, *, gain: bool = True, freq: bool = True, phase: bool = True, out=None,
            search_bins_: int | None = None) -> tuple:
    """Estimate and apply in ONE launch -> ``(y, est)``: ``y`` complex64 ``(R, N)`` with the gain, the frequency and the phase
    taken out (each can be left in), ``est`` the :class:`Estimates`.  ``out``: a tensor to write; it must not overlap rows."""
    import torch
    R, N, _ = _rows(rows)
    _check_shape(N, int(order))
    sb = search_bins(N, order, search) if search_bins_ is None else int(search_bins_)
    out, out_stride = _out(out, R, N, rows)
    raw = torch.empty((R, RECORD_BYTES), dtype=torch.uint8, device=rows.device)
    _run(rows, order, sb, _flags(gain, freq, phase), raw, out, out_stride)
    return out, Estimates(raw, N, int(order))


def apply(rows, est: Estimates, *, gain: bool = True, freq: bool = True, phase: bool = True, out=None):
    """Take GIVEN records out of ``rows`` -> ``y``: nothing is estimated; row r gets record r's gain, phase_step and phase0 as
    they are -- one estimate for many frames (:func:`combine`), or one smoothed on the host (:meth:`Estimates.from_numpy`)."""
    R, N, _ = _rows(rows)
    if not isinstance(est, Estimates) or len(est) != R:
        raise ValueError(f"est must be the Estimates of the {R} rows")
    if N != est.n:
        raise ValueError(f"the records were estimated on rows of {est.n} samples, these have {N}")
    raw = est.raw if est.raw.device == rows.device else est.raw.to(rows.device)
    out, out_stride = _out(out, R, N, rows)
    _run(rows, est.order, 0, _flags(gain, freq, phase) | _lib.CARRIER_GIVEN, raw, out, out_stride)
    return out


def combine(est: Estimates, groups) -> Estimates:
    """One frequency per emitter: the records with every row's ``phase_step`` replaced by the (lower) MEDIAN of its group's and
    its ``phase0`` moved to match -- the phase at the row's centre stays what the row's own estimate made it,
    ``phase0' = phase0 + (phase_step - median) (N - 1) / 2``, reduced to 0 ... 1 / order again.  Power, gain and quality stay the
    row's own; bin and frac too (what the row itself answered).  ``groups``: an integer per row (rows with the same integer are
    one emitter), as a tensor or a sequence, or one int: that many consecutive rows per emitter.  Torch glue, on est's device."""
    import torch
    R = len(est)
    dev = est.raw.device
    if isinstance(groups, (int, np.integer)):
        if int(groups) < 1:
            raise ValueError("groups: at least one row per emitter")
        gid = torch.arange(R, device=dev) // int(groups)
    else:
        gid = torch.as_tensor(groups, device=dev).long().reshape(-1)
        if int(gid.shape[0]) != R:
            raise ValueError(f"groups names {int(gid.shape[0])} rows, the estimates hold {R}")
    raw = est.raw.clone()
    step, ph = est.phase_step.clone(), est.phase0
    med = step.clone()
    for g in torch.unique(gid).tolist():
        at = gid == g
        med[at] = step[at].median()                                    # the lower of the two middle ones
    lm = ORDERS.index(est.order)
    half = ((step - med) * (est.n - 1)) >> 1                           # int64, wrapping as the kernel's words do
    ph64 = (ph << 32) + half
    new_ph = (ph64 >> 32) & ((1 << (32 - lm)) - 1)
    raw.view(torch.int64)[:, 0] = med
    raw.view(torch.int32)[:, 2] = torch.where(new_ph >= 1 << 31, new_ph - (1 << 32), new_ph).int()
    return Estimates(raw, est.n, est.order)


def recover_frames(frames, recover_opt, sample_rate=None, groups=None):
    """What ``recover`` of :func:`amcpy_amd.sigmf.extract_sigmf` (a key of its ``tune`` dict), :func:`amcpy_amd.waveform.dataset_features` and
    :func:`amcpy_amd.occupancy.occupied_features` does to their ``(R, N)`` frames before the features: ``recover_opt`` is
    ``dict(order=M, search_hz=F, per="frame" | "emitter")`` -- ``search_hz`` needs ``sample_rate`` (the frames' own); without it
    the search covers N / 16 bins; ``search`` gives it in cycles per sample instead.  ``per="emitter"``: :func:`combine` over
    ``groups`` (default: all frames are one emitter).  -> ``(y, est)``."""
    known = {"order", "search_hz", "search", "per"}
    if not isinstance(recover_opt, dict) or set(recover_opt) - known or "order" not in recover_opt:
        raise ValueError(f"recover: a dict of {sorted(known)}, order among them")
    per = recover_opt.get("per", "frame")
    if per not in ("frame", "emitter"):
        raise ValueError(f"recover: per is 'frame' or 'emitter', not {per!r}")
    search = recover_opt.get("search")
    if recover_opt.get("search_hz") is not None:
        if search is not None:
            raise ValueError("recover: either search or search_hz")
        if not sample_rate:
            raise ValueError("recover: search_hz needs the frames' sample rate")
        search = Fraction(float(recover_opt["search_hz"])) / Fraction(float(sample_rate))
    order = int(recover_opt["order"])
    if per == "frame":
        return recover(frames, order, search)
    est = combine(estimate(frames, order, search), max(1, int(frames.shape[0])) if groups is None else groups)
    return apply(frames, est), est
