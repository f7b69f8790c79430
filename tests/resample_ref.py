"""The float64 reference of the rational resampler (include/amcx.h, amcx_resample) and the criterion it is held to.

    phi(n) = (phase0 + n * phase_step) mod 2^64               -- Python integers, exact (ddc_ref.phases)
    v[n]   = x[n] * exp(2j pi phi(n) / 2^64)                  -- numpy float64 / complex128
    P      = ceil(T / L),   t_m = m D + tau0,   p_m = t_m mod L,   n_m = (P - 1) + t_m // L
    y[m]   = sum_{q >= 0, p_m + q L < T} h[p_m + q L] v[n_m - q]   -- summed in float64
    S[m]   = sum_q |h[p_m + q L]| |x[n_m - q]|

THE CRITERION: |y - y64| <= (P + 8) 2^-24 S[m] for every output.  This is tests/ddc_ref.py's argument with the at most P terms
of one phase in place of the T of the down-converter: P - 1 FMAs and one product, each rounding once (2^-24 relative to a
partial sum that sum_q |h||v| bounds), is the worst case of ANY fp32 order of the terms; the other 8 x 2^-24 |h||x| per term
cover the mixed sample itself (the angle's fp32 rounding and the two polynomials, under 2.5 x 2^-24 together, and the rounded
complex product, under 2.9 x 2^-24 in magnitude).  Derived, not fitted.  A phase with no tap has S = 0 and must be exactly 0.

WHAT IT SEES.  With taps from +-[0.5, 1] a dropped or shifted tap costs at least S / (2 P), which is 2^24 / (2 P (P + 8)) times the
bound: 20 000 at P = 17 (the designer's 16 taps per phase), 1900 at P = 63 -- and 2 at P = 2048, below 1 from P = 2893 on, 0.5
at P = 4096 (L = 1, T = 4096), where a single missing term passes the bound about as often as not.  The shapes with thousands
of taps per phase are held to an EQUALITY instead: tests/chain_exact.py makes data on which fp32 arithmetic in any order is
exact, and tests/test_gpu_chain_exact.py compares every output with == against int64 arithmetic."""
import numpy as np

from tests.ddc_ref import MASK64, ODD_STEP, U, make_taps, phases, widen  # noqa: F401  (shared with the tests)


def phase_taps(T, L):
    return -(-int(T) // int(L))


def out_samples_brute(S, T, L, D, tau0=0):
    """M by enumeration: the outputs m = 0, 1, ... whose newest sample n_m = (P - 1) + (m D + tau0) // L is at most S - 1."""
    P, m = phase_taps(T, L), 0
    while (P - 1) + (m * D + tau0) // L <= S - 1:
        m += 1
    return m


def out_samples(S, T, L, D, tau0=0):
    P = phase_taps(T, L)
    last = (S - P + 1) * L - 1 - tau0
    return 0 if S < P or last < 0 else last // D + 1


def gather(M, T, L, D, tau0):
    """(idx (M, P) int64, tap (M, P) int64, live (M, P) bool): the sample and the tap index of term q of output m, and
    whether that term exists (p_m + q L < T); dead entries point at sample n_m and tap 0"""
    P = phase_taps(T, L)
    t = np.arange(M, dtype=np.int64) * D + tau0
    p, top = t % L, (P - 1) + t // L
    q = np.arange(P, dtype=np.int64)
    tap = p[:, None] + q[None, :] * L
    live = tap < T
    return np.where(live, top[:, None] - q[None, :], top[:, None]), np.where(live, tap, 0), live


def reference(x, taps, L, D, tau0=0, phase0=0, phase_step=0, M=None):
    """x: complex128 samples (widen), taps: float32 -> (y64 (M,) complex128, S (M,) float64)"""
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    T = h.shape[0]
    M = out_samples(x.shape[0], T, L, D, tau0) if M is None else int(M)
    if M == 0:
        return np.zeros(0, np.complex128), np.zeros(0, np.float64)
    idx, tap, live = gather(M, T, L, D, tau0)
    need = np.unique(idx)                                   # mix every sample that is read once
    v = x[need] * np.exp(2j * np.pi * phases(need, phase0, phase_step))
    pos = np.searchsorted(need, idx)
    hw = np.where(live, h[tap], 0.0)
    return (v[pos] * hw).sum(axis=1), (np.abs(x[need])[pos] * np.abs(hw)).sum(axis=1)


def worst_ratio(y, y64, s, P):
    """max over the outputs of |y - y64| / ((P + 8) 2^-24 S): the criterion holds iff <= 1 (an output whose S is 0 must be
    exactly 0: ratio inf otherwise)"""
    if y64.shape[0] == 0:
        return 0.0
    err = np.abs(np.asarray(y).astype(np.complex128) - y64)
    bound = (P + 8) * U * s
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def numpy_resample(x, taps, interp, decim, *, shift=0.0, sample_index0=0, phase_index0=0, scale=None):
    """A resampler over numpy chunks with the signature amcpy_amd.resample.Resampler's ``compute`` takes, POSITION
    INDEPENDENT as the kernel is: a sample is mixed by element-wise float64 arithmetic and an output is summed term by term
    in ascending q (a term that does not exist adds nothing: not even a zero), so its bits do not depend on where in a call
    it stands.  x: complex64 (S,) or integer (S, 2); -> complex64 (M,)."""
    from amcpy_amd.ddc import _format_of, _scale_of, phase_step_of
    fmt = _format_of(x)
    step = phase_step_of(shift)
    xw = widen(x, fmt, _scale_of(fmt, scale))
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    T, L, D, tau0 = h.shape[0], int(interp), int(decim), int(phase_index0)
    M = out_samples(xw.shape[0], T, L, D, tau0)
    y = np.zeros(M, np.complex128)
    if M == 0:
        return y.astype(np.complex64)
    idx, tap, live = gather(M, T, L, D, tau0)
    n = np.arange(int(idx.max()) + 1)
    v = xw[n] * np.exp(2j * np.pi * phases(n, (int(sample_index0) * step) & MASK64, step))
    for q in range(idx.shape[1]):
        y = np.where(live[:, q], y + h[tap[:, q]] * v[idx[:, q]], y)
    return y.astype(np.complex64)
