"""The float64 reference of the digital down-converter (include/amcx.h, amcx_tune_decimate) and the criterion it is held to.

    phi(n) = (phase0 + n * phase_step) mod 2^64     -- Python integers, exact
    v[n]   = x[n] * exp(2j pi phi(n) / 2^64)        -- numpy float64 / complex128
    y[m]   = sum_k h[k] v[m D + T - 1 - k]          -- summed in float64
    S[m]   = sum_k |h[k]| |x[m D + T - 1 - k]|

THE CRITERION: |y - y64| <= (T + 8) 2^-24 S[m] for every output.  T - 1 FMAs and one product, each rounding once
(2^-24 relative to a partial sum that sum_k |h||v| bounds), is the worst case of ANY fp32 order of the T terms; the other
8 x 2^-24 |h||x| per term cover the mixed sample itself: a sine and a cosine of an angle whose integer reduction is exact
(the angle's fp32 rounding and the two polynomials: under 2.5 x 2^-24 together) and the rounded complex product (three
roundings per component: under 2.9 x 2^-24 in magnitude).  Derived, not fitted.

WHAT IT SEES.  With taps from +-[0.5, 1] a dropped or shifted tap costs at least S / (2 T), which is 2^24 / (2 T (T + 8)) times the
bound: 1900 at T = 63, 60 at T = 365, 8 at T = 1024 -- and 2 at T = 2048, below 1 from T = 2893 on (0.5 at the resampler's
P = 4096).  At the largest tap counts the bound is as large as a whole missing term, so one term lost at one tile seam passes
it about as often as not.  Those shapes are held to an EQUALITY instead: tests/chain_exact.py makes data on which fp32
arithmetic in any order is exact, and tests/test_gpu_chain_exact.py compares every output with == against int64 arithmetic."""
import numpy as np

from amcpy_amd import _formats

MASK64 = (1 << 64) - 1
ODD_STEP = 0x9E3779B97F4A7C15          # an odd 64-bit constant: every bit of the phase accumulator moves
U = 2.0 ** -24


def out_samples(S, T, D):
    return 0 if S < T else (S - T) // D + 1


def widen(raw, fmt, scale):
    """What a stored sample stands for, as complex128 holding the exact float32 values: complex64 as it is; integers as
    float32(i) * float32(scale), cu8 as byte - 128."""
    if fmt == "cf32":
        return np.asarray(raw, dtype=np.complex64).astype(np.complex128)
    ints = raw.astype(np.int32) - _formats.get(fmt).zero
    w = ints.astype(np.float32) * np.float32(scale)
    return w[:, 0].astype(np.float64) + 1j * w[:, 1].astype(np.float64)


def phases(indices, phase0, phase_step):
    """phi at these sample indices as float64 turns in [0, 1): Python integers up to the division"""
    p0, st = int(phase0), int(phase_step)
    return np.array([((p0 + int(n) * st) & MASK64) / 18446744073709551616 for n in indices], dtype=np.float64)


def reference(x, taps, D, phase0=0, phase_step=0, M=None):
    """x: complex128 samples (widen), taps: float32 -> (y64 (M,) complex128, S (M,) float64)"""
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    T, D = h.shape[0], int(D)
    M = out_samples(x.shape[0], T, D) if M is None else int(M)
    if M == 0:
        return np.zeros(0, np.complex128), np.zeros(0, np.float64)
    if D <= T:                                        # every sample of the span is read
        n = np.arange((M - 1) * D + T)
        v = x[n] * np.exp(2j * np.pi * phases(n, phase0, phase_step))
        y = np.convolve(v, h, "valid")[::D]
        s = np.convolve(np.abs(x[n]), np.abs(h), "valid")[::D]
        return y[:M], s[:M]
    idx = np.arange(M)[:, None] * D + (T - 1 - np.arange(T))[None, :]          # (M, T): the sample tap k multiplies
    flat = idx.ravel()
    v = (x[flat] * np.exp(2j * np.pi * phases(flat, phase0, phase_step))).reshape(M, T)
    return v @ h, np.abs(x[flat]).reshape(M, T) @ np.abs(h)


def worst_ratio(y, y64, s, T):
    """max over the outputs of |y - y64| / ((T + 8) 2^-24 S): the criterion holds iff <= 1 (an output whose S is 0 must be
    exactly 0: ratio inf otherwise)"""
    if y64.shape[0] == 0:
        return 0.0
    err = np.abs(np.asarray(y).astype(np.complex128) - y64)
    bound = (T + 8) * U * s
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def make_taps(T, seed=0):
    """T taps from +-[0.5, 1]: every tap counts (a windowed sinc's end taps would hide an off-by-one)"""
    rng = np.random.default_rng(1000 + T + seed)
    return (rng.uniform(0.5, 1.0, T) * rng.choice([-1.0, 1.0], T)).astype(np.float32)


def numpy_ddc(x, taps, decim, *, shift=0.0, sample_index0=0, scale=None):
    """A down-converter over numpy chunks with the signature amcpy_amd.ddc.Channelizer's ``compute`` takes, POSITION
    INDEPENDENT as the kernel is: a sample is mixed by element-wise float64 arithmetic and an output is summed tap by tap
    in the order k = 0 ... T - 1, so its bits do not depend on where in a call it stands.  x: complex64 (S,) or integer
    (S, 2); -> complex64 (M,)."""
    from amcpy_amd.ddc import _format_of, _scale_of, phase_step_of
    fmt = _format_of(x)
    step = phase_step_of(shift)
    xw = widen(x, fmt, _scale_of(fmt, scale))
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    T, D = h.shape[0], int(decim)
    M = out_samples(xw.shape[0], T, D)
    n = np.arange((M - 1) * D + T if M else 0)
    v = xw[n] * np.exp(2j * np.pi * phases(n, (int(sample_index0) * step) & MASK64, step))
    y = np.zeros(M, np.complex128)
    for k in range(T if M else 0):
        y += h[k] * v[T - 1 - k::D][:M]
    return y.astype(np.complex64)
