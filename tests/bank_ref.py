"""The float64 reference of the polyphase filter bank (include/amcx.h, amcx_filter_bank) and the criterion it is held to.

THE REFERENCE.  By definition channel c of the bank is the down-converter (tests/ddc_ref.py, reference) with

    phase_step_c = phase_step - c 2^64 / C          phase0_c = phase0 - c (sample_index0 mod C) 2^64 / C        (mod 2^64)

C is a power of two, so both are exact integers: y[c, m] = sum_k h[k] x[n_m - k] exp(2 pi j (phi(n_m - k) - c a(n_m - k) / C))
with a(n) = (sample_index0 + n) mod C, and phi(n) 2^-64 - c a(n) / C differs from (phase0_c + n phase_step_c) 2^-64 by an integer.

THE CRITERION: |y - y64| <= (P + 8 + 7 log2 C) 2^-24 S[m], P = ceil(T / C), S[m] = sum_k |h[k]| |x[n_m - k]|.  Derived:
  - P + 8 is the down-converter's argument (tests/ddc_ref.py) per branch: a branch sum u[p] is one product and P - 1 FMAs,
    each rounding once relative to a partial sum that S_p = sum_q |h[p + q C]| |x[.]| bounds, and 8 x 2^-24 |h||x| per term
    cover the mixed sample itself.  The branches' bounds add up to (P + 8) 2^-24 S, and the transform's exact coefficients
    have modulus 1, so that is what reaches every output.
  - a radix-2 stage (decimation in frequency) forms A + B and (A - B) w: the sum or difference rounds by 2^-24 of its result,
    the twiddle w = ddc_mixer(exact integer angle) is off by at most 2.4 x 2^-24 (the angle's fp32 rounding and the two
    polynomials; 0 at +-1 and +-j), the rounded complex product by at most 2.9 x 2^-24 of its modulus (three roundings per
    component): at most 6.3, taken as 7, in units of 2^-24 of a partial sum of the transform, and every partial sum's modulus
    is at most sum_p |u_p| <= S (to first order; the second-order terms, (1 + 7 x 2^-24)^8 - 1 - 56 x 2^-24, are below 1e-4
    of the bound).  log2 C stages: 7 log2 C.
  - a radix-2 transform is what the kernel runs (two stages per pass over its rows, the same operations), so the 7 stands.
A dropped tap costs at least S / (2 T) with taps from +-[0.5, 1] (ddc_ref.make_taps): 25 times the bound at the largest
shape, C = 256, T = 4096 (P + 8 + 56 = 80: 80 x 2^-24 = 4.8e-6 against 1 / 8192 = 1.2e-4).  With FEW channels and many taps the
bound is as large as the term -- C = 2, T = 4096: P + 8 + 7 = 2063, 1.23e-4 against 1.22e-4 -- so those shapes are held to an
equality on data where fp32 arithmetic is exact (tests/chain_exact.py, tests/test_gpu_chain_exact.py), and at C >= 8 on the same
data to the transform's 7 log2 C alone."""
import numpy as np

from tests import ddc_ref
from tests.ddc_ref import MASK64, U


def log2_exact(C):
    C = int(C)
    assert C >= 2 and C & (C - 1) == 0, C
    return C.bit_length() - 1


def channel_phases(c, C, phase0, phase_step, sample_index0):
    """(phase0_c, phase_step_c): the down-converter that channel c of the bank is"""
    unit = (1 << 64) // int(C)
    return ((int(phase0) - c * (int(sample_index0) % int(C)) * unit) & MASK64, (int(phase_step) - c * unit) & MASK64)


def reference_by_definition(x, taps, C, D, phase0=0, phase_step=0, sample_index0=0, channels=None):
    """THE DEFINITION, one down-converter per channel: x: complex128 samples (ddc_ref.widen), taps: float32 ->
    (y64 (len(channels), M) complex128, S (M,) float64).  ``channels``: the channels to compute, default all C."""
    chans = range(int(C)) if channels is None else list(channels)
    ys, s = [], None
    for c in chans:
        p0, st = channel_phases(c, C, phase0, phase_step, sample_index0)
        y, s = ddc_ref.reference(x, taps, D, p0, st)
        ys.append(y)
    return np.stack(ys), s


def reference(x, taps, C, D, phase0=0, phase_step=0, sample_index0=0, channels=None):
    """The same sums as :func:`reference_by_definition`, in float64 too, but with the work the channels share done once (256
    channels of 4096 taps in a second, not a minute): phi(n) in uint64 arithmetic, which wraps mod 2^64 and is exact as
    Python's integers are; the mixed samples every tap of every output multiplies, gathered once as an (M, T) array; channel
    c's factor exp(-2 pi j c a(n) / C) from a table of the C-th roots of unity, indexed by the exact integer (c a(n)) mod C.
    It rounds a few more times than the definition does, each 2^-53: tests/test_bank_host.py holds the two together to
    1e-12 S, seven orders below the criterion."""
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    T, C, D = h.shape[0], int(C), int(D)
    chans = list(range(C)) if channels is None else list(channels)
    M = ddc_ref.out_samples(x.shape[0], T, D)
    if M == 0:
        return np.zeros((len(chans), 0), np.complex128), np.zeros(0, np.float64)
    idx = np.arange(M)[:, None] * D + (T - 1 - np.arange(T))[None, :]          # (M, T): the sample tap k multiplies
    with np.errstate(over="ignore"):
        phi = np.uint64(int(phase0) & MASK64) + idx.astype(np.uint64) * np.uint64(int(phase_step) & MASK64)
    v = x[idx] * np.exp(2j * np.pi * (phi.astype(np.float64) / 18446744073709551616.0))
    a = (idx + int(sample_index0) % C) % C
    roots = np.exp(-2j * np.pi * np.arange(C) / C)
    y = np.stack([(v * roots[(c * a) % C]) @ h for c in chans])
    return y, np.abs(x[idx]) @ np.abs(h)


def bound_factor(T, C):
    """P + 8 + 7 log2 C"""
    return -(-int(T) // int(C)) + 8 + 7 * log2_exact(C)


def worst_ratio(y, y64, s, T, C):
    """max over channels and outputs of |y - y64| / ((P + 8 + 7 log2 C) 2^-24 S): the criterion holds iff <= 1 (an output
    whose S is 0 must be exactly 0: ratio inf otherwise)"""
    if y64.size == 0:
        return 0.0
    err = np.abs(np.asarray(y).astype(np.complex128) - y64)
    bound = np.broadcast_to(bound_factor(T, C) * U * s, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def numpy_bank(x, taps, channels, decim, *, shift=0.0, sample_index0=0, scale=None):
    """A filter bank over numpy chunks with the signature amcpy_amd.bank.FilterBank's ``compute`` takes, POSITION INDEPENDENT
    as the kernel is: a sample is mixed by element-wise float64 arithmetic, a branch is summed tap by tap in ascending q, the
    transform is summed term by term in ascending r with a coefficient that depends on (c r) mod C alone -- every operation is
    element-wise over the outputs, so an output's bits do not depend on where in a call it stands.  x: complex64 (S,) or
    integer (S, 2); -> complex64 (C, M)."""
    from amcpy_amd.ddc import _format_of, _scale_of, phase_step_of
    fmt = _format_of(x)
    step = phase_step_of(shift)
    xw = ddc_ref.widen(x, fmt, _scale_of(fmt, scale))
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    T, C, D = h.shape[0], int(channels), int(decim)
    M = ddc_ref.out_samples(xw.shape[0], T, D)
    if M == 0:
        return np.zeros((C, 0), np.complex64)
    n = np.arange((M - 1) * D + T)
    index0 = int(sample_index0)
    v = xw[n] * np.exp(2j * np.pi * ddc_ref.phases(n, (index0 * step) & MASK64, step))
    top = np.arange(M) * D + T - 1                                  # n_m
    a = (index0 % C + top) % C
    u = np.zeros((M, C), np.complex128)
    for p in range(min(C, T)):
        for k in range(p, T, C):
            u[:, p] += h[k] * v[top - k]
    w = np.exp(2j * np.pi * np.arange(C) / C)
    w[0] = 1.0
    y = np.zeros((C, M), np.complex128)
    c = np.arange(C)
    for r in range(C):
        y += w[(c * r) % C][:, None] * u[np.arange(M), (r + a) % C][None, :]
    return y.astype(np.complex64)
