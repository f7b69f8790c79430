"""Data on which the down-converter, the filter bank and the resampler (include/amcx.h: amcx_tune_decimate, amcx_filter_bank,
amcx_resample) are EXACT in float32, and what they must give, in int64 (tests/test_chain_exact_host.py checks all of this on
the CPU, tests/test_gpu_chain_exact.py runs it through the kernels).  numpy only; nothing here touches the GPU.

WHY.  The derived bounds of tests/ddc_ref.py, bank_ref.py and resample_ref.py grow with the tap count: one term of one output,
lost or doubled, is 2^24 / (2 T (T + 8)) times the bound -- 1900 at T = 63, 2 at T = 2048, 0.5 at P = 4096.  At the largest
shapes a tolerance cannot see a single term.  An equality can.

THE DATA.  Every I and Q is k g: k an integer, 1 <= |k| <= 128 (no component is 0), g one power of two per stream -- cf32: k
itself (g = 1); ci8: the byte; cu8: byte - 128; sc16: 256 k, so that the high byte and its sign extension carry the value
(-32768 is among them); g = 2^-7 for the three at their default scales.  Taps are integers, 1 <= |h| <= 8, as float32.  The
pre-mixer stands at quarter turns: phase_step and phase0 are multiples of 2^62, where ddc_mixer gives exactly +-1 or +-j and
ddc_mix exact swaps and sign changes, so v[n] = x[n] j^((sample_index0 + n) qs) in Gaussian integers, qs = 4 shift.  Every
product and every partial sum of any order is then an integer multiple of g of at most n_taps x 8 x 128 <= 2^22 < 2^24 units:
float32 products, sums and FMAs in ANY order are exact, and the comparison is == (so +0 equals -0).

THE CAP IS A CONDITION: ``check_cap`` asserts n_taps max|h| max|k| < 2^24 for everything ``case_data`` builds.

The bank's channel factors exp(-2 pi j c a / C) are +-1 and +-j for C <= 4: fully exact.  For C >= 8 they are irrational, but
the branch sums u_r (the taps' part) are still exact, so ONLY THE TRANSFORM ROUNDS: tests/bank_ref.py's derivation without
its P + 8 -- |y - exact| <= 7 log2 C 2^-24 S, S = sum_k |h[k]| |x[n_m - k]|.
"""
from fractions import Fraction

import numpy as np

from amcpy_amd import _formats

FORMATS = _formats.NAMES
NUMPY = {f.name: f.plain for f in _formats.TABLE}
UNIT = {"cf32": 1.0, "sc16": 2.0 ** -7, "ci8": 2.0 ** -7, "cu8": 2.0 ** -7}     # g, at the formats' default scales (asserted there)
K_MAX, H_MAX = 128, 8
U = 2.0 ** -24

# (shift in cycles per sample, sample_index0): the four quarter turns, each at a start that leaves another q0
QUARTER_TURNS = [(Fraction(0), 0), (Fraction(1, 4), 1), (Fraction(1, 2), 3), (Fraction(-1, 4), 2)]
BANK_INDEX0 = (1 << 33) + 12345             # odd, 57 mod 256: no multiple of any C (tests/test_gpu_bank.py, INDEX0)
# the bank's sample_index0 also sets the channels' phases: odd, and no multiple of C, at every one of the four
BANK_QUARTER_TURNS = [(shift, BANK_INDEX0 + 2 * i) for i, (shift, _) in enumerate(QUARTER_TURNS)]

# ---- the GPU cases: the largest tap counts, where the rounding bounds are as large as a term ---------------------------------
DDC_CASES = [(2048, 1), (2048, 5), (2047, 2), (1025, 4096)]                                              # (T, D)
RESAMPLE_CASES = [(4096, 1, 1), (4096, 2, 1), (4095, 2, 3), (4096, 3, 2), (4093, 7, 5), (4096, 256, 255), (4096, 5, 4096)]  # (T, L, D)
BANK_EXACT_CASES = [(2, 4096, 1), (2, 4096, 2), (2, 4095, 2), (4, 4096, 4), (4, 4093, 3)]                # (C, T, D)
BANK_LDS_MAX_CASE, BANK_LDS_MAX = (2, 4096, 2), 131072                                                   # amcx_bank_kernel.h
BANK_TRANSFORM_CASES = [(8, 4096, 8), (16, 4096, 16), (32, 4095, 32), (128, 4096, 96), (256, 4096, 256)]
# ---- small copies for the CPU: the same structure (odd T, L and D coprime or not, D > T, both kinds of C), (..., M) -----------
DDC_SMALL = [(8, 1, 19), (8, 5, 11), (7, 2, 13), (5, 16, 7)]                                             # (T, D, M)
RESAMPLE_SMALL = [(16, 1, 1, 19), (16, 2, 1, 19), (15, 2, 3, 13), (16, 3, 2, 13), (13, 7, 5, 23), (16, 8, 7, 19), (16, 5, 64, 7),
                  (3, 5, 3, 11)]                                                                         # (T, L, D, M)
BANK_SMALL = [(2, 16, 1, 11), (2, 16, 2, 11), (2, 15, 2, 11), (4, 16, 4, 9), (4, 13, 3, 9), (8, 16, 8, 7), (16, 37, 11, 5),
              (32, 31, 32, 3)]                                                                           # (C, T, D, M)


def check_cap(n_taps, h_max=H_MAX, k_max=K_MAX):
    """the condition under which float32 arithmetic in any order is exact on this data"""
    assert int(n_taps) * int(h_max) * int(k_max) < 1 << 24, (n_taps, h_max, k_max)


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def make_ints(S, seed=0):
    """(S, 2) int64: I and Q in -128 ... 127 without 0, both ends of the range among them"""
    rng = np.random.default_rng([77, int(S), int(seed)])
    k = rng.integers(1, K_MAX, (int(S), 2)) * rng.choice([-1, 1], (int(S), 2))          # 1 <= |k| <= 127
    k[rng.integers(0, S, max(1, S // 16)), rng.integers(0, 2, max(1, S // 16))] = -K_MAX
    assert k.min() == -K_MAX and np.abs(k).min() >= 1 and k.max() <= K_MAX - 1
    return k.astype(np.int64)


def encode(k, fmt):
    """the stream of a format whose samples stand for k g: complex64 (S,), or int16 / int8 / uint8 (S, 2)"""
    k = np.asarray(k, dtype=np.int64)
    if fmt == "cf32":
        return (k[:, 0] + 1j * k[:, 1]).astype(np.complex64)
    raw = k * (256 if fmt == "sc16" else 1) + _formats.get(fmt).zero
    info = np.iinfo(NUMPY[fmt])
    assert raw.min() >= info.min and raw.max() <= info.max
    return np.ascontiguousarray(raw.astype(NUMPY[fmt]))


def make_taps(T, seed=0):
    """T integer taps, 1 <= |h| <= 8, as float32"""
    check_cap(T)
    rng = np.random.default_rng([78, int(T), int(seed)])
    return (rng.integers(1, H_MAX + 1, int(T)) * rng.choice([-1, 1], int(T))).astype(np.float32)


def int_taps(taps):
    h = np.asarray(taps, dtype=np.float64)
    hi = np.rint(h).astype(np.int64)
    assert np.array_equal(hi, h) and np.abs(hi).min(initial=1) >= 1
    check_cap(hi.shape[0], int(np.abs(hi).max(initial=1)))
    return hi


def quarter_step(shift):
    """qs: the quarter turns per sample of a shift that is a multiple of 1 / 4"""
    qs = Fraction(shift) * 4
    assert qs.denominator == 1, shift
    return int(qs) % 4


def times_j_power(re, im, q):
    """(re + j im) j^q, q an integer array or scalar: swaps and sign changes"""
    q = np.asarray(q) % 4
    return (np.select([q == 0, q == 1, q == 2, q == 3], [re, -im, -re, im]),
            np.select([q == 0, q == 1, q == 2, q == 3], [im, re, -im, -re]))


def mix(k, shift, sample_index0):
    """v[n] = x[n] j^((sample_index0 + n) qs) in units of g: (re, im) int64"""
    k = np.asarray(k, dtype=np.int64)
    n = np.arange(k.shape[0], dtype=np.int64)
    q = ((int(sample_index0) % 4 + n) * quarter_step(shift)) % 4
    return times_j_power(k[:, 0], k[:, 1], q)


# ---------------------------------------------------------------------------------------------------------------------
# stream lengths
# ---------------------------------------------------------------------------------------------------------------------
def ddc_span(M, T, D):
    """a stream that gives exactly M outputs of the down-converter or the bank, not the shortest where D > 1"""
    return (M - 1) * D + T + min(D - 1, 3)


def phase_taps(T, L):
    return -(-int(T) // int(L))


def resample_out_samples(S, T, L, D, tau0):
    P = phase_taps(T, L)
    last = (S - P + 1) * L - 1 - tau0
    return 0 if S < P or last < 0 else last // D + 1


def resample_span(M, T, L, D, tau0):
    """(S, M'): the shortest stream that gives at least M outputs, and the M' >= M it gives (interp > decim lets several
    outputs end on one sample)"""
    S = phase_taps(T, L) + ((M - 1) * D + tau0) // L
    got = resample_out_samples(S, T, L, D, tau0)
    assert got >= M and resample_out_samples(S - 1, T, L, D, tau0) < M
    return S, got


# ---------------------------------------------------------------------------------------------------------------------
# the three operations in int64, by their definitions
# ---------------------------------------------------------------------------------------------------------------------
def ddc_exact(v, taps, D, M):
    """y[m] = sum_k h[k] v[m D + T - 1 - k], m < M: (re, im) int64.  v: (re, im) int64 of the mixed stream."""
    h = int_taps(taps)
    T, D, M = h.shape[0], int(D), int(M)
    assert v[0].shape[0] >= (M - 1) * D + T
    if D <= T:                                             # every sample of the span is read: a convolution, every D-th kept
        span = (M - 1) * D + T
        return tuple(np.convolve(c[:span], h, "valid")[::D] for c in v)
    idx = np.arange(M)[:, None] * D + (T - 1 - np.arange(T))[None, :]          # few outputs: (M, T), the sample tap k multiplies
    return tuple(c[idx] @ h for c in v)


def resample_exact(v, taps, L, D, tau0, M):
    """y[m] = sum_{q >= 0, p_m + q L < T} h[p_m + q L] v[n_m - q], t_m = m D + tau0, p_m = t_m mod L, n_m = (P - 1) + t_m // L:
    (re, im) int64.  One gather per phase: the outputs of phase p with that phase's taps h[p::L]; a phase with no tap gives 0."""
    h = int_taps(taps)
    T, L, D, tau0, M = h.shape[0], int(L), int(D), int(tau0), int(M)
    P = phase_taps(T, L)
    t = np.arange(M, dtype=np.int64) * D + tau0
    p, top = t % L, (P - 1) + t // L
    assert v[0].shape[0] > int(top.max())
    out = (np.zeros(M, np.int64), np.zeros(M, np.int64))
    for ph in np.unique(p):
        hp = h[ph::L]                                       # h[ph + q L], q = 0 ... : at most P of them, none where ph >= T
        if hp.shape[0] == 0:
            continue
        at = np.nonzero(p == ph)[0]
        if 4 * at.shape[0] > v[0].shape[0]:                 # many outputs of this phase: convolve once, pick
            for o, c in zip(out, v):
                o[at] = np.convolve(c, hp)[top[at]]
        else:
            idx = top[at][:, None] - np.arange(hp.shape[0])[None, :]
            for o, c in zip(out, v):
                o[at] = c[idx] @ hp
    return out


def bank_branch_sums(v, taps, C, D, M, sample_index0, gather=None):
    """u[m, r] = sum over the taps k with (sample_index0 + n_m - k) mod C == r of h[k] v[n_m - k], n_m = m D + T - 1: the sum
    the channels' common factor exp(-2 pi j c r / C) multiplies.  (re, im) int64 (M, C).  Few channels: one convolution per
    residue over the stream with the other residues' samples zeroed; many (or ``gather``): an (M, T) gather, M being small
    there."""
    h = int_taps(taps)
    T, C, D, M = h.shape[0], int(C), int(D), int(M)
    span = (M - 1) * D + T
    assert v[0].shape[0] >= span
    top = np.arange(M, dtype=np.int64) * D + T - 1
    a0 = int(sample_index0) % C
    out = (np.zeros((M, C), np.int64), np.zeros((M, C), np.int64))
    if C <= 8 if gather is None else not gather:
        res =(a0 + np.arange(span, dtype=np.int64)) % C
        for r in range(C):
            for o, c in zip(out, v):
                o[:, r] = np.convolve(np.where(res == r, c[:span], 0), h, "valid")[::D]
        return out
    assert 16 * M * T <= 256 << 20                          # the gather stays small
    rows = np.arange(M)
    for o, c in zip(out, v):
        prod = c[top[:, None] - np.arange(T)[None, :]] * h[None, :]              # (M, T)
        for kk in range(min(C, T)):                                             # the taps kk, kk + C, ...: one residue per output
            o[rows, (a0 + top - kk) % C] = prod[:, kk::C].sum(axis=1)
    return out


def bank_exact(u, C):
    """C <= 4: y[c, m] = sum_r u[m, r] (-j)^((c r 4 / C) mod 4): (re, im) int64 (C, M)"""
    C = int(C)
    assert C in (2, 4)
    M = u[0].shape[0]
    out = (np.zeros((C, M), np.int64), np.zeros((C, M), np.int64))
    for c in range(C):
        for r in range(C):
            re, im = times_j_power(u[0][:, r], u[1][:, r], -((c * r * (4 // C)) % 4))
            out[0][c] += re
            out[1][c] += im
    return out


def bank_float64(u, C):
    """any C: y[c, m] = sum_r u[m, r] exp(-2 pi j c r / C) with the exact u in float64 and the C-th roots of unity from a table
    indexed by the exact integer (c r) mod C: complex128 (C, M), in units of g"""
    C = int(C)
    roots = np.exp(-2j * np.pi * np.arange(C) / C)
    roots[0], roots[C // 2] = 1.0, -1.0                     # the quarter turns to the bit
    if C % 4 == 0:
        roots[C // 4], roots[3 * C // 4] = -1j, 1j
    cr = (np.arange(C)[:, None] * np.arange(C)[None, :]) % C
    return roots[cr] @ (u[0].astype(np.float64) + 1j * u[1].astype(np.float64)).T


def abs_sums(k, taps, D, M):
    """S[m] = sum_k |h[k]| |x[n_m - k]| in units of g, float64 (the scale of the bounds)"""
    h = np.abs(np.asarray(taps, dtype=np.float64))
    T = h.shape[0]
    a = np.hypot(k[:, 0].astype(np.float64), k[:, 1].astype(np.float64))[:(M - 1) * D + T]
    return np.convolve(a, h, "valid")[::D]


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
def as_float32(exact, g):
    """the complex64 an exact result (re, im) in units of g must be, and the check that it is representable"""
    re, im = exact
    assert max(int(np.abs(re).max(initial=0)), int(np.abs(im).max(initial=0))) < 1 << 24
    g = float(g)
    assert np.frexp(g)[0] == 0.5                            # a power of two
    return (re.astype(np.float64) * g).astype(np.float32), (im.astype(np.float64) * g).astype(np.float32)


def mismatches(y, exact, g):
    """how many outputs differ from the exact result in either component, compared with == (so +0 equals -0)"""
    re, im = as_float32(exact, g)
    y = np.asarray(y)
    assert y.dtype == np.complex64 and y.shape == re.shape, (y.dtype, y.shape, re.shape)
    return int(np.count_nonzero((y.real != re) | (y.imag != im)))


def without_term(exact, term, m, factor=-1):
    """a copy of an exact result with ``factor`` times the Gaussian integer ``term`` added to output m: -1 drops a term, +1
    doubles it"""
    re, im = exact[0].copy(), exact[1].copy()
    re[m] += factor * int(term[0])
    im[m] += factor * int(term[1])
    return re, im
