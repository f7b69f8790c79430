"""The numpy reference of the waveform generator (include/amcx.h, amcx_synth_c64; ABI 16.2) and the criterion it is held to.

EVERY INTEGER of the contract comes from tests/train_ref.philox4x32_10 with Python or uint64 arithmetic and is therefore exact:
the row words (phase0_r, step_r, tau_r), the symbol indices, the noise words (u, the noise angle), t_n, p_n, k_n and phi.  From
those integers ``generate`` evaluates s, v, z and out in float64:

    s64[n]   = sum_q g[p_n + q U] a[k_n - q]                  S[n] = sum_q |g| |a|
    v64[n]   = s64[n] exp(2 pi j phi / 2^64)
    z64[n]   = sigma sqrt(-ln u) exp(2 pi j w2 / 2^32)        u = ((w1 >> 8) + 1) 2^-24
    out64[n] = v64[n] + z64[n]

THE CRITERION per output: |out - out64| <= (P + 8) 2^-24 S + B 2^-24 sigma sqrt(-ln u) + 2^-24 |out64|.
  * the first term is the resampler's derived bound (tests/resample_ref.py): P roundings of the sum and 8 x 2^-24 per term for a
    mixed sample.  There the mixer stands in front of the filter, here behind it; it is linear in the sample, so the 8 |g||a| per
    term cover the mixed SUM as they cover the mixed terms.
  * B is derived from the operations the kernel uses for z = (sigma * sqrtf(0 - logf(u))) * mixer(w2), in units of 2^-24 relative
    to sigma sqrt(-ln u) (one ulp is at most 2 x 2^-24 of its value, half an ulp at most 1 x 2^-24):
      logf         the device library's float32 logarithm.  AMD's table gives it 1 ulp; the library is built to the OpenCL rule,
                   3 ulp, which is what is taken here: 6 x 2^-24 relative on ln u (0 - ln u is exact), and the square root halves
                   a relative error ............................................................................ 3
      sqrtf        correctly rounded ................................................................................. 1
      sigma * .    one product ....................................................................................... 1
      mixer(w2)    the down-converter's mixer on an exact angle: under 2.5 x 2^-24 in magnitude (tests/resample_ref.py) ...... 2.5
      amp * w      one product per component, each within 2^-24 of its value: 2^-24 amp in magnitude ....................... 1
    8.5 in the first order; the products of two of those errors are below 2^-24 of that, and B = 9 holds them.  Not fitted to a run.
  * the last term is the one float32 addition per component.
Where sigma == 0 the noise term is 0 and out must equal the mixed sum within the first and last terms; where order == 0 and
sigma == 0 every output must be exactly 0."""
import numpy as np

from tests.train_ref import philox4x32_10

M32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1
EPS = 2.0 ** -24
B_NOISE = 9.0
RANDOM_PHASE, RANDOM_TIMING = 1, 2
STREAM_ROW, STREAM_SYMBOLS, STREAM_NOISE = 0, 1, 2


def key_of(seed):
    return int(seed) & M32, (int(seed) >> 32) & M32


def words(seed, stream, j, r):
    """Philox(counter(stream, j, r)) for an array (or one) j < 2^60 and one absolute row r -> four uint32 arrays"""
    j = np.asarray(j, dtype=np.uint64)
    r = int(r) & MASK64
    c1 = (np.uint64(int(stream) << 28) | (j >> np.uint64(32))).astype(np.uint64)
    return philox4x32_10((j & np.uint64(M32), c1, np.uint64(r & M32), np.uint64(r >> 32)), key_of(seed))


def mulhi32(x, m):
    return (np.asarray(x, dtype=np.uint64) * np.uint64(int(m))) >> np.uint64(32)


def row_params(seed, r, U, *, phase_step=0, cfo_max=0, flags=RANDOM_PHASE | RANDOM_TIMING, tau0=0):
    """(phase0_r, step_r, tau_r) as Python integers"""
    W = [int(w) for w in words(seed, STREAM_ROW, 0, r)]
    phase0 = (W[0] << 32) if flags & RANDOM_PHASE else 0
    w1 = W[1] - (1 << 32) if W[1] >= 1 << 31 else W[1]                     # (int32)W[1]
    step = (int(phase_step) + w1 * int(cfo_max)) & MASK64
    tau = (W[2] * int(U)) >> 32 if flags & RANDOM_TIMING else int(tau0)
    return phase0, step, tau


def symbol_indices(seed, r, k, order):
    """the table index of symbols k (int array, k >= 0) of row r"""
    k = np.asarray(k, dtype=np.uint64)
    X = np.stack(words(seed, STREAM_SYMBOLS, k >> np.uint64(2), r), axis=-1)
    w = np.take_along_axis(X, (k & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]
    return mulhi32(w, order).astype(np.int64)


def noise_words(seed, r, n):
    """(w1, w2) of samples n (int array) of row r, as uint64 arrays holding 32-bit words"""
    n = np.asarray(n, dtype=np.uint64)
    X = np.stack(words(seed, STREAM_NOISE, n >> np.uint64(1), r), axis=-1)
    at = (np.uint64(2) * (n & np.uint64(1))).astype(np.int64)
    w1 = np.take_along_axis(X, at[..., None], axis=-1)[..., 0]
    w2 = np.take_along_axis(X, at[..., None] + 1, axis=-1)[..., 0]
    return w1.astype(np.uint64), w2.astype(np.uint64)


def uniform_of(w1):
    """u = ((w1 >> 8) + 1) 2^-24 as float64 (exact; exact in float32 too)"""
    return ((np.asarray(w1, dtype=np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * EPS


def noise64(seed, r, n, sigma):
    """(z64, sigma sqrt(-ln u)) of samples n of row r"""
    w1, w2 = noise_words(seed, r, n)
    amp = float(sigma) * np.sqrt(-np.log(uniform_of(w1)))
    return amp * np.exp(2j * np.pi * (w2.astype(np.float64) / 4294967296.0)), amp


def timing(n, U, V, T, tau):
    """(p_n, k_n, P) of samples n (int64 array, n V + tau < 2^63)"""
    P = -(-int(T) // int(U))
    t = np.asarray(n, dtype=np.int64) * int(V) + int(tau)
    return t % int(U), (P - 1) + t // int(U), P


def phi_turns(n, phase0, step):
    """phi = (phase0 + n step) mod 2^64 as (uint64 array, float64 turns)"""
    with np.errstate(over="ignore"):
        phi = np.uint64(int(phase0) & MASK64) + np.asarray(n, dtype=np.uint64) * np.uint64(int(step) & MASK64)
    return phi, phi.astype(np.float64) / 18446744073709551616.0


def symbols(seed, r, k, table):
    """a[k] as complex128 holding the table's complex64 values"""
    tab = np.asarray(table, dtype=np.complex64).astype(np.complex128)
    return tab[symbol_indices(seed, r, k, tab.shape[0])]


def generate(seed, r, n0, count, table, taps, U, V, sigma, *, phase_step=0, cfo_max=0, flags=RANDOM_PHASE | RANDOM_TIMING, tau0=0):
    """Samples n0 ... n0 + count - 1 of absolute row r.  table: `order` complex points (None or empty: the noise class).
    Returns a dict: out64, bound (the criterion), s64, v64, z64, u, phi (uint64), tau, and S."""
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    T = h.shape[0]
    order = 0 if table is None else len(table)
    phase0, step, tau = row_params(seed, r, U, phase_step=phase_step, cfo_max=cfo_max, flags=flags, tau0=tau0)
    n = np.arange(int(n0), int(n0) + int(count), dtype=np.int64)
    p, top, P = timing(n, U, V, T, tau)
    s64, S = np.zeros(n.shape[0], np.complex128), np.zeros(n.shape[0], np.float64)
    if order:
        q = np.arange(P, dtype=np.int64)
        tap = p[:, None] + q[None, :] * int(U)
        live = tap < T
        k = np.where(live, top[:, None] - q[None, :], top[:, None])
        need = np.unique(k)
        a = symbols(seed, r, need, table)[np.searchsorted(need, k)]
        hw = np.where(live, h[np.where(live, tap, 0)], 0.0)
        s64, S = (a * hw).sum(axis=1), (np.abs(a) * np.abs(hw)).sum(axis=1)
    phi, turns = phi_turns(n, phase0, step)
    v64 = np.where(phi < np.uint64(1 << 32), s64, s64 * np.exp(2j * np.pi * turns))
    z64, amp = noise64(seed, r, n, sigma)
    out64 = v64 + z64
    bound = (P + 8) * EPS * S + B_NOISE * EPS * amp + EPS * np.abs(out64)
    return dict(out64=out64, bound=bound, s64=s64, v64=v64, z64=z64, S=S, phi=phi, tau=tau, step=step, phase0=phase0,
                u=uniform_of(noise_words(seed, r, n)[0]))


def worst_ratio(out, ref):
    """max over the outputs of |out - out64| / bound: the criterion holds iff <= 1 (a bound of 0 asks for exactly out64)"""
    err = np.abs(np.asarray(out).astype(np.complex128) - ref["out64"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(ref["bound"] > 0, err / ref["bound"], np.where(err == 0, 0.0, np.inf))
    return float(ratio.max()) if ratio.size else 0.0


def numpy_generate(table, taps, U, V, n_rows, row_samples, sigma, frames_per_group, *, seed=0, row_index0=0, sample_index0=0,
                   phase_step=0, cfo_max=0, flags=RANDOM_PHASE | RANDOM_TIMING, tau0=0):
    """The call amcpy_amd.waveform's injected ``compute`` stands for, over numpy: complex64 (n_rows, row_samples), the float64
    evaluation rounded once.  sigma: one value per group of frames_per_group rows."""
    sigma = np.atleast_1d(np.asarray(sigma, dtype=np.float32))
    out = np.empty((int(n_rows), int(row_samples)), np.complex64)
    for f in range(int(n_rows)):
        out[f] = generate(seed, int(row_index0) + f, sample_index0, row_samples, table, taps, U, V, float(sigma[f // int(frames_per_group)]),
                          phase_step=phase_step, cfo_max=cfo_max, flags=flags, tau0=tau0)["out64"].astype(np.complex64)
    return out
