"""The fading multipath channel (include/amcx.h, amcx_channel_c64; ABI 16.2.1) restated in numpy, the float64 closed form of its
gains, and the bounds the GPU tests hold the kernel to.  No GPU, no torch.

THE RESTATEMENT is the header's contract operation by operation: the draws come from tests/synth_ref.words (the generator's
key and counter layout, stream 3), every mixer value from tests/psd_ref.mixer32 and every FMA from tests/psd_ref.fma32, which
give ddc_mixer's and a float32 FMA's bits; the sums are float32 additions in the stated order.  ``restate`` WITHOUT noise is
therefore what the kernel must write, compared with ``==``.

THE NOISE is the generator's: out = acc + z, one float32 addition per component, z held to tests/synth_ref's derived bound
(B_NOISE 2^-24 sigma sqrt(-ln u) for z, 2^-24 |out| for the addition) around ``noise64``.

THE CLOSED FORM ``gain64`` evaluates c_l[n] = los_gain e(phase0 + n step) + diffuse_gain sum_s e(phase0_ls + n step_ls),
e(p) = exp(2 pi j p / 2^64), at EVERY sample from the exact integer phases in float64.  ``physics_bound`` is what a one-path
Rayleigh gain with diffuse_gain = 1 / sqrt(S) may differ from it by (u = 2^-24, f_d the maximum Doppler in cycles per sample):
  * the interpolation chord.  Between two nodes B samples apart a sinusoid a e(phi0 + n step) moves through the angle
    w B <= 2 pi f_d B, and the chord of a twice differentiable curve is within max|c''| B^2 / 8 = a (w B)^2 / 8 of it.  S
    sinusoids of amplitude 1 / sqrt(S): sqrt(S) (2 pi f_d B)^2 / 8.  (B = 1: the weight f is 0 and the node is the sample -- the term
    is kept all the same: it is what the formula states.)
  * the rounding, in units of u sqrt(S) (sqrt(S) is the sum of the S amplitudes 1 / sqrt(S)).  A mixer value is within 2.5 u of
    the exact one (tests/resample_ref.py) and the angle's lower 32 bits, which the mixer drops, turn it by less than
    2 pi 2^-32 < 0.4 u: 3 u per sinusoid, S of them at 1 / sqrt(S) ............................................................ 3
    the S - 1 additions round partial sums of 2, 3, ... S terms of magnitude 1: under u S^2 / 2, times 1 / sqrt(S) ......... S / 2
    the product by diffuse_gain, the FMA that adds the line of sight, the difference of two nodes and the interpolating
    FMA: one u each of values of at most sqrt(S) ............................................................................. 4
    3 + S / 2 + 4 <= S + 8.
Together: sqrt(S) (2 pi f_d B)^2 / 8 + (S + 8) 2^-24 sqrt(S).  Not fitted to a run."""
import numpy as np

from tests import synth_ref
from tests.psd_ref import fma32, mixer32
from tests.train_ref import philox4x32_10

M32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1
EPS = 2.0 ** -24
STREAM_CHANNEL = 3
LOS_COUNTER = 512
RANDOM_PHASE = 1
MAX_PATHS, MAX_SINUSOIDS, MAX_DELAY, MAX_INTERP_LOG2 = 16, 32, 1024, 16
RECORD = np.dtype([("delay", "<i4"), ("diffuse_gain", "<f4"), ("los_gain", "<f4"), ("los_doppler_q31", "<i4")])


def records_of(paths) -> np.ndarray:
    """[(delay, diffuse_gain, los_gain, los_doppler_q31), ...] -> the 16-byte records"""
    return np.array([tuple(p) for p in paths], dtype=RECORD)


def channel_words(seed, j, r):
    """Philox(counter(3, j, r)) -> four uint32 arrays: tests/synth_ref.words for one row; for an array of rows the same counter
    layout broadcast (j < 2^32 here, so the counter's second word is the stream number alone)"""
    if np.ndim(r) == 0:
        return synth_ref.words(seed, STREAM_CHANNEL, j, r)
    r = np.asarray(r, dtype=np.uint64)
    j = np.asarray(j, dtype=np.uint64)
    return philox4x32_10((j & np.uint64(M32), np.uint64(STREAM_CHANNEL << 28), r & np.uint64(M32), r >> np.uint64(32)),
                         synth_ref.key_of(seed))


def draws(seed, r, records, S, doppler_max, flags):
    """(phase0 (..., L, S), step (..., L, S), los phase0 (..., L), los step (..., L)) as uint64, mod 2^64; r one row or an array"""
    L = len(records)
    rows = np.asarray(r, dtype=np.uint64)
    lead = rows.shape
    j = (32 * np.arange(L)[:, None] + np.arange(S)[None, :]).astype(np.uint64)
    jl = (LOS_COUNTER + np.arange(L)).astype(np.uint64)
    if lead:
        X = channel_words(seed, j[None], rows.reshape(-1, 1, 1))
        XL = channel_words(seed, jl[None], rows.reshape(-1, 1))
    else:
        X, XL = channel_words(seed, j, int(r)), channel_words(seed, jl, int(r))
    phase0 = X[0].astype(np.uint64) << np.uint64(32)
    c = mixer32(X[1])[0]                                                   # the cosine of a uniform arrival angle, float32
    ci = np.trunc(c.astype(np.float64) * 2.0 ** 31).astype(np.int64)       # exact product, toward zero
    step = (ci * np.int64(int(doppler_max))).view(np.uint64)               # |ci| <= 2^31, doppler_max < 2^32: no overflow
    los0 = (XL[0].astype(np.uint64) << np.uint64(32)) if flags & RANDOM_PHASE else np.zeros(XL[0].shape, np.uint64)
    q31 = np.asarray(records["los_doppler_q31"], dtype=np.int64)
    los_step = np.broadcast_to((q31 * np.int64(int(doppler_max))).view(np.uint64), los0.shape)
    return phase0, step, los0, los_step


def _top32(phase0, step, at):
    with np.errstate(over="ignore"):
        return (phase0 + at * step) >> np.uint64(32)


def node_gains(seed, r, records, S, interp_log2, doppler_max, flags, k):
    """G_l[k] for the node indices k (int array) of one row -> (re, im) float32 (L, len(k))"""
    phase0, step, los0, los_step = draws(seed, r, records, S, doppler_max, flags)
    kB = (np.asarray(k, dtype=np.uint64) << np.uint64(int(interp_log2)))[None, :]
    dre = dim = None
    for s in range(S):                                                     # ascending s, from the s = 0 value
        re, im = mixer32(_top32(phase0[:, s, None], step[:, s, None], kB))
        dre, dim = (re, im) if s == 0 else (dre + re, dim + im)
    wre, wim = mixer32(_top32(los0[:, None], los_step[:, None], kB))
    dg = np.asarray(records["diffuse_gain"], dtype=np.float32)[:, None]
    lg = np.asarray(records["los_gain"], dtype=np.float32)[:, None]
    return fma32(lg, wre, dg * dre), fma32(lg, wim, dg * dim)


def sample_gains(seed, r, records, S, interp_log2, doppler_max, flags, n):
    """c_l[n] for the absolute samples n (ascending int array) of one row -> (re, im) float32 (L, len(n))"""
    b = int(interp_log2)
    n = np.asarray(n, dtype=np.int64)
    k = n >> b
    k0 = int(k.min())
    Gre, Gim = node_gains(seed, r, records, S, b, doppler_max, flags, np.arange(k0, int(k.max()) + 2))
    j = k - k0
    f = ((n & ((1 << b) - 1)).astype(np.float32) * np.float32(2.0 ** -b))[None, :]
    return fma32(f, Gre[:, j + 1] - Gre[:, j], Gre[:, j]), fma32(f, Gim[:, j + 1] - Gim[:, j], Gim[:, j])


def restate(x, records, S, interp_log2, doppler_max, flags, *, seed, r, n0):
    """One row without noise: x complex64 (count + H,), the outputs n0 ... n0 + count - 1 -> complex64 (count,), the kernel's bits"""
    x = np.asarray(x, dtype=np.complex64)
    delays = [int(d) for d in records["delay"]]
    H = max(delays)
    count = x.shape[0] - H
    cre, cim = sample_gains(seed, r, records, S, interp_log2, doppler_max, flags, int(n0) + np.arange(count, dtype=np.int64))
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    are = aim = None
    for l, delay in enumerate(delays):
        pr, pi = xr[H - delay:H - delay + count], xi[H - delay:H - delay + count]
        if l == 0:
            are = fma32(cre[0], pr, -(cim[0] * pi))
            aim = fma32(cre[0], pi, cim[0] * pr)
        else:
            are = fma32(cre[l], pr, are)
            are = fma32(-cim[l], pi, are)
            aim = fma32(cre[l], pi, aim)
            aim = fma32(cim[l], pr, aim)
    out = np.empty(count, np.complex64)
    out.real, out.imag = are, aim
    return out


def numpy_apply(x, records, S, interp_log2, doppler_max, flags, sigma, frames_per_group, *, seed=0, row_index0=0, sample_index0=0):
    """The call amcpy_amd.channel.apply's injected ``compute`` stands for, over numpy: x complex64 (R, count + H) ->
    (R, count).  The signal is ``restate``; the noise (sigma: None, or one value per group of frames_per_group rows) is the
    generator's float64 ``noise64`` added and rounded once."""
    x = np.asarray(x, dtype=np.complex64)
    H = int(max(records["delay"]))
    count = x.shape[1] - H
    out = np.empty((x.shape[0], count), np.complex64)
    n = int(sample_index0) + np.arange(count, dtype=np.int64)
    for f in range(x.shape[0]):
        r = (int(row_index0) + f) & MASK64
        y = restate(x[f], records, S, interp_log2, doppler_max, flags, seed=seed, r=r, n0=sample_index0)
        s = 0.0 if sigma is None else float(np.atleast_1d(np.asarray(sigma, dtype=np.float32))[f // int(frames_per_group)])
        if s != 0.0:
            y = (y.astype(np.complex128) + synth_ref.noise64(seed, r, n, s)[0]).astype(np.complex64)
        out[f] = y
    return out


def gain64(seed, r, records, S, doppler_max, flags, n):
    """The closed form at the absolute samples n, float64: complex128 (..., L, len(n)); r one row or an array of rows"""
    phase0, step, los0, los_step = draws(seed, r, records, S, doppler_max, flags)
    at = np.asarray(n, dtype=np.uint64)
    turn = lambda p0, st: np.exp(2j * np.pi * (_wrap(p0[..., None], st[..., None], at).astype(np.float64) / 2.0 ** 64))   # noqa: E731
    dg = np.asarray(records["diffuse_gain"], dtype=np.float32).astype(np.float64)[:, None]
    lg = np.asarray(records["los_gain"], dtype=np.float32).astype(np.float64)[:, None]
    return lg * turn(los0, los_step) + dg * turn(phase0, step).sum(axis=-2)


def _wrap(phase0, step, at):
    with np.errstate(over="ignore"):
        return phase0 + at * step


def physics_bound(S, doppler, interp_log2) -> float:
    """the module docstring's bound for a one-path Rayleigh gain, diffuse_gain = 1 / sqrt(S)"""
    B = 2.0 ** int(interp_log2)
    return float(np.sqrt(S) * (2.0 * np.pi * float(doppler) * B) ** 2 / 8.0 + (S + 8) * EPS * np.sqrt(S))


def noise_bound(seed, r, n, sigma, out64):
    """the generator's criterion for the noise and the one addition: B_NOISE 2^-24 sigma sqrt(-ln u) + 2^-24 |out64|"""
    return synth_ref.B_NOISE * EPS * synth_ref.noise64(seed, r, n, sigma)[1] + EPS * np.abs(out64)
