"""References for blind carrier recovery (include/amcx.h, ABI 16.2.3; amcpy_amd/csrc/amcx_carrier_kernel.h): the contract
restated in numpy float32 operation by operation, the integer word arithmetic in Python integers, a plain float64 version of the
same estimator, and the two derived bounds (frac against float64, phase0 against the float64 atan2).  No GPU, no torch.

THE RESTATEMENT (``estimate32`` / ``apply32``) takes ``fft32``, ``mixer32`` and ``fma32`` from tests/psd_ref.py: the transform
is the spectrogram's sequence, the mixer the down-converter's.  Every field but phase0 is the kernel's, bit for bit; phase0 goes
through the device library's atan2f and is restated from the float64 atan2 of the restated Z[bin] instead.

THE phase0 BOUND (units of 2^-32 cycle, before the shift by log2 M).  w = rintf((atan2f(y, x) * C) * 2^32), C = float32(1 / 2 pi):
    atan2f     within ATAN2_ULP = 6 ulp of the exact angle a (the OpenCL rule for atan2, which the device library is built
               to): |a32 - a| <= 6 * 2^-23 |a|, |a| <= pi
    C          |C - 1 / 2 pi| = C_ERR (evaluated below), a relative 2^-24 at most
    product    one rounding, relative 2^-24;  times 2^32: exact;  rintf: 0.5
so with t = |a| / 2 pi <= 0.5:  |w - 2^32 a / 2 pi| <= 2^32 t (6 * 2^-23 + C_ERR * 2 pi + 2^-24) (1 + 2^-23) + 0.5.
The integer correction (F (N - 1)) >> lg is exact (it comes from the fields compared with ==), and a shift by log2 M of two
words d apart gives words at most d / M + 1 apart on the circle of 2^(32 - lm) (the dropped low bits).

THE frac BOUND (against ``estimate64``; u = 2^-24, L = lg).  z32 and the float64 z of the same x differ per sample by a relative
    e_0 = ((L + 2) / 2 + 3) u    power: two roundings per q, L tree levels over non-negative terms: (L + 2) u; the root halves it
                                 and rounds (u); the quotient (u); gain * x (u)
    e_k+1 = 2 e_k + 3 u          one squaring: the relative error doubles, the product adds 2 sqrt 2 u < 3 u
and the transform is linear, so with S1 = sum |z| every Z[k] is within
    delta = (((1 + K u)^L - 1) + e_lm (1 + e_lm)) S1         psd_ref's stage bound (K = psd_ref.K_STAGE) without its window term
of the float64 one.  With r = num / den (frac = -Re r): |d num| <= 2 delta, |d den| <= 4 delta, so
    |frac32 - frac64| <= (2 delta + 4 delta |r|) / (|den| - 4 delta) + 13 u |r|
the last term the float32 evaluation of the quotient itself (component differences u and 2 u, two roundings in either fma, one in
the division: 12 u |r| to first order).  It holds where both picked the same bin and neither frac is cut at 0.5."""
import numpy as np

from tests.bank_ref import log2_exact
from tests.psd_ref import K_STAGE, U, fft32, fma32, mixer32

RECORD = np.dtype([("phase_step", "<i8"), ("phase0", "<u4"), ("bin", "<i4"), ("frac", "<f4"), ("power", "<f4"), ("gain", "<f4"),
                   ("quality", "<f4")])
GAIN, FREQ, PHASE, GIVEN = 1, 2, 4, 8
ORDERS = (1, 2, 4, 8)
MASK64 = (1 << 64) - 1
ATAN2_ULP = 6.0
C_INV_2PI = np.float32(0.15915494309189535)
C_ERR = abs(float(C_INV_2PI) - 1.0 / (2.0 * np.pi))
f32 = np.float32


def tree32(q):
    """THE TREE over the last axis (a power of two long), float32: q'[i] = q[2 i] + q[2 i + 1] until one value is left."""
    q = np.asarray(q, dtype=np.float32)
    while q.shape[-1] > 1:
        q = (q[..., 0::2] + q[..., 1::2]).astype(np.float32)
    return q[..., 0]


def mul32(dre, dim, wre, wim):
    """psd_mul: (fma(d.re, w.re, -(d.im * w.im)), fma(d.re, w.im, d.im * w.re))"""
    dre, dim, wre, wim = (np.asarray(v, dtype=np.float32) for v in (dre, dim, wre, wim))
    return fma32(dre, wre, -(dim * wim)), fma32(dre, wim, dim * wre)


# ---- the integer words, in Python integers --------------------------------------------------------------------------------------
def wrap_i64(v: int) -> int:
    v &= MASK64
    return v - (1 << 64) if v >= 1 << 63 else v


def frac_word(frac) -> int:
    """F = (int64)rintf(frac 2^31): the product is exact (a power of two), rintf rounds half to even."""
    return int(np.rint(np.float32(frac) * np.float32(2.0 ** 31)))


def step_word(bin_: int, frac, N: int, order: int) -> int:
    """phase_step: step_M = bin 2^(64 - lg) + F 2^(33 - lg) as an int64, shifted right ARITHMETICALLY by log2 M."""
    lg, lm = log2_exact(N), ORDERS.index(order)
    step_m = wrap_i64(int(bin_) * (1 << (64 - lg)) + frac_word(frac) * (1 << (33 - lg)))
    return step_m >> lm                                   # Python's shift of a negative integer is arithmetic


def phase_word(w: int, frac, N: int, order: int) -> int:
    """phase0 from the angle word w: theta_M = (uint32)(w - ((F (N - 1)) >> lg)), shifted right LOGICALLY by log2 M."""
    lg, lm = log2_exact(N), ORDERS.index(order)
    theta_m = (int(w) - ((frac_word(frac) * (N - 1)) >> lg)) & 0xFFFFFFFF
    return theta_m >> lm


def angle_word64(zre, zim) -> int:
    """2^32 a / 2 pi rounded to an integer, a the float64 atan2 of the float32 components."""
    return int(np.rint(np.arctan2(float(zim), float(zre)) / (2.0 * np.pi) * 4294967296.0))


def phase0_tolerance(zre, zim, order: int) -> int:
    """The module docstring's phase0 bound for one Z[bin], in units of 2^-32 cycle AFTER the shift by log2 M."""
    t = abs(np.arctan2(float(zim), float(zre))) / (2.0 * np.pi)
    d = 4294967296.0 * t * (ATAN2_ULP * 2.0 ** -23 + C_ERR * 2.0 * np.pi + 2.0 ** -24) * (1.0 + 2.0 ** -23) + 0.5 + 0.5   # (+ 0.5: angle_word64's own rint)
    return int(np.ceil(d / order)) + 1


def phase0_distance(a: int, b: int, order: int) -> int:
    """The distance of two phase0 words on their circle of 2^(32 - lm)."""
    m = 1 << (32 - ORDERS.index(order))
    d = (int(a) - int(b)) % m
    return min(d, m - d)


# ---- float32, operation by operation --------------------------------------------------------------------------------------------
def spectrum32(x, order: int) -> dict:
    """What does not depend on the search range: x complex64 (R, N) -> ``power``, ``gain``, ``bad``, ``ure``, ``uim``, ``zsum`` and
    ``Zre``, ``Zim`` (R, N) float32 in FFT order with ``P``."""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex64))
    R, N = x.shape
    lm = ORDERS.index(order)
    assert 64 <= N <= 4096
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    with np.errstate(all="ignore"):
        power = (tree32(fma32_any(im, im, re * re)) * f32(1.0 / N)).astype(np.float32)
        bad = ~((power > 0) & (power < np.inf))
        gain = np.where(bad, f32(0), f32(1.0) / np.sqrt(np.where(bad, f32(1), power), dtype=np.float32)).astype(np.float32)
        good = ~bad
        ure, uim = (gain[:, None] * re).astype(np.float32), (gain[:, None] * im).astype(np.float32)
        zre, zim = np.where(good[:, None], ure, f32(0)), np.where(good[:, None], uim, f32(0))      # (a bad row's record is zeros)
        for _ in range(lm):
            zre, zim = mul32(zre, zim, zre, zim)
        zsum = tree32(fma32(zim, zim, zre * zre))
        Zre, Zim = fft32(zre, zim)
        P = fma32(Zim, Zim, Zre * Zre)
    return dict(power=power, gain=gain, bad=bad, ure=ure, uim=uim, zsum=zsum, Zre=Zre, Zim=Zim, P=P, N=N, order=order)


def estimate32(x, order: int, search_bins: int, spec=None) -> dict:
    """x complex64 (R, N) -> the records (RECORD; phase0 from the float64 atan2 of the restated Z[bin]) beside what they were
    made from (:func:`spectrum32`'s, which ``spec`` may hand in)."""
    spec = spectrum32(x, order) if spec is None else spec
    power, gain, bad, zsum, Zre, Zim, P, N = (spec[k] for k in ("power", "gain", "bad", "zsum", "Zre", "Zim", "P", "N"))
    assert spec["order"] == order
    R, sb, good = power.shape[0], int(search_bins), ~bad
    assert 0 <= sb <= N // 2 - 1
    rec = np.zeros(R, RECORD)
    rec["power"], rec["gain"] = power, gain
    ks = np.arange(-sb, sb + 1)
    for r in np.flatnonzero(good):
        key = P[r, ks % N].astype(np.float32)
        key = np.where(np.isnan(key), f32(-1), key)
        k = int(ks[int(np.argmax(key))])                  # argmax: the first of the largest, ks ascending
        a, b, c = ((Zre[r, (k + d) % N], Zim[r, (k + d) % N]) for d in (-1, 0, 1))
        with np.errstate(all="ignore"):
            num = (f32(c[0] - a[0]), f32(c[1] - a[1]))
            den = (f32(f32(b[0] - a[0]) + f32(b[0] - c[0])), f32(f32(b[1] - a[1]) + f32(b[1] - c[1])))
            frac = f32(-(f32(fma32(num[1], den[1], f32(num[0] * den[0]))) / f32(fma32(den[1], den[1], f32(den[0] * den[0])))))
        if not abs(frac) <= f32(0.5):
            frac = f32(0.0)
        rec["bin"][r], rec["frac"][r] = k, frac
        rec["phase_step"][r] = step_word(k, frac, N, order)
        rec["phase0"][r] = phase_word(angle_word64(b[0], b[1]), frac, N, order)
        with np.errstate(all="ignore"):
            rec["quality"][r] = f32(key.max()) / f32(f32(N) * zsum[r])
    return dict(spec, rec=rec)


def fma32_any(a, b, c):
    """fma32 where an operand may be inf or NaN (a bad row's power): the finite lanes are fma32's, the others numpy's sum."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    with np.errstate(all="ignore"):
        plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        return np.where(fin, fma32(np.where(fin, a, 0), np.where(fin, b, 0), np.where(fin, c, 0)), plain)


def apply32(x, rec, flags: int, bad=None) -> np.ndarray:
    """The output rows from GIVEN records, bit for bit: x complex64 (R, N), rec RECORD (R,) -> complex64 (R, N).  ``bad``: the rows
    an estimating call writes zeros for (a GIVEN call has none)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex64))
    R, N = x.shape
    n = np.arange(N, dtype=np.uint64)
    out = np.empty((R, N), np.complex64)
    for r in range(R):
        with np.errstate(over="ignore"):
            phi = np.zeros(N, np.uint64)
            if flags & PHASE:
                phi = phi + np.uint64(int(rec["phase0"][r]) << 32)
            if flags & FREQ:
                phi = phi + n * np.uint64(int(rec["phase_step"][r]) & MASK64)
            ang = (np.uint64(0) - phi) >> np.uint64(32)
        wre, wim = mixer32(ang)
        re, im = np.ascontiguousarray(x[r].real), np.ascontiguousarray(x[r].imag)
        with np.errstate(all="ignore"):
            if flags & GAIN:
                g = np.float32(rec["gain"][r])
                re, im = (g * re).astype(np.float32), (g * im).astype(np.float32)
            fin = np.isfinite(re) & np.isfinite(im)
            yre, yim = mul32(np.where(fin, re, 0), np.where(fin, im, 0), wre, wim)
            plain_re = (re.astype(np.float64) * wre - im.astype(np.float64) * wim).astype(np.float32)
            plain_im = (re.astype(np.float64) * wim + im.astype(np.float64) * wre).astype(np.float32)
        out[r].real, out[r].imag = np.where(fin, yre, plain_re), np.where(fin, yim, plain_im)
        if bad is not None and bad[r]:
            out[r] = 0
    return out


# ---- float64 ----------------------------------------------------------------------------------------------------------------------
def estimate64(x, order: int, search_bins: int) -> dict:
    """The same estimator in plain float64 with numpy.fft: ``bin``, ``frac``, ``cycles`` (the offset in cycles per sample of x),
    ``phase`` (cycles, one of the M), ``lead`` (the peak's power over the runner-up's inside the range, inf at sb = 0),
    and ``frac_bound`` (the module docstring's, per row)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex64)).astype(np.complex128)
    R, N = x.shape
    lg, lm, sb = log2_exact(N), ORDERS.index(order), int(search_bins)
    power = np.mean(np.abs(x) ** 2, axis=1)
    z = (x / np.sqrt(power)[:, None]) ** order
    Z = np.fft.fft(z, axis=1)
    ks = np.arange(-sb, sb + 1)
    P = np.abs(Z[:, ks % N]) ** 2
    at = np.argmax(P, axis=1)
    k = ks[at]
    rows = np.arange(R)
    a, b, c = Z[rows, (k - 1) % N], Z[rows, k % N], Z[rows, (k + 1) % N]
    num, den = c - a, (b - a) + (b - c)
    r = num / den
    frac = -r.real
    cut = ~(np.abs(frac) <= 0.5)
    frac = np.where(cut, 0.0, frac)
    srt = np.sort(P, axis=1)
    lead = srt[:, -1] / srt[:, -2] if P.shape[1] > 1 else np.full(R, np.inf)
    e = ((lg + 2) / 2.0 + 3.0) * U
    for _ in range(lm):
        e = 2.0 * e + 3.0 * U
    delta = (((1.0 + K_STAGE * U) ** lg - 1.0) + e * (1.0 + e)) * np.abs(z).sum(axis=1)
    room = np.abs(den) - 4.0 * delta
    with np.errstate(divide="ignore", invalid="ignore"):
        frac_bound = np.where(room > 0, (2.0 * delta + 4.0 * delta * np.abs(r)) / room + 13.0 * U * np.abs(r), np.inf)
    cycles = (k + frac) / (order * N)
    phase = ((np.angle(b) / (2.0 * np.pi) - frac * (N - 1) / N) / order) % (1.0 / order)
    return dict(bin=k, frac=frac, cycles=cycles, phase=phase, lead=lead, frac_bound=frac_bound, cut=cut, power=power)


def recover64(x, order: int, search_bins: int) -> np.ndarray:
    """The rows with gain, frequency and phase taken out, in float64 (complex128)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.complex64)).astype(np.complex128)
    e = estimate64(x, order, search_bins)
    n = np.arange(x.shape[1])
    rot = np.exp(-2j * np.pi * (e["phase"][:, None] + e["cycles"][:, None] * n[None, :]))
    return x / np.sqrt(e["power"])[:, None] * rot


def words_cycles(rec) -> np.ndarray:
    """phase_step of records as cycles per sample, float64."""
    return np.asarray(rec["phase_step"], dtype=np.int64).astype(np.float64) * 2.0 ** -64


def qpsk_rows(R: int, N: int, seed: int, sps: int = 4, cfo: float = 0.0, snr_db: float = 20.0, level: float = 1.0) -> tuple:
    """Random rectangular-pulse QPSK rows with a drawn offset in [-cfo, cfo), a drawn phase and noise -> (complex64 (R, N),
    the offsets)."""
    rng = np.random.default_rng(seed)
    sym = np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, (R, -(-N // sps)))))
    x = np.repeat(sym, sps, axis=1)[:, :N]
    f = rng.uniform(-cfo, cfo, R) if cfo else np.zeros(R)
    ph = rng.uniform(0, 1, R)
    x = x * np.exp(2j * np.pi * (ph[:, None] + f[:, None] * np.arange(N)[None, :]))
    x = x + 10.0 ** (-snr_db / 20.0) * (rng.standard_normal((R, N)) + 1j * rng.standard_normal((R, N))) / np.sqrt(2.0)
    return (level * x).astype(np.complex64), f
