"""References for the Welch spectrogram (include/amcx.h, ABI 15; amcpy_amd/csrc/amcx_psd_kernel.h): the float64 definition,
the kernel's operation sequence restated in numpy float32 operation by operation (any nfft), the error bound derived from that
sequence, the numpy stand-ins for injected computes, and test signals.  No GPU, no torch.

THE RESTATEMENT.  numpy has no fused multiply-add; ``fma32`` gives its bits: the product of two float32 is exact in float64,
the float64 sum with the addend is corrected to ROUND TO ODD from its exact error term (TwoSum), and a round-to-odd value of
53 bits rounds to the nearest float32 as the exact value does (53 >= 2 * 24 + 2).  With it the mixer's polynomials, the
butterflies and the power are the kernel's, bit for bit: ``float32_rows`` is what the GPU test compares with ``==``.

THE BOUND (u = 2^-24, L = log2 nfft).  Every transform output X[b] is a sum over n of xw[n] times a product of at most L
twiddles, accumulated through L stages.  One stage does to every partial term: one addition or subtraction per component
(relative u on the complex magnitude), and -- on the odd branch -- one product mul(d, w): per component
|fl - exact| <= u (|b d| + |result|) <= 2 u (|a c| + |b d|) <= 2 u |d| |w|, so 2 sqrt(2) u |d| on the complex value, with a
stored twiddle within TW u of the exact one (TW = 2: the test of the table holds the mixer to it at every angle used).  A
stage therefore multiplies a term's magnitude bound by at most 1 + (1 + 2 sqrt(2) + TW) u < 1 + K u, K = 6, and
    |Xc[b] - X[b]| <= delta := ((1 + K u)^L - 1) S1 + u S1 ~ (K L + 1) u S1,     S1 = sum_n |xw[n]|
(the last u S1: xw itself is one float32 product per component; the float64 reference multiplies exactly).  The power
p = fma(im, im, re re) rounds twice: |pc - |Xc|^2| <= 2 u |Xc|^2, and | |Xc|^2 - |X|^2 | <= 2 |X| delta + delta^2.  The row sum
adds A terms in ascending order, A - 1 roundings on the longest path over non-negative partial sums:
    |P - P64| <= sum_a [2 |X_a| delta_a + delta_a^2 + 2 u (|X_a| + delta_a)^2] + (A - 1) u (1 + 2 u) sum_a (|X_a| + delta_a)^2
plus the reference's own rounding (float64 FFT: far below u).  ``bound`` evaluates it per cell from the float64 spectra.
"""
import numpy as np

from amcpy_amd import _formats
from tests import ddc_ref
from tests.bank_ref import log2_exact

U = 2.0 ** -24
K_STAGE = 6.0           # 1 (add) + 2 sqrt 2 (product) + TW, rounded up
TW_UNITS = 2.0          # |stored twiddle - exact| <= TW_UNITS * u, asserted by tests/test_psd_host.py over the whole table
FORMATS, DEFAULT_SCALE = _formats._NUMPY, _formats._DEFAULT_SCALE          # by format name: a component's numpy type, the scale


def out_rows(S: int, nfft: int, hop: int, A: int) -> int:
    return ((S - nfft) // hop + 1) // A if S >= nfft else 0


def out_rows_brute(S: int, nfft: int, hop: int, A: int) -> int:
    nseg, s = 0, 0
    while s + nfft <= S:
        nseg, s = nseg + 1, s + hop
    return nseg // A


def _segments(x, nfft, hop, A, R):
    """(R, A, nfft) view-like gather of the stream's segments."""
    idx = (np.arange(R * A)[:, None] * hop + np.arange(nfft)[None, :]).reshape(R, A, nfft)
    return np.asarray(x)[idx]


# ---- float64 ---------------------------------------------------------------------------------------------------------------
def spectra64(x, window, nfft, hop, A):
    """complex128 (R, A, nfft): the exact product w[n] x[n] of the float32 values, transformed in float64."""
    x = np.asarray(x, dtype=np.complex64)
    R = out_rows(len(x), nfft, hop, A)
    seg = _segments(x, nfft, hop, A, R).astype(np.complex128) * np.asarray(window, dtype=np.float32).astype(np.float64)[None, None, :]
    return np.fft.fft(seg, axis=-1)


def reference(x, window, nfft, hop, A):
    """P in float64, (R, nfft)."""
    X = spectra64(x, window, nfft, hop, A)
    return (X.real ** 2 + X.imag ** 2).sum(axis=1)


def bound(x, window, nfft, hop, A):
    """The module docstring's bound per cell, float64 (R, nfft)."""
    x = np.asarray(x, dtype=np.complex64)
    L = log2_exact(nfft)
    R = out_rows(len(x), nfft, hop, A)
    X = np.abs(spectra64(x, window, nfft, hop, A))
    xw = _segments(x, nfft, hop, A, R).astype(np.complex128) * np.asarray(window, dtype=np.float32).astype(np.float64)[None, None, :]
    S1 = np.abs(xw).sum(axis=-1)[:, :, None]
    delta = (((1.0 + K_STAGE * U) ** L - 1.0) + U) * S1
    big = (X + delta) ** 2
    return (2.0 * X * delta + delta ** 2 + 2.0 * U * big).sum(axis=1) + (A - 1) * U * (1.0 + 2.0 * U) * big.sum(axis=1)


def worst_fraction(P, x, window, nfft, hop, A) -> float:
    """max over cells of |P - P64| / bound: the criterion holds iff <= 1."""
    err = np.abs(np.asarray(P).astype(np.float64) - reference(x, window, nfft, hop, A))
    b = bound(x, window, nfft, hop, A)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


# ---- float32, operation by operation ------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, elementwise (finite operands)."""
    a64, b64, c64 = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a64 * b64                                         # exact: 48 bits
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)                       # s + e == p + c exactly
    bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def mixer32(p):
    """ddc_mixer (amcx_ddc_kernel.h) on uint32 angles ``p`` -> (re, im) float32: exp(2 pi j p / 2^32)."""
    p = np.asarray(p, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    q = ((p + np.uint64(0x20000000)) & np.uint64(0xFFFFFFFF)) >> np.uint64(30)
    r = ((p - (q << np.uint64(30))) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    f = np.float32
    t = r.astype(np.float32) * f(1.4629180792671596e-9)
    z = t * t
    s = fma32(z, f(-1.9515295891e-4), f(8.3321608736e-3))
    s = fma32(z, s, f(-1.6666654611e-1))
    s = fma32(t * z, s, t)
    c = fma32(z, f(2.443315711809948e-5), f(-1.388731625493765e-3))
    c = fma32(z, c, f(4.166664568298827e-2))
    c = fma32(z * z, c, fma32(z, f(-0.5), f(1.0)))
    odd = (q & np.uint64(1)) != 0
    a, b = np.where(odd, s, c), np.where(odd, c, s)
    re = np.where(((q + np.uint64(1)) & np.uint64(2)) != 0, -a, a)
    im = np.where((q & np.uint64(2)) != 0, -b, b)
    return re.astype(np.float32), im.astype(np.float32)


def twiddles32():
    """tw[k] = ddc_mixer((0 - k) << 20), k < 2048: (re, im) float32."""
    k = np.arange(2048, dtype=np.uint64)
    return mixer32(((np.uint64(1 << 32) - k) << np.uint64(20)) & np.uint64(0xFFFFFFFF))


def _mul32(dre, dim, wre, wim):
    """(fma(d.re, w.re, -(d.im * w.im)), fma(d.re, w.im, d.im * w.re))"""
    return fma32(dre, wre, -(dim * wim)), fma32(dre, wim, dim * wre)


def fft32(re, im):
    """The kernel's transform of (..., nfft) float32 planes: radix-2 decimation in frequency, every butterfly multiplying;
    returns the planes in FFT order (the kernel's bit-reversed places undone)."""
    re, im = np.array(re, dtype=np.float32), np.array(im, dtype=np.float32)
    nfft = re.shape[-1]
    L = log2_exact(nfft)
    twr, twi = twiddles32()
    lead = re.shape[:-1]
    for l in range(L):
        h = nfft >> (l + 1)
        vr, vi = re.reshape(lead + (-1, 2, h)), im.reshape(lead + (-1, 2, h))
        ur, ui, dr, di = vr[..., 0, :], vi[..., 0, :], vr[..., 1, :], vi[..., 1, :]
        wr, wi = twr[np.arange(h) * (2048 // h)], twi[np.arange(h) * (2048 // h)]
        mr, mi = _mul32(ur - dr, ui - di, np.broadcast_to(wr, ur.shape), np.broadcast_to(wi, ur.shape))
        re = np.stack([ur + dr, mr], axis=-2).reshape(lead + (nfft,))
        im = np.stack([ui + di, mi], axis=-2).reshape(lead + (nfft,))
    rev = np.array([int(format(b, f"0{L}b")[::-1], 2) for b in range(nfft)])
    return re[..., rev], im[..., rev]


def float32_rows(x, window, nfft, hop, A):
    """The kernel's rows, bit for bit: x complex64 (S,) (widened already), window float32 (nfft,) -> float32 (R, nfft)."""
    x = np.asarray(x, dtype=np.complex64)
    w = np.asarray(window, dtype=np.float32)
    R = out_rows(len(x), nfft, hop, A)
    if R == 0:
        return np.empty((0, nfft), np.float32)
    seg = _segments(x, nfft, hop, A, R)
    re, im = fft32(w[None, None, :] * seg.real.astype(np.float32), w[None, None, :] * seg.imag.astype(np.float32))
    p = fma32(im, im, re * re)
    acc = p[:, 0, :]
    for a in range(1, A):
        acc = (acc + p[:, a, :]).astype(np.float32)
    return acc


# ---- the injected computes ---------------------------------------------------------------------------------------------------
def numpy_psd(x, nfft, *, hop=None, averages=1, window=None, scale=None):
    """The ``compute`` of amcpy_amd.psd.Spectrogram: chunks as numpy (complex64 (S,) or integer (S, 2)); the float64
    reference rounded once (within the bound of the kernel's rows, not their bits)."""
    from amcpy_amd import _formats, psd
    x = np.asarray(x)
    fmt = _formats.by_plain(x.dtype).name
    hop = nfft // 2 if hop is None else hop
    w = psd.window(nfft, window or "hann") if window is None or isinstance(window, str) else np.asarray(window, np.float32)
    wide = ddc_ref.widen(x, fmt, _formats.scale_of(fmt, scale)).astype(np.complex64)
    return reference(wide, w, nfft, hop, averages).astype(np.float32)


def numpy_psd_detect(P, floor_rank: int, threshold):
    """Exact float32: P (R, bins) -> (floor (R,), mask (R, bins) bool): tests/occupancy_ref.numpy_detect, transposed."""
    from tests import occupancy_ref
    floor, mask, _ = occupancy_ref.numpy_detect(np.asarray(P, dtype=np.float32).T, floor_rank, threshold)
    return floor, np.ascontiguousarray(mask.T)


# ---- signals ---------------------------------------------------------------------------------------------------------------
def spread_signal(S: int, nfft: int, seed: int) -> np.ndarray:
    """complex64 (S,) whose spectrum's bins lie three decades apart in magnitude, so that a permuted bin cannot hide: a sum of
    nfft tones, one per bin, with magnitudes 10^(-3 ... 0) in a shuffled order and random phases, plus noise at 1e-4."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.permutation(np.linspace(-3.0, 0.0, nfft))
    spec = mag * np.exp(2j * np.pi * rng.random(nfft))
    one = np.fft.ifft(spec) * np.sqrt(nfft)
    x = np.tile(one, -(-S // nfft))[:S]
    x = x + 1e-4 * (rng.standard_normal(S) + 1j * rng.standard_normal(S))
    return x.astype(np.complex64)


PLANTED = ((0.1370, 0.03, 15.0), (-0.3011, 0.08, 12.0), (0.4000, 0.02, 18.0))     # centre, width (cycles / sample), in-band SNR dB


def synthetic_recording(S: int = 1 << 18, seed: int = 0) -> np.ndarray:
    """Unit complex noise plus three band-limited Gaussian emitters (PLANTED), the third present only in the second half:
    complex64 (S,).  An emitter is white Gaussian noise cut to its band in the frequency domain (a brick wall over the whole
    record), scaled so that its power is SNR times the noise power that falls into its band (width of the unit noise)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(S) + 1j * rng.standard_normal(S)) / np.sqrt(2.0)
    f = np.fft.fftfreq(S)
    n = np.arange(S)
    for j, (fc, width, snr_db) in enumerate(PLANTED):
        g = np.fft.fft((rng.standard_normal(S) + 1j * rng.standard_normal(S)) / np.sqrt(2.0))
        g[np.abs(f) > width / 2.0] = 0.0
        e = np.fft.ifft(g)
        e *= np.sqrt(width * 10.0 ** (snr_db / 10.0) / np.mean(np.abs(e) ** 2))
        e = e * np.exp(2j * np.pi * fc * n)
        if j == 2:
            e[:S // 2] = 0.0
        x = x + e
    return x.astype(np.complex64)


SAMPLE_RATE = 2.0e6
CAPTURE_FREQUENCIES = (100.0e6, 101.0e6)
OWN_ANNOTATION = {"core:sample_start": 5, "core:sample_count": 10, "core:comment": "the recording's own"}


def write_recording(tmp_path, x, datatype: str, name: str = "band", sample_rate=SAMPLE_RATE):
    """x complex64 -> a TWO-capture SigMF recording under tmp_path (the second capture begins at half the samples, retuned by
    1 MHz), in cf32_le, ci16_le or ci8 (integers scaled to most of their range without clipping), with one annotation of its
    own -> (stem, what the recording holds as complex64 after the reader's default scale)."""
    import json
    from pathlib import Path
    x = np.asarray(x, dtype=np.complex64)
    stem = Path(tmp_path) / name
    if datatype == "cf32_le":
        blob, held = x.tobytes(), x
    else:
        fmt, top = ("sc16", 32000.0) if datatype == "ci16_le" else ("ci8", 120.0)
        peak = float(max(np.abs(x.real).max(), np.abs(x.imag).max()))
        q = np.round(np.stack([x.real, x.imag], axis=-1) * (top / peak)).astype(FORMATS[fmt])
        blob, held = q.tobytes(), ddc_ref.widen(q, fmt, DEFAULT_SCALE[fmt]).astype(np.complex64)
    Path(str(stem) + ".sigmf-data").write_bytes(blob)
    glob = {"core:datatype": datatype, "core:version": "1.0.0"}
    if sample_rate is not None:
        glob["core:sample_rate"] = sample_rate
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps({
        "global": glob,
        "captures": [{"core:sample_start": 0, "core:frequency": CAPTURE_FREQUENCIES[0]},
                     {"core:sample_start": len(x) // 2, "core:frequency": CAPTURE_FREQUENCIES[1]}],
        "annotations": [OWN_ANNOTATION]}))
    return stem, held


def planted_bands(nfft: int, second_half: bool):
    """The planted (lo_bin, hi_bin) in signed bins, ascending, for a row of the first or the second half."""
    out = []
    for j, (fc, width, _) in enumerate(PLANTED):
        if j == 2 and not second_half:
            continue
        out.append(((fc - width / 2.0) * nfft, (fc + width / 2.0) * nfft))
    return sorted(out)
