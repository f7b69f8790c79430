"""The continuous-phase generator (include/amcx.h, amcx_synth_cpm_c64; ABI 16.2.2) restated in numpy.  No GPU, no torch.

EVERY INTEGER comes from tests/train_ref.philox4x32_10 through tests/synth_ref (the generator's key, counters, row draw, timing,
symbol indices and noise words) in uint64 arithmetic reduced mod 2^32, so the phase is exact:

    alpha_j = 2 idx_j - (order - 1)
    Phi[n]  = sum_{j = 0 ... k_n} alpha_j Qc(t_n - (j - P + 1) U)                 ``phi_definition``: the header's one line
            = phase_full A(k_n - cnt_n + 1) + sum_{q < cnt_n} alpha[k_n - q] phase_taps[p_n + q U]      ``phi_computed``

The carrier is the float32 mixer restatement tests/channel_ref.py uses (tests/psd_ref.mixer32, fma32) on the top 32 bits of
phase0_r + n step_r + (Phi << 32), multiplied into (1, 0) as ddc_mix does it: ``restate`` WITHOUT noise is what the kernel
must write, compared with ``==``.

THE NOISE is the generator's.  ``generate64`` evaluates exp(2 pi j p / 2^32) + z64 in float64 at the integer angle p the mixer
reads, and ``bound`` is the generator's derived criterion (tests/synth_ref.py) with the pulse term replaced by the mixer's
own error on a unit sample, per component:  2.5 x 2^-24  +  9 x 2^-24 sigma sqrt(-ln u)  +  2^-24 |out64|."""
import numpy as np

from tests import synth_ref
from tests.psd_ref import fma32, mixer32

M32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1
EPS = 2.0 ** -24
MIXER_BOUND = 2.5


def alphas(seed, r, j, order):
    """alpha_j of the symbols j (int array) of row r, as int64"""
    return 2 * synth_ref.symbol_indices(seed, r, j, order) - (int(order) - 1)


def prefix(seed, r, K, order, *, start=0, acc=0):
    """A(K) mod 2^32 from A(start) = acc by brute force (K >= start, K - start small enough to draw)"""
    if K <= start:
        return int(acc) & M32
    return (int(acc) + int(alphas(seed, r, np.arange(start, K, dtype=np.int64), order).sum())) & M32


def phi_definition(seed, r, n, order, phase_taps, phase_full, U, V, tau):
    """The header's one line, symbol by symbol from j = 0, for the samples n (small): uint64 array holding Phi mod 2^32"""
    taps = [int(v) for v in np.asarray(phase_taps, dtype=np.uint32)]
    T = len(taps)
    P = -(-T // int(U))
    out = []
    for nn in np.atleast_1d(np.asarray(n, dtype=np.int64)):
        t = int(nn) * int(V) + int(tau)
        k = (P - 1) + t // int(U)
        a = alphas(seed, r, np.arange(0, k + 1, dtype=np.int64), order)
        phi = 0
        for j in range(k + 1):
            i = t - (j - P + 1) * int(U)                                  # >= 0 for every j <= k_n
            phi += int(a[j]) * (taps[i] if i < T else int(phase_full))
        out.append(phi & M32)
    return np.asarray(out, dtype=np.uint64)


def phi_computed(seed, r, n0, count, order, phase_taps, phase_full, U, V, tau, acc_in=0):
    """The computed form for the samples n0 ... n0 + count - 1 from acc_in = A(floor(n0 V / U)) -> (Phi uint64 array mod 2^32,
    acc_out = A(floor((n0 + count) V / U)))"""
    taps = np.asarray(phase_taps, dtype=np.uint32).astype(np.uint64)
    T, U, V = taps.shape[0], int(U), int(V)
    n = int(n0) + np.arange(int(count), dtype=np.int64)
    p, top, P = synth_ref.timing(n, U, V, T, tau)
    K0, K1 = int(n0) * V // U, (int(n0) + int(count)) * V // U
    hi = max(int(top.max()) + 1, K1)
    a = alphas(seed, r, np.arange(K0, hi, dtype=np.int64), order)        # alpha_j at a[j - K0]
    A = (int(acc_in) + np.concatenate(([0], np.cumsum(a)))) & M32         # A(K) at A[K - K0]
    cnt = P - (p >= T - (P - 1) * U)
    phi = (np.uint64(int(phase_full)) * A[top - cnt + 1 - K0].astype(np.uint64)) & np.uint64(M32)
    for q in range(P):
        live = q < cnt
        al = a[np.where(live, top - q - K0, 0)] & M32                      # two's complement, mod 2^32
        tp = taps[np.where(live, p + q * U, 0)]
        phi = (phi + np.where(live, (al.astype(np.uint64) * tp) & np.uint64(M32), np.uint64(0))) & np.uint64(M32)
    return phi, int(A[K1 - K0])


def angles(seed, r, n0, count, order, phase_taps, phase_full, U, V, *, acc_in=0, phase_step=0, cfo_max=0,
           flags=synth_ref.RANDOM_PHASE | synth_ref.RANDOM_TIMING, tau0=0):
    """(p, acc_out): the uint32 angle the mixer reads at every sample -- the top 32 bits of phase0_r + n step_r + (Phi << 32)"""
    phase0, step, tau = synth_ref.row_params(seed, r, U, phase_step=phase_step, cfo_max=cfo_max, flags=flags, tau0=tau0)
    phi, acc_out = phi_computed(seed, r, n0, count, order, phase_taps, phase_full, U, V, tau, acc_in)
    n = int(n0) + np.arange(int(count), dtype=np.int64)
    carrier, _ = synth_ref.phi_turns(n, phase0, step)
    with np.errstate(over="ignore"):
        total = carrier + (phi << np.uint64(32))
    return total >> np.uint64(32), acc_out


def mix_unit(p):
    """ddc_mix((1, 0), p << 32) -> complex64: the mixer's value times (1, 0), an angle of 0 the sample itself"""
    wre, wim = mixer32(p)
    one, zero = np.float32(1.0), np.float32(0.0)
    re = fma32(one, wre, -(zero * wim))
    im = fma32(one, wim, zero * wre)
    zero_angle = np.asarray(p, dtype=np.uint64) == 0
    out = np.empty(np.shape(p), np.complex64)
    out.real, out.imag = np.where(zero_angle, one, re), np.where(zero_angle, zero, im)
    return out


def restate(seed, r, n0, count, order, phase_taps, phase_full, U, V, **kw):
    """One row without noise -> (complex64 (count,), the kernel's bits; acc_out)"""
    p, acc_out = angles(seed, r, n0, count, order, phase_taps, phase_full, U, V, **kw)
    return mix_unit(p), acc_out


def generate64(seed, r, n0, count, order, phase_taps, phase_full, U, V, sigma, **kw):
    """float64 at the exact integer angle, with the noise -> dict(out64, bound (per component), acc_out)"""
    p, acc_out = angles(seed, r, n0, count, order, phase_taps, phase_full, U, V, **kw)
    n = int(n0) + np.arange(int(count), dtype=np.int64)
    z64, amp = synth_ref.noise64(seed, r, n, sigma)
    out64 = np.exp(2j * np.pi * (p.astype(np.float64) / 4294967296.0)) + z64
    return dict(out64=out64, bound=MIXER_BOUND * EPS + synth_ref.B_NOISE * EPS * amp + EPS * np.abs(out64), acc_out=acc_out)


def worst_component_ratio(out, ref):
    """max over the outputs and both components of |out - out64| / bound"""
    d = np.asarray(out).astype(np.complex128) - ref["out64"]
    return float(np.maximum(np.abs(d.real), np.abs(d.imag)).__truediv__(ref["bound"]).max())


def numpy_generate(order, phase_taps, phase_full, U, V, n_rows, row_samples, sigma, frames_per_group, *, acc_in=None, acc_out=None,
                   seed=0, row_index0=0, sample_index0=0, phase_step=0, cfo_max=0,
                   flags=synth_ref.RANDOM_PHASE | synth_ref.RANDOM_TIMING, tau0=0):
    """The call amcpy_amd.waveform's injected ``compute`` stands for where the name is a continuous-phase one: complex64 (n_rows,
    row_samples), the signal ``restate``'s bits, the noise the float64 ``noise64`` added and rounded once.  acc_in: n_rows words or
    None (sample_index0 == 0); acc_out: an array of n_rows uint32 to fill, or None."""
    sigma = np.atleast_1d(np.asarray(sigma, dtype=np.float32))
    out = np.empty((int(n_rows), int(row_samples)), np.complex64)
    n = int(sample_index0) + np.arange(int(row_samples), dtype=np.int64)
    for f in range(int(n_rows)):
        r = (int(row_index0) + f) & MASK64
        a0 = 0 if acc_in is None else int(np.asarray(acc_in).reshape(-1)[f])
        y, a1 = restate(seed, r, sample_index0, row_samples, order, phase_taps, phase_full, U, V, acc_in=a0, phase_step=phase_step,
                        cfo_max=cfo_max, flags=flags, tau0=tau0)
        s = float(sigma[f // int(frames_per_group)])
        if s != 0.0:
            y = (y.astype(np.complex128) + synth_ref.noise64(seed, r, n, s)[0]).astype(np.complex64)
        out[f] = y
        if acc_out is not None:
            np.asarray(acc_out).reshape(-1)[f] = a1
    return out


def numpy_compute(*args, **kw):
    """an injected ``compute`` for data sets that mix linear and continuous-phase names: the first operand tells them apart"""
    if isinstance(args[0], (int, np.integer)):
        return numpy_generate(*args, **kw)
    return synth_ref.numpy_generate(*args, **kw)
