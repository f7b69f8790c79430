#!/usr/bin/env python3
"""How narrow may a frame's phase be before f2 / f3 from fp32 sums about ZERO miss the parity contract?

    python tools/phase_sum_study.py [--frames 8] [--kappa 0.05]

The N = 2048 wave kernels sum theta, |theta| and theta^2 about zero (amcx_wave_kernel.h, StatsT with kShiftedPhase =
false) and the finaliser flags the frames whose variance is below kappa_phi times the mean square (amcx_math.h,
phase_suspect); flagged frames take f2 / f3 from an fp64 sweep.  This is the CPU half of choosing kappa_phi: a numpy
restatement of the kernel's fp32 arithmetic --

  * the angle: fast_angle on the guarded envelope, operation for operation in float32 (the reciprocal and the square root
    are taken correctly rounded here; the GPU's are good to 1 ulp);
  * the summation order: lane l holds samples 128 i + 2 l + {0, 1} of rows i = 0 .. 15 and adds them in that order, 32 terms
    per lane (the square sum through a fused multiply-add: the product exact in float64, ONE rounding of the sum to
    float64 and one to float32 -- a double rounding in ~1e-9 of the additions);
  * the reduction tree: lanes l and l + 32, then l and l + 16, then the four DPP steps inside a 16-lane row (xor 1, xor 2,
    the two halves of eight, the two eights);
  * the finaliser: the predicate in float32 on the three totals, the variances in float64

-- over (a) the benchmark's frames, every modulation of the BASELINE configs[1] shape at every SNR of its grid, and (b)
synthetic frames whose phase spread sweeps std / rms from 0 to 0.5 about the centres 0, pi / 2 and just under +-pi.  The
error of f2 / f3 against oracle/iq_features_oracle.py is reported in units of the parity criterion (1e-5, plain relative),
by bins of the smaller of the two ratios var / mean square, so that the smallest kappa_phi that keeps every UNFLAGGED
frame at or below half the criterion can be read off; the share of frames a given kappa flags is printed beside it.
The GPU half (every frame of the configs[1] arena) is tests/manual/phase_flag_arena.py."""
import argparse
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from amcpy_amd import synth                                   # noqa: E402
from oracle import iq_features_oracle as orc                  # noqa: E402

N = 2048
F32 = np.float32
CRITERION = 1e-5
PI = F32(3.14159265358979323846)
TINY = F32(1.0e-37)
COEF = [F32(c) for c in (-8.109134424e-03, 4.372591574e-02, -1.118246535e-01, 1.928439466e-01, -2.781725910e-01,
                         3.989313130e-01, -6.665971279e-01, 1.999998671e+00)]


def fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, np.float64)).astype(F32)


def fast_angle(re, im):
    """amcx_math.h, fast_angle(re, im, guarded_envelope(re, im)), in float32."""
    a = np.sqrt(fma(re, re, fma(im, im, TINY)))
    den = a + np.abs(re)
    u = im * (F32(1.0) / den)
    s = u * u
    q = np.full_like(s, COEF[0])
    for c in COEF[1:]:
        q = fma(q, s, c)
    phi = q * u
    flip = np.copysign(PI, im) - phi
    return np.where(np.signbit(re), flip, phi).astype(F32)


def tree(v):
    """(F, 64) per-lane float32 sums -> (F,) totals in the kernel's order (reduce_sums)."""
    v = v[:, :32] + v[:, 32:]
    v = v[:, :16] + v[:, 16:]
    for _ in range(4):                                        # xor 1, xor 2, half mirror, mirror: neighbours pair up
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def kernel_phase_sums(x):
    """(F, 2048) complex64 -> the kernel's float32 totals (sum theta, sum theta^2, sum |theta|)."""
    th = fast_angle(x.real.astype(F32), x.imag.astype(F32))
    lanes = th.reshape(-1, N // 128, 64, 2)                   # [frame][row i][lane][b]
    st1 = np.zeros((x.shape[0], 64), F32)
    st2, sab1 = st1.copy(), st1.copy()
    for i in range(N // 128):
        for b in range(2):
            t = lanes[:, i, :, b]
            st1 = st1 + t
            st2 = fma(t, t, st2)
            sab1 = sab1 + np.abs(t)
    return tree(st1), tree(st2), tree(sab1)


def kernel_f2_f3(st1, st2, sab1):
    """The finaliser: the two ratios var / mean square in float32 (phase_suspect) and f2, f3 in float64 (finalize_features)."""
    inv = F32(1.0 / N)
    ms, mt, ma = st2 * inv, st1 * inv, sab1 * inv
    with np.errstate(all="ignore"):
        ratio = np.minimum(fma(-mt, mt, ms), fma(-ma, ma, ms)) / ms
    n = float(N)
    s1, s2, a1 = st1.astype(np.float64), st2.astype(np.float64), sab1.astype(np.float64)
    f3 = np.sqrt(np.maximum(s2 - n * (s1 / n) ** 2, 0.0) / (n - 1.0))
    f2 = np.sqrt(np.maximum(s2 - n * (a1 / n) ** 2, 0.0) / (n - 1.0))
    return ratio, f2.astype(F32), f3.astype(F32)


def benchmark_frames(n_frames):
    grid = synth.snr_grid(26)
    return np.concatenate([synth.host_block(m, float(snr), n_frames, N, seed=1000 + 10 * mi + si)
                           for mi, m in enumerate(synth.MODS6) for si, snr in enumerate(grid)]).astype(np.complex64)


def spread_frames(n_per_step, seed=3):
    """Unit-envelope (times a random amplitude) frames with Gaussian phase of a given std about a centre: std / rms of
    theta sweeps 0 ... 0.5 about the centres pi / 2 and just under +-pi; about the centre 0 the sweep is that of |theta|
    (theta itself then has rms = std)."""
    rng = np.random.default_rng(seed)
    out = []
    ratios = np.concatenate([[0.0, 1e-4, 1e-3, 1e-2], np.linspace(0.02, 0.5, 49)])
    for centre in (0.0, np.pi / 2, np.pi - 0.6, -(np.pi - 0.6)):
        for r in ratios:
            for _ in range(n_per_step):
                if centre == 0.0:                             # |theta|: a half-normal has std / rms = 0.60; offset it
                    c = 1.0
                    std = r * c / np.sqrt(max(1.0 - r * r, 1e-12))
                    th = c + std * rng.standard_normal(N)
                    th *= rng.choice([-1.0, 1.0], N)          # theta spans both signs, |theta| is narrow
                else:
                    std = r * abs(centre) / np.sqrt(max(1.0 - r * r, 1e-12))
                    th = centre + np.clip(std * rng.standard_normal(N), -0.55, 0.55)
                amp = rng.uniform(0.5, 2.0) * (1.0 + 0.1 * rng.standard_normal(N))
                out.append(amp * np.exp(1j * th))
    return np.asarray(out).astype(np.complex64)


def report(name, x, kappa):
    gold = orc.features18_batch(x).astype(F32)
    ratio, f2, f3 = kernel_f2_f3(*kernel_phase_sums(x))
    with np.errstate(all="ignore"):
        err = np.maximum(np.abs(f2.astype(np.float64) - gold[:, 1]) / np.abs(gold[:, 1]),
                         np.abs(f3.astype(np.float64) - gold[:, 2]) / np.abs(gold[:, 2])) / CRITERION
    err[~np.isfinite(err)] = np.inf                           # a zero reference: only the exact path serves
    print(f"== {name}: {x.shape[0]} frames; smallest var / mean square {np.nanmin(ratio):.3g}")
    print("   ratio bin          frames   worst error / criterion   99.9 %")
    edges = [0.0, 1e-4, 1e-3, 5e-3, 1e-2, 2e-2, 3e-2, 5e-2, 7.5e-2, 0.1, 0.15, 0.2, 0.3, 0.5, 1.01]
    for lo, hi in zip(edges[:-1], edges[1:]):
        m = (ratio >= lo) & (ratio < hi)
        if m.any():
            print(f"   [{lo:7.4f}, {hi:7.4f})  {int(m.sum()):7d}   {err[m].max():10.3g}          {np.quantile(err[m], 0.999):10.3g}")
    un = ~(ratio < kappa)
    print(f"   kappa_phi = {kappa}: flagged {int((~un).sum())} of {x.shape[0]} ({100.0 * (~un).mean():.3f} %); "
          f"worst UNFLAGGED frame {err[un].max() if un.any() else 0.0:.3g} of the criterion (wanted: <= 0.5)")
    return err[un].max() if un.any() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8, help="frames per (modulation, SNR) cell of the benchmark's shape")
    ap.add_argument("--per-step", type=int, default=4, help="synthetic frames per (centre, spread) step")
    ap.add_argument("--kappa", type=float, default=0.05)
    a = ap.parse_args()
    worst = max(report("benchmark shape: 6 modulations x 26 SNR", benchmark_frames(a.frames), a.kappa),
                report("phase-spread sweep, std / rms 0 ... 0.5", spread_frames(a.per_step), a.kappa))
    print(f"worst unflagged frame over both sets: {worst:.3g} of the criterion")
    return 0 if worst <= 0.5 else 1


if __name__ == "__main__":
    sys.exit(main())
