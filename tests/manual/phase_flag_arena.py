#!/usr/bin/env python3
"""The narrow-phase flag of the N = 2048 wave kernels (amcx_math.h, phase_suspect) over EVERY frame of the benchmark's
arena: what share of BASELINE configs[1] (6 modulations x 26 SNR x 4096 frames x 2048 samples, synth.device_frames) it
flags, and how far f2 / f3 of the flagged and of the unflagged frames are from an fp64 evaluation of the same samples,
in units of the parity criterion (1e-5, plain relative).  The GPU half of tools/phase_sum_study.py.

    python tests/manual/phase_flag_arena.py [--frames 4096] [--kappa 0.05]       (AMCX_LIB selects the library)

The reference is torch's own: angle of the samples widened to complex128, standard deviations in float64.  Which frames
the kernel flags is not in its output; the predicate is restated here on the fp64 sums (a frame within a rounding of the
threshold may fall on the other side in the kernel)."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import torch                                                  # noqa: E402
from amcpy_amd import _lib, synth                             # noqa: E402
from amcpy_amd.features import features18                     # noqa: E402

N, S = 2048, 26
CRITERION = 1e-5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--kappa", type=float, default=0.05)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library {_lib.LIB_PATH.name}, kernel {_lib.kernel_name(N)}; {len(synth.MODS6)} x {S} x {a.frames} frames of {N}; kappa_phi = {a.kappa}")
    tot = flagged_tot = 0
    worst = {True: 0.0, False: 0.0}
    errs = {True: [], False: []}
    for mi, mod in enumerate(synth.MODS6):
        x = synth.device_frames(mod, S, a.frames, N, device=dev, rank=0, mod_idx=mi).reshape(-1, N)
        got = features18(x)[:, 1:3].double()
        ref = torch.empty_like(got)
        ratio = torch.empty(x.shape[0], dtype=torch.float64, device=dev)
        for lo in range(0, x.shape[0], 8192):
            th = torch.angle(x[lo:lo + 8192].to(torch.complex128))
            ab = th.abs()
            ref[lo:lo + 8192, 0] = ab.std(dim=-1, unbiased=True)
            ref[lo:lo + 8192, 1] = th.std(dim=-1, unbiased=True)
            ms = (th * th).mean(dim=-1)
            ratio[lo:lo + 8192] = torch.minimum(ms - th.mean(dim=-1) ** 2, ms - ab.mean(dim=-1) ** 2) / ms
        err = ((got - ref).abs() / ref.abs()).max(dim=1).values / CRITERION
        flag = ratio < a.kappa
        per_snr = flag.reshape(S, a.frames).double().mean(dim=1)
        line = f"{mod:6s} flagged {int(flag.sum()):6d} of {flag.numel()} ({100.0 * flag.double().mean().item():6.3f} %)"
        for f in (False, True):
            e = err[flag == f]
            if e.numel():
                worst[f] = max(worst[f], e.max().item())
                errs[f].append(e.cpu())
                line += f"   {'flagged' if f else 'unflagged'}: worst {e.max().item():.3f}, 99.9 % {torch.quantile(e, 0.999).item():.3f}"
        print(line)
        if flag.any():
            print("       share flagged by SNR (-20 ... +30 dB):", " ".join(f"{100 * v:.1f}" for v in per_snr.tolist()))
        print(f"       smallest var / mean square of an unflagged frame {ratio[~flag].min().item():.4f}")
        tot += flag.numel()
        flagged_tot += int(flag.sum())
    print(f"ALL    flagged {flagged_tot} of {tot} ({100.0 * flagged_tot / tot:.3f} %)")
    for f in (False, True):
        if errs[f]:
            e = torch.cat(errs[f])
            print(f"       {'flagged' if f else 'unflagged'} frames: worst error {e.max().item():.3f} of the criterion, 99.9 % {torch.quantile(e[:: max(1, e.numel() // 1000000)], 0.999).item():.3f}, "
                  f"99 % {torch.quantile(e[:: max(1, e.numel() // 1000000)], 0.99).item():.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
