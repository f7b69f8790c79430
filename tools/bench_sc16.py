#!/usr/bin/env python3
"""sc16 kernels against the complex64 kernels of the same size and plan, same box, alternating runs timed with HIP events.

    python tools/bench_sc16.py [--sizes 128,...,4096] [--rounds 5] [--launches 20] [--out profiles/NAME.json]

One arena of sc16 samples (Gaussian noise quantised with round(x * 2048), generated in HBM) and its widened complex64 twin
(float32(I) * 2^-15: the same values, so every data-dependent slow path is taken equally often), viewed as (F, N) frames
at every size: as many frames as 638 976 frames of N = 2048 take as complex64, the arena of profiles/r7_subsets_bench.json.
For each (size, plan) a round is: `launches` launches of the complex64 kernel between two events, the same of the sc16
kernel, and the complex64 kernel ONCE MORE -- complex64 against itself, whose ratio is the spread a ratio of this job can
be told from.  Reported per (size, plan): frames/s of both, the fraction of the 8 TB/s HBM roofline at the algorithmic bytes
(sc16: 4 N + 72, complex64: 8 N + 72), the ratio sc16 / complex64 per round and its median, and the spread.  bench.py is not
involved."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

BENCH_FRAMES_2048 = 638_976
HBM_BYTES_PER_S = 8.0e12
SCALE = 2.0 ** -15


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512,1024,2048,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _lib
    from amcpy_amd.features import features18, features18_sc16

    plans = {"all": _lib.FEATURES_ALL, "no_spectral": _lib.FEATURES_NO_SPECTRAL, "cumulants": _lib.FEATURES_CUMULANTS}
    samples = BENCH_FRAMES_2048 * 2048
    g = torch.Generator(device="cuda").manual_seed(2026)
    arena16 = torch.empty((samples, 2), dtype=torch.int16, device="cuda")
    arena64 = torch.empty((samples, 2), dtype=torch.float32, device="cuda")
    step = 1 << 26
    for s0 in range(0, samples, step):                    # in parts: the temporaries stay small
        s1 = min(samples, s0 + step)
        q = (torch.randn((s1 - s0, 2), device="cuda", generator=g) * 2048.0).round_().clamp_(-32768, 32767)
        arena16[s0:s1] = q.to(torch.int16)
        arena64[s0:s1] = arena16[s0:s1].to(torch.float32) * SCALE
    arena64 = torch.view_as_complex(arena64)
    rows = []
    for N in [int(t) for t in a.sizes.split(",")]:
        F = samples // N
        x16, x64 = arena16[:F * N].view(F, N, 2), arena64[:F * N].view(F, N)
        out = torch.empty((F, 18), dtype=torch.float32, device="cuda")
        for p, m in plans.items():
            ids = None if p == "all" else [j + 1 for j in range(18) if (m >> j) & 1]
            runs = {"c64": lambda: features18(x64, out=out, feature_ids=ids),
                    "sc16": lambda: features18_sc16(x16, out=out, scale=SCALE, feature_ids=ids)}
            check = features18(x64, feature_ids=ids)      # warm, and the two paths agree on this arena
            runs["sc16"]()
            same = bool(((out == check) | (out.isnan() & check.isnan())).all())
            del check
            for _ in range(3):
                runs["c64"](); runs["sc16"]()
            torch.cuda.synchronize()
            t = {"c64": [], "sc16": [], "c64_again": []}
            for _ in range(a.rounds):
                for key in ("c64", "sc16", "c64_again"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.launches):
                        runs[key.split("_")[0]]()
                    e1.record()
                    torch.cuda.synchronize()
                    t[key].append(e0.elapsed_time(e1) * 1e-3 / a.launches)
            c, s, c2 = (np.array(t[k]) for k in ("c64", "sc16", "c64_again"))
            ratio = c / s
            spread = float(np.abs(c / c2 - 1.0).max())
            ms, mc = float(np.median(s)), float(np.median(c))
            rows.append({"N": N, "plan": p, "frames": F, "bit_identical": same,
                         "kernel_sc16": _lib.kernel_name_sc16(N, _lib.VARIANT_AUTO, m),
                         "kernel_c64": _lib.kernel_name_subset(N, _lib.VARIANT_AUTO, m),
                         "sc16_frames_per_s": F / ms, "c64_frames_per_s": F / mc,
                         "sc16_hbm_fraction": F * (4 * N + 72) / ms / HBM_BYTES_PER_S,
                         "c64_hbm_fraction": F * (8 * N + 72) / mc / HBM_BYTES_PER_S,
                         "ratio_sc16_over_c64_median": float(np.median(ratio)),
                         "ratio_per_round": [round(float(v), 4) for v in ratio],
                         "c64_vs_itself_spread": spread,
                         "seconds_sc16": [round(float(v), 7) for v in s], "seconds_c64": [round(float(v), 7) for v in c],
                         "seconds_c64_again": [round(float(v), 7) for v in c2]})
            r = rows[-1]
            print(f"N={N:5d} {p:12s} sc16 {r['sc16_frames_per_s'] / 1e6:7.1f} M frames/s ({r['sc16_hbm_fraction']:.3f} of 8 TB/s)  "
                  f"c64 {r['c64_frames_per_s'] / 1e6:7.1f} ({r['c64_hbm_fraction']:.3f})  ratio x{r['ratio_sc16_over_c64_median']:.3f}  "
                  f"spread {spread:.4f}  identical {same}", flush=True)
        del x16, x64, out
    doc = {"what": "tools/bench_sc16.py", "rounds": a.rounds, "launches_per_round": a.launches, "scale": SCALE,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    try:
        sys.path.insert(0, str(REPO / "tools"))
        import codeobj_gate
        doc["code_object"] = codeobj_gate.digests(_lib.LIB_PATH)
    except Exception as exc:                              # (the digest needs the LLVM tools of a ROCm install)
        doc["code_object"] = f"unavailable: {exc}"
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
