#!/usr/bin/env python3
"""Feature-subset plans against the 18-feature kernel, same box, alternating runs timed with HIP events.

    python tools/bench_subsets.py [--sizes 128,...,4096] [--reps 5] [--out profiles/NAME.json]

One synthetic arena of the benchmark's bytes (638 976 frames at N = 2048: complex Gaussian noise, generated in HBM) is viewed
as (F, N) frames at every size.  For each size the three kernels -- the 18-feature kernel (mask AMCX_FEATURES_ALL), the
no-spectral plan (AMCX_FEATURES_NO_SPECTRAL) and the cumulants plan (AMCX_FEATURES_CUMULANTS) -- run in turn, `reps` rounds,
one warm launch each first; a launch is timed alone between two events.  Reported per (size, plan): the median time,
frames/s and the fraction of the 8 TB/s HBM roofline at the algorithmic 8 N + 72 bytes per frame, and the speed-up over
the 18-feature kernel of the same round.  bench.py is not involved."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

BENCH_FRAMES_2048 = 638_976
HBM_BYTES_PER_S = 8.0e12


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256,512,1024,2048,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _lib
    from amcpy_amd.features import features18

    lib = _lib.load()
    plans = {"all": _lib.FEATURES_ALL, "no_spectral": _lib.FEATURES_NO_SPECTRAL, "cumulants": _lib.FEATURES_CUMULANTS}
    samples = BENCH_FRAMES_2048 * 2048
    g = torch.Generator(device="cuda").manual_seed(2026)
    arena = torch.complex(torch.randn(samples, device="cuda", generator=g),
                          torch.randn(samples, device="cuda", generator=g)).to(torch.complex64)
    rows = []
    for N in [int(t) for t in a.sizes.split(",")]:
        F = samples // N
        x = arena[:F * N].view(F, N)
        out = torch.empty((F, 18), dtype=torch.float32, device="cuda")
        names = {p: _lib.kernel_name_subset(N, _lib.VARIANT_AUTO, m) for p, m in plans.items()}
        times = {p: [] for p in plans}
        for p, m in plans.items():                       # warm: one launch of every kernel
            features18(x, out=out, feature_ids=None if p == "all" else [j + 1 for j in range(18) if (m >> j) & 1])
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for p, m in plans.items():
                ids = None if p == "all" else [j + 1 for j in range(18) if (m >> j) & 1]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                features18(x, out=out, feature_ids=ids)
                e1.record()
                torch.cuda.synchronize()
                times[p].append(e0.elapsed_time(e1) * 1e-3)
        base = np.array(times["all"])
        for p in plans:
            t = np.array(times[p])
            med = float(np.median(t))
            rows.append({"N": N, "plan": p, "kernel": names[p], "frames": F, "seconds_median": med,
                         "seconds_all": [round(v, 7) for v in t.tolist()],
                         "frames_per_s": F / med, "hbm_fraction": F * (8 * N + 72) / med / HBM_BYTES_PER_S,
                         "speedup_vs_all_median": float(np.median(base / t)),
                         "never_slower": bool((t <= base * 1.005).all())})
            r = rows[-1]
            print(f"N={N:5d} {p:12s} {r['kernel']:45s} {med * 1e3:8.3f} ms  {r['frames_per_s'] / 1e6:7.1f} M frames/s  "
                  f"{r['hbm_fraction']:.3f} of 8 TB/s  x{r['speedup_vs_all_median']:.3f}", flush=True)
        del x, out
    doc = {"what": "tools/bench_subsets.py", "reps": a.reps, "device": torch.cuda.get_device_name(0), "rows": rows}
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
