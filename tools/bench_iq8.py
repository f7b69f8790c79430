#!/usr/bin/env python3
"""Resident 8-bit IQ against its widened sc16 twin, same box, alternating runs timed with HIP events.

    python tools/bench_iq8.py [--sizes 128,1024,2048,4096] [--rounds 5] [--launches 20] [--out profiles/NAME.json]

One arena of ci8 samples (Gaussian noise quantised with round(x * 30), generated in HBM) and its int16 twin, viewed as (F, N)
frames at every size: as many frames as 638 976 frames of N = 2048 (the arena of tools/bench_sc16.py).  For each (size, plan)
a round is: `launches` calls of features18_sc16 on the twin between two events, the same of features18_iq8 in chunks that
widen to 64 MiB (its first default: `default_chunk_frames` in the output), of features18_iq8 as ONE whole-arena call (its
default since), and sc16 ONCE MORE -- sc16 against itself, whose ratio is the spread a
ratio of this job can be told from.  features18_iq8 widens a chunk into a workspace (2 N bytes read, 4 N written per frame)
in front of a kernel that reads 4 N, so its rate is expected BELOW sc16's: the table says by how much, and whether the
64 MiB chunks or the whole-arena call is the faster.  bench.py is not involved."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

BENCH_FRAMES_2048 = 638_976
SCALE = 2.0 ** -7
IQ8_CHUNK_BYTES = 64 << 20


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,1024,2048,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _lib
    from amcpy_amd.features import features18_iq8, features18_sc16

    plans = {"all": None, "cumulants_13_15": [13, 15]}
    samples = BENCH_FRAMES_2048 * 2048
    g = torch.Generator(device="cuda").manual_seed(2026)
    arena8 = torch.empty((samples, 2), dtype=torch.int8, device="cuda")
    arena16 = torch.empty((samples, 2), dtype=torch.int16, device="cuda")
    step = 1 << 26
    for s0 in range(0, samples, step):                    # in parts: the temporaries stay small
        s1 = min(samples, s0 + step)
        q = (torch.randn((s1 - s0, 2), device="cuda", generator=g) * 30.0).round_().clamp_(-128, 127)
        arena8[s0:s1] = q.to(torch.int8)
        arena16[s0:s1] = arena8[s0:s1].to(torch.int16)
    rows = []
    for N in [int(t) for t in a.sizes.split(",")]:
        F = samples // N
        x8, x16 = arena8[:F * N].view(F, N, 2), arena16[:F * N].view(F, N, 2)
        out = torch.empty((F, 18), dtype=torch.float32, device="cuda")
        for p, ids in plans.items():
            runs = {"sc16": lambda: features18_sc16(x16, out=out, scale=SCALE, feature_ids=ids),
                    "iq8": lambda: features18_iq8(x8, out=out, scale=SCALE, feature_ids=ids,
                                                  chunk_frames=max(1, IQ8_CHUNK_BYTES // (8 * N))),
                    "iq8whole": lambda: features18_iq8(x8, out=out, scale=SCALE, feature_ids=ids, chunk_frames=F)}
            check = features18_sc16(x16, scale=SCALE, feature_ids=ids)      # warm, and the paths agree on this arena
            same = True
            for key in ("iq8", "iq8whole"):
                runs[key]()
                same = same and bool(((out == check) | (out.isnan() & check.isnan())).all())
            del check
            torch.cuda.synchronize()
            order = ("sc16", "iq8", "iq8whole", "sc16_again")
            t = {k: [] for k in order}
            for _ in range(a.rounds):
                for key in order:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.launches):
                        runs[key.split("_")[0]]()
                    e1.record()
                    torch.cuda.synchronize()
                    t[key].append(e0.elapsed_time(e1) * 1e-3 / a.launches)
            sec = {k: np.array(v) for k, v in t.items()}
            spread = float(np.abs(sec["sc16"] / sec["sc16_again"] - 1.0).max())
            mask = _lib.FEATURES_ALL if ids is None else _lib.feature_mask(ids)
            rows.append({"N": N, "plan": p, "frames": F, "bit_identical": same,
                         "kernel": _lib.kernel_name_iq8(N, _lib.VARIANT_AUTO, mask),
                         "default_chunk_frames": max(1, IQ8_CHUNK_BYTES // (8 * N)),
                         "sc16_frames_per_s": F / float(np.median(sec["sc16"])),
                         "iq8_frames_per_s": F / float(np.median(sec["iq8"])),
                         "iq8_whole_arena_frames_per_s": F / float(np.median(sec["iq8whole"])),
                         "ratio_iq8_over_sc16_median": float(np.median(sec["sc16"] / sec["iq8"])),
                         "ratio_iq8_whole_over_sc16_median": float(np.median(sec["sc16"] / sec["iq8whole"])),
                         "ratio_default_chunk_over_whole_median": float(np.median(sec["iq8whole"] / sec["iq8"])),
                         "sc16_vs_itself_spread": spread,
                         **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in order}})
            r = rows[-1]
            print(f"N={N:5d} {p:16s} sc16 {r['sc16_frames_per_s'] / 1e6:7.1f} M frames/s  iq8 {r['iq8_frames_per_s'] / 1e6:7.1f} "
                  f"(x{r['ratio_iq8_over_sc16_median']:.3f})  whole arena {r['iq8_whole_arena_frames_per_s'] / 1e6:7.1f} "
                  f"(x{r['ratio_iq8_whole_over_sc16_median']:.3f})  spread {spread:.4f}  identical {same}", flush=True)
        del x8, x16, out
    doc = {"what": "tools/bench_iq8.py", "rounds": a.rounds, "launches_per_round": a.launches, "scale": SCALE,
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
