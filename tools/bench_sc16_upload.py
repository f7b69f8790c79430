#!/usr/bin/env python3
"""The host path on sc16 against complex64: one BASELINE configs[1] modulation (26 x 4096 x 2048 frames) from pageable host
memory through HipEngine, once as int16 (I, Q) pairs and once as the widened complex64 twin, alternating runs.

    python tools/bench_sc16_upload.py [--rounds 5] [--out profiles/NAME.json]

Reported per kind: GB/s of container bytes, frames/s, the bytes that crossed the link (upload_stats), per round and the
median; complex64 runs twice per round, and complex64 against itself is the spread the comparison can be told from.  The
two results are compared (the sc16 rows must equal the complex64 rows)."""
import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    from amcpy_amd.feature_extraction import HipEngine

    S, K, N = 26, 4096, 2048
    F = S * K
    rng = np.random.default_rng(2026)
    block = np.clip(np.rint(rng.standard_normal((1 << 22, 2)) * 2048.0), -32768, 32767).astype(np.int16)
    x16 = np.empty((F, N, 2), np.int16)                   # tiled from a 16 MB block: the rate does not depend on the values
    flat = x16.reshape(-1, 2)
    for s0 in range(0, flat.shape[0], block.shape[0]):
        n = min(block.shape[0], flat.shape[0] - s0)
        flat[s0:s0 + n] = block[:n]
    x64 = np.empty((F, N), np.complex64)
    x64.view(np.float32).reshape(F, N, 2)[...] = x16.astype(np.float32) * np.float32(2.0 ** -15)
    eng = HipEngine(N)
    runs = {"sc16": x16, "c64": x64}
    res = {k: eng(v) for k, v in runs.items()}            # warm: slots, threads, kernels
    same = bool(np.array_equal(res["sc16"], res["c64"], equal_nan=True))
    t = {"c64": [], "sc16": [], "c64_again": []}
    pcie = {}
    for _ in range(a.rounds):
        for key in ("c64", "sc16", "c64_again"):
            kind = key.split("_")[0]
            t0 = time.perf_counter()
            eng(runs[kind])
            t[key].append(time.perf_counter() - t0)
            pcie[kind] = int(eng.stats["pcie_bytes"])
    eng.close()
    c, s, c2 = (np.array(t[k]) for k in ("c64", "sc16", "c64_again"))
    spread = float(np.abs(c / c2 - 1.0).max())
    doc = {"what": "tools/bench_sc16_upload.py", "frames": F, "frame_size": N, "rounds": a.rounds, "results_equal": same,
           "sc16": {"container_bytes": int(x16.nbytes), "pcie_bytes": pcie["sc16"], "seconds": [round(float(v), 5) for v in s],
                    "frames_per_s_median": F / float(np.median(s)), "container_GB_per_s_median": x16.nbytes / float(np.median(s)) / 1e9},
           "c64": {"container_bytes": int(x64.nbytes), "pcie_bytes": pcie["c64"], "seconds": [round(float(v), 5) for v in c],
                   "seconds_again": [round(float(v), 5) for v in c2],
                   "frames_per_s_median": F / float(np.median(c)), "container_GB_per_s_median": x64.nbytes / float(np.median(c)) / 1e9},
           "ratio_frames_per_s_sc16_over_c64": float(np.median(c / s)), "ratio_per_round": [round(float(v), 4) for v in c / s],
           "c64_vs_itself_spread": spread}
    doc["condition_sc16_not_slower_than_c64_beyond_spread"] = bool(doc["ratio_frames_per_s_sc16_over_c64"] >= 1.0 - spread)
    print(json.dumps(doc, indent=1))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
