#!/usr/bin/env python3
"""The host path on 8-bit IQ against sc16 and complex64: one BASELINE configs[1] modulation (26 x 4096 x 2048 frames) from
pageable host memory through HipEngine -- as int8 (I, Q) pairs (ci8), as their int16 twin (sc16) and as the widened complex64
twin -- alternating runs.

    python tools/bench_iq8_upload.py [--rounds 5] [--out profiles/NAME.json]

The yardstick is sc16 on the same box: the link carries half its bytes as ci8, so up to x2 is possible.  sc16 runs twice per
round, and sc16 against itself is the spread the comparison can be told from.  Reported per kind: frames/s, GB/s of
container bytes, the bytes that crossed the link and the phase timers of amcx_upload_stats (staging, waiting for a pinned
slot, prepare, tail), per round and the median.  The three results are compared (they must be equal rows: the scales are
2^-7 for ci8 and sc16 alike, on the same integers)."""
import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

TIMERS = ("seconds_staging", "seconds_waiting", "seconds_prepare", "seconds_tail", "seconds_native")


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
    block = np.clip(np.rint(rng.standard_normal((1 << 22, 2)) * 30.0), -128, 127).astype(np.int8)
    x8 = np.empty((F, N, 2), np.int8)                     # tiled from an 8 MB block: the rate does not depend on the values
    flat = x8.reshape(-1, 2)
    for s0 in range(0, flat.shape[0], block.shape[0]):
        n = min(block.shape[0], flat.shape[0] - s0)
        flat[s0:s0 + n] = block[:n]
    x16 = x8.astype(np.int16)
    x64 = np.empty((F, N), np.complex64)
    x64.view(np.float32).reshape(F, N, 2)[...] = x16.astype(np.float32) * np.float32(2.0 ** -7)
    eng = HipEngine(N, sc16_scale=2.0 ** -7, iq8_scale=2.0 ** -7)
    runs = {"ci8": x8, "sc16": x16, "c64": x64}
    res = {k: eng(v) for k, v in runs.items()}            # warm: slots, threads, kernels
    same = bool(np.array_equal(res["ci8"], res["sc16"], equal_nan=True) and np.array_equal(res["ci8"], res["c64"], equal_nan=True))
    order = ("sc16", "ci8", "c64", "sc16_again")
    t = {k: [] for k in order}
    timers = {k: {name: [] for name in TIMERS} for k in order}
    pcie = {}
    for _ in range(a.rounds):
        for key in order:
            kind = key.split("_")[0]
            t0 = time.perf_counter()
            eng(runs[kind])
            t[key].append(time.perf_counter() - t0)
            pcie[kind] = int(eng.stats["pcie_bytes"])
            for name in TIMERS:
                timers[key][name].append(round(float(eng.stats.get(name, 0.0)), 5))
    eng.close()
    sec = {k: np.array(v) for k, v in t.items()}
    spread = float(np.abs(sec["sc16"] / sec["sc16_again"] - 1.0).max())
    doc = {"what": "tools/bench_iq8_upload.py", "frames": F, "frame_size": N, "rounds": a.rounds, "results_equal": same}
    for kind, x in runs.items():
        med = float(np.median(sec[kind]))
        doc[kind] = {"container_bytes": int(x.nbytes), "pcie_bytes": pcie[kind], "seconds": [round(float(v), 5) for v in sec[kind]],
                     "frames_per_s_median": F / med, "container_GB_per_s_median": x.nbytes / med / 1e9,
                     "link_GB_per_s_median": pcie[kind] / med / 1e9,
                     "timers_per_round": timers[kind], "timers_median": {n: float(np.median(v)) for n, v in timers[kind].items()}}
    doc["sc16"]["seconds_again"] = [round(float(v), 5) for v in sec["sc16_again"]]
    doc["ratio_frames_per_s_ci8_over_sc16"] = float(np.median(sec["sc16"] / sec["ci8"]))
    doc["ratio_frames_per_s_ci8_over_c64"] = float(np.median(sec["c64"] / sec["ci8"]))
    doc["ratio_per_round_ci8_over_sc16"] = [round(float(v), 4) for v in sec["sc16"] / sec["ci8"]]
    doc["sc16_vs_itself_spread"] = spread
    print(json.dumps(doc, indent=1))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
