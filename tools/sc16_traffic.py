#!/usr/bin/env python3
"""HBM traffic of the N = 2048 sc16 18-feature kernel from `rocprofv3 --pmc` passes, each a run of its own with no tracing
beside it (gfx950 cannot collect FETCH_SIZE and WRITE_SIZE in one pass: "Request exceeds the capabilities of the hardware"):

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR/fetch -- python tools/sc16_traffic.py run
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d DIR/write -- python tools/sc16_traffic.py run
    python tools/sc16_traffic.py summarise DIR [OUT.json]

`run` launches the sc16 kernel and, beside it, the complex64 kernel on the widened twin of the same arena (Gaussian noise,
26 x 4096 frames); `summarise` reads the counter CSVs: bytes per frame of each kernel over its algorithmic bytes
(sc16: 4 N + 72, complex64: 8 N + 72).  FETCH_SIZE / WRITE_SIZE count KiB; FETCH_SIZE counts 64 B per 128-B request on wide
coalesced reads (tools/prof_summary.py doubles it for the complex64 kernels' 16-byte-per-lane loads): both the raw and the
doubled figure are given, and the complex64 kernel measured beside it says which applies to it on this box."""
import csv
import glob
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
N, FRAMES, LAUNCHES = 2048, 26 * 4096, 4


def run() -> int:
    import torch
    from amcpy_amd.features import features18, features18_sc16
    g = torch.Generator(device="cuda").manual_seed(7)
    x16 = (torch.randn((FRAMES, N, 2), device="cuda", generator=g) * 2048.0).round_().clamp_(-32768, 32767).to(torch.int16)
    x64 = torch.view_as_complex(x16.to(torch.float32) * 2.0 ** -15)
    out = torch.empty((FRAMES, 18), dtype=torch.float32, device="cuda")
    for _ in range(LAUNCHES):
        features18_sc16(x16, out=out)
        features18(x64, out=out)
    torch.cuda.synchronize()
    return 0


def summarise(directory: str, out=None) -> int:
    acc, seen = {}, {}
    for f in glob.glob(directory + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"].split("(")[0]
            if "features18_wave" not in k:
                continue
            acc.setdefault(k, {}).setdefault(r["Counter_Name"], 0.0)
            acc[k][r["Counter_Name"]] += float(r["Counter_Value"])
            seen.setdefault(k, {}).setdefault(r["Counter_Name"], set()).add(r["Dispatch_Id"])
    doc = {"what": "tools/sc16_traffic.py: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE, a run each, no tracing", "n": N,
           "frames_per_launch": FRAMES, "kernels": {}}
    for k, v in sorted(acc.items()):
        per = {c: max(1, len(ids)) for c, ids in seen[k].items()}      # dispatches of this kernel in each counter's pass
        n = per.get("FETCH_SIZE", 1)
        sc16 = "sc16" in k
        algo = (4 if sc16 else 8) * N + 72
        fetch, write = v.get("FETCH_SIZE", 0.0) * 1024 / n, v.get("WRITE_SIZE", 0.0) * 1024 / per.get("WRITE_SIZE", 1)
        doc["kernels"][k] = {"dispatches": n, "fetch_size_bytes_per_launch_raw": fetch, "write_bytes_per_launch": write,
                             "algorithmic_bytes_per_frame_value": algo,
                             "ratio_to_algorithmic_fetch_raw": (fetch + write) / FRAMES / algo,
                             "ratio_to_algorithmic_fetch_doubled": (2 * fetch + write) / FRAMES / algo}
    print(json.dumps(doc, indent=1))
    if out:
        Path(out).write_text(json.dumps(doc, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "summarise":
        sys.exit(summarise(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None))
    sys.exit(run())
