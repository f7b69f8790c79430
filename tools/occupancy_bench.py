#!/usr/bin/env python3
"""Occupancy detection (ABI 14) on resident data: the row-power kernel against the read probe and stock PyTorch, and the
route "power, detect, gather, features of the occupied cells" against "features of every cell", same box, alternating runs
timed with HIP events.

    python tools/occupancy_bench.py [--rows 638976] [--rounds 5] [--launches 20] [--torch-launches 2]
                                    [--channels 64] [--frames 4096] [--out profiles/NAME.json]

POWER.  One resident arena of `rows` x 2048 complex64 samples, read as rows of 2048, of 128 and of 32768 (the same bytes).  A
round is `launches` calls of amcx_row_power_c64 between two events, then amcx_probe_read_bw over the same buffer (the same
bytes, the same 16-byte non-temporal loads, four adds per load instead of four FMAs, no tree, no store per row), the probe
once more (the spread a ratio to it can be told from), stock PyTorch `(x.real ** 2 + x.imag ** 2).sum(-1)`, and the kernel
once more (its own spread).

ROUTE.  A (channels x frames) grid of N = 2048 cells of unit-power noise; a planted share f of the channels carries 20 dB more.
f = 1 / 16 and 1 / 4 are detected at the defaults (6 dB over the rank-0.25 floor).  f = 1 has no free channel, which the
detector's assumption excludes: there EVERY cell is made to pass with threshold_db = -3, so the route pays for the power pass,
the detection and a gather of everything before it computes what today's route computes at once.  Timed per f: today's route
(features18 on every cell); the new route (row_power, detect with its count read-back, gather_rows, features18 on the
occupied cells); and the PyTorch plumbing between the same two kernels (kthvalue, nonzero, index_select).  bench.py is not
involved: the feature kernels are byte-identical to the parent's (profiles/r21_occupancy_codeobj_kernels.txt)."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=638976, help="rows of 2048 samples in the arena (a multiple of 16)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--route-launches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _lib, occupancy
    from amcpy_amd.features import features18

    lib = _lib.load()
    doc = {"what": "tools/occupancy_bench.py", "rounds": a.rounds, "launches_per_round": a.launches,
           "torch_launches_per_round": a.torch_launches, "device": torch.cuda.get_device_name(0), "power": [], "route": []}

    def save():
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")

    def timed(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    def rounds(funcs):
        t = {k: [] for k in funcs}
        for _ in range(a.rounds):
            for k, (f, n) in funcs.items():
                t[k].append(timed(f, n))
        return {k: np.array(v) for k, v in t.items()}

    # ---- the power kernel -------------------------------------------------------------------------------------------------
    g = torch.Generator(device="cuda").manual_seed(2026)
    arena = torch.view_as_complex(torch.randn((a.rows * 2048, 2), device="cuda", generator=g))
    n_bytes = arena.numel() * 8
    partial = torch.empty((4096,), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for N in (2048, 128, 32768):
        x = arena.view(-1, N)
        R = x.shape[0]
        out = torch.empty((R,), dtype=torch.float32, device="cuda")

        def ours():
            _lib.check(lib.amcx_row_power_c64(x.data_ptr(), R, N, N, out.data_ptr(), stream))

        def probe():
            _lib.check(lib.amcx_probe_read_bw(arena.data_ptr(), n_bytes, partial.data_ptr(), stream))

        def stock():
            return (x.real ** 2 + x.imag ** 2).sum(-1)

        ours()
        ref = stock()
        torch.cuda.synchronize()
        rel = float(((out - ref).abs() / ref).max())
        del ref
        torch.cuda.empty_cache()
        sec = rounds({"power": (ours, a.launches), "probe": (probe, a.launches), "probe_again": (probe, a.launches),
                      "torch": (stock, a.torch_launches), "power_again": (ours, a.launches)})
        med = {k: float(np.median(v)) for k, v in sec.items()}
        row = {"N": N, "rows": R, "bytes": n_bytes, "kernel": _lib.kernel_name_occupancy(0),
               "power_TB_per_s": n_bytes / med["power"] / 1e12, "probe_TB_per_s": n_bytes / med["probe"] / 1e12,
               "torch_TB_per_s": n_bytes / med["torch"] / 1e12,
               "ratio_power_over_probe_median": float(np.median(sec["probe"] / sec["power"])),
               "ratio_power_over_torch_median": float(np.median(sec["torch"] / sec["power"])),
               "power_vs_itself_spread": float(np.abs(sec["power"] / sec["power_again"] - 1.0).max()),
               "probe_vs_itself_spread": float(np.abs(sec["probe"] / sec["probe_again"] - 1.0).max()),
               "max_relative_difference_to_torch": rel,
               **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in sec}}
        doc["power"].append(row)
        print(f"power N={N:5d}: {row['power_TB_per_s']:.3f} TB/s, probe {row['probe_TB_per_s']:.3f} TB/s (x{row['ratio_power_over_probe_median']:.3f}, "
              f"probe spread {row['probe_vs_itself_spread']:.4f}), torch {row['torch_TB_per_s']:.3f} TB/s (x{row['ratio_power_over_torch_median']:.2f}), "
              f"own spread {row['power_vs_itself_spread']:.4f}", flush=True)
        save()
        del out
    del arena
    torch.cuda.empty_cache()

    # ---- the route --------------------------------------------------------------------------------------------------------
    Cn, K, N = a.channels, a.frames, 2048
    cells = torch.view_as_complex(torch.randn((Cn * K * N, 2), device="cuda", generator=g) * (0.5 ** 0.5)).view(Cn, K, N)
    flat = cells.view(Cn * K, N)
    loud = 0
    for share, thr_db in ((1.0 / 16, 6.0), (1.0 / 4, 6.0), (1.0, -3.0)):
        want = Cn if share == 1.0 else int(round(share * Cn))
        if share < 1.0 and want > loud:                                     # channels loud ... want - 1 get their 20 dB
            cells[loud:want] *= 10.0
            loud = want
        rank, thr = occupancy.floor_rank_of(Cn, 0.25), float(occupancy.threshold_of(thr_db))

        def today():
            return features18(flat)

        def route():
            occ = occupancy.detect(occupancy.row_power(flat).view(Cn, K), floor_quantile=0.25, threshold_db=thr_db)
            return occ, features18(occupancy.gather_rows(flat, occ.rows))

        def plumbing():
            power = occupancy.row_power(flat).view(Cn, K)
            floor = torch.kthvalue(power, rank + 1, dim=0).values
            rows = (power > thr * floor[None, :]).view(-1).nonzero().view(-1)
            return rows, features18(flat.index_select(0, rows))

        occ, packed = route()
        rows_t, packed_t = plumbing()
        full = today()
        torch.cuda.synchronize()
        n_occ = int(occ.rows.shape[0])
        same = bool(torch.equal(occ.rows.long(), rows_t)) and packed.cpu().numpy().tobytes() == packed_t.cpu().numpy().tobytes() \
            and packed.cpu().numpy().tobytes() == full[occ.rows.long()].cpu().numpy().tobytes()
        del occ, packed, rows_t, packed_t, full
        torch.cuda.empty_cache()
        sec = rounds({"today": (today, a.route_launches), "route": (route, a.route_launches), "plumbing": (plumbing, a.route_launches),
                      "today_again": (today, a.route_launches)})
        med = {k: float(np.median(v)) for k, v in sec.items()}
        row = {"channels": Cn, "frames": K, "N": N, "bytes": Cn * K * N * 8, "planted_share": share, "threshold_db": thr_db,
               "occupied_cells": n_occ, "occupied_share": n_occ / (Cn * K), "routes_agree_bit_for_bit": same,
               "ms_today": med["today"] * 1e3, "ms_route": med["route"] * 1e3, "ms_plumbing": med["plumbing"] * 1e3,
               "ratio_route_over_today_median": float(np.median(sec["today"] / sec["route"])),
               "ratio_route_over_plumbing_median": float(np.median(sec["plumbing"] / sec["route"])),
               "today_vs_itself_spread": float(np.abs(sec["today"] / sec["today_again"] - 1.0).max()),
               **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in sec}}
        doc["route"].append(row)
        print(f"route share {share:.4f} ({n_occ} of {Cn * K} cells occupied, agree {same}): today {row['ms_today']:.2f} ms, "
              f"route {row['ms_route']:.2f} ms (x{row['ratio_route_over_today_median']:.2f}), plumbing {row['ms_plumbing']:.2f} ms "
              f"(route x{row['ratio_route_over_plumbing_median']:.2f}), spread {row['today_vs_itself_spread']:.4f}", flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
