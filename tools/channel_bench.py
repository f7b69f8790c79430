#!/usr/bin/env python3
"""The fading channel (amcx_channel_c64) against two yardsticks, same box, alternating runs timed with HIP events.

    python tools/channel_bench.py [--rows 16384] [--row-samples 4096] [--rounds 5] [--launches 20] [--torch-launches 1] [--out profiles/NAME.json]

64 Mi output samples by default, at a maximum Doppler of 1e-3 cycles per sample.  Cells (L paths, S sinusoids, interp_log2):
(1, 16, default), (6, 16, default), (16, 32, default), (6, 16, 0), each with and without noise; the paths are an exponential
profile one sample apart, 1 dB per path.  A round is `launches` calls of the kernel between two events, the yardsticks, and the
kernel ONCE MORE: the kernel against itself, whose ratio is the spread a ratio of this job can be told from.

  (a) the stock-PyTorch formulation of the same model: per row and path uniform phases and arrival angles (torch.rand), the
      node gains as a sum over torch.polar of the phase ramps, torch.lerp between neighbouring nodes gathered per sample, the
      delayed rows multiplied and summed over the paths, normal_ noise.  Rows are taken 2048 at a time to bound its temporaries.
  (b) the floor: amcx_probe_read_bw over the bytes the kernel reads and writes (rows x (2 row_samples + H) x 8).

Reported per cell: G samples/s, the fraction of 8 TB/s that the 16 bytes read and written per sample are, each yardstick's rate
and the ratio, and the spread.  No ratio is promised: where the kernel loses, the row says so.  bench.py is not involved."""
import argparse
import json
import math
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

HBM_BYTES_PER_S = 8.0e12
DOPPLER, SIGMA = 1e-3, 0.3
CELLS = [(1, 16, None), (6, 16, None), (16, 32, None), (6, 16, 0)]
STOCK_ROWS = 2048


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 14)
    ap.add_argument("--row-samples", type=int, default=1 << 12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--torch-launches", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _lib, channel as ch

    R, N = a.rows, a.row_samples
    lib = _lib.load()
    out = torch.empty((R, N), dtype=torch.complex64, device="cuda")
    partial = torch.empty(1 << 16, dtype=torch.float32, device="cuda")
    sigma_dev = torch.full((1,), SIGMA, dtype=torch.float32, device="cuda")
    rows = []

    def timed(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    for L, S, b in CELLS:
        profile = ch.exponential(L, 1, 1.0)
        H = profile.history
        b = ch.default_interp_log2(DOPPLER) if b is None else b
        B = 1 << b
        x = torch.view_as_complex(torch.randn((R, N + H, 2), dtype=torch.float32, device="cuda") * math.sqrt(0.5))
        moved = (R * (2 * N + H) * 8) // 16 * 16
        both = torch.empty(moved // 8, dtype=torch.complex64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        dg = [float(g) / math.sqrt(S) for g in profile.diffuse_gain]
        K = (N - 1) // B + 2
        node_at = torch.arange(K, device="cuda", dtype=torch.float32)[None, None, :] * float(B)
        k_of = (torch.arange(N, device="cuda") // B)[None, :]
        frac = ((torch.arange(N, device="cuda") % B).to(torch.float32) / B)[None, :].to(torch.complex64)     # lerp takes its operands' type

        for noise in (True, False):
            def ours():
                return ch.apply(x, profile, doppler=DOPPLER, sinusoids=S, interp_log2=b, seed=1, sigma=sigma_dev if noise else None, out=out)

            def stock():
                for r0 in range(0, R, STOCK_ROWS):
                    n = min(STOCK_ROWS, R - r0)
                    acc = torch.zeros((n, N), dtype=torch.complex64, device="cuda")
                    for l in range(L):
                        phase = torch.rand((n, S, 1), device="cuda") * (2.0 * math.pi)
                        step = torch.cos(torch.rand((n, S, 1), device="cuda") * (2.0 * math.pi)) * (2.0 * math.pi * DOPPLER)
                        angle = phase + step * node_at
                        nodes = torch.polar(torch.ones_like(angle), angle).sum(dim=1) * dg[l]            # (n, K)
                        idx = k_of.expand(n, N)
                        g = torch.lerp(torch.gather(nodes, 1, idx), torch.gather(nodes, 1, idx + 1), frac)
                        acc += g * x[r0:r0 + n, H - l:H - l + N]
                    if noise:
                        z = torch.view_as_complex(torch.empty((n, N, 2), dtype=torch.float32, device="cuda").normal_())
                        acc.add_(z, alpha=SIGMA * math.sqrt(0.5))
                    out[r0:r0 + n] = acc

            def floor():
                _lib.check(lib.amcx_probe_read_bw(both.data_ptr(), moved, partial.data_ptr(), stream))

            ours()
            torch.cuda.synchronize()
            power = float((out.abs() ** 2).mean())
            stock()
            stock_power = float((out.abs() ** 2).mean())
            order_of_runs = ["channel", "torch", "floor", "channel_again"]
            funcs = {"channel": (ours, a.launches), "channel_again": (ours, a.launches), "torch": (stock, a.torch_launches),
                     "floor": (floor, a.launches)}
            t = {k: [] for k in order_of_runs}
            for _ in range(a.rounds):
                for key in order_of_runs:
                    t[key].append(timed(*funcs[key]))
            sec = {k: np.array(v) for k, v in t.items()}
            med = float(np.median(sec["channel"]))
            tile, lds = _lib.channel_plan(L, S, b, H)
            row = {"cell": f"L={L} S={S} interp_log2={b} {'noise' if noise else 'no noise'}", "paths": L, "sinusoids": S, "interp_log2": b,
                   "history": H, "noise": noise, "doppler": DOPPLER, "rows": R, "row_samples": N, "kernel": _lib.kernel_name_channel(),
                   "tile_outputs": tile, "lds_bytes": lds, "mean_power": power, "torch_mean_power": stock_power,
                   "channel_G_samples_per_s": R * N / med / 1e9, "channel_fraction_of_8TBps": moved / med / HBM_BYTES_PER_S,
                   "channel_vs_itself_spread": float(np.abs(sec["channel"] / sec["channel_again"] - 1.0).max()),
                   "torch_G_samples_per_s": R * N / float(np.median(sec["torch"])) / 1e9,
                   "read_bw_G_samples_per_s": R * N / float(np.median(sec["floor"])) / 1e9,
                   "read_bw_TB_per_s": moved / float(np.median(sec["floor"])) / 1e12,
                   "ratio_channel_over_torch_median": float(np.median(sec["torch"] / sec["channel"])),
                   "ratio_channel_over_read_bw_median": float(np.median(sec["floor"] / sec["channel"])),
                   **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in order_of_runs}}
            rows.append(row)
            print(f"{row['cell']:38s} channel {row['channel_G_samples_per_s']:7.2f} G samples/s ({100 * row['channel_fraction_of_8TBps']:5.1f} % of 8 TB/s)  "
                  f"torch {row['torch_G_samples_per_s']:7.2f} x{row['ratio_channel_over_torch_median']:.2f}  read {row['read_bw_G_samples_per_s']:7.2f} "
                  f"x{row['ratio_channel_over_read_bw_median']:.2f}  spread {row['channel_vs_itself_spread']:.4f}  power {power:.3f} / {stock_power:.3f}",
                  flush=True)
            if a.out:                                          # after every cell: a cut-off run keeps what it measured
                doc = {"what": "tools/channel_bench.py", "rounds": a.rounds, "launches_per_round": a.launches,
                       "torch_launches_per_round": a.torch_launches, "sigma": SIGMA, "doppler": DOPPLER,
                       "device": torch.cuda.get_device_name(0), "rows": rows}
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
        del x, both
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
