#!/usr/bin/env python3
"""The continuous-phase generator (amcx_synth_cpm_c64) against three yardsticks, same box, alternating runs timed with HIP events.

    python tools/cpm_bench.py [--rows 16384] [--row-samples 4096] [--long-row 4194304] [--rounds 5] [--launches 20]
                              [--torch-launches 2] [--out profiles/NAME.json]

64 Mi output samples by default in three cells -- MSK at 8 / 1, GMSK (BT 0.3 over 4 symbols) at 8 / 1, 4FSK (h = 1) at 8 / 3 --
and ONE row of 2^22 samples of GMSK at 8 / 1, which the plan cuts into segments; all at sigma = 0.3 with a drawn phase, timing
and carrier offset.  A round is `launches` calls of the generator between two events, the yardsticks, and the generator ONCE
MORE: the kernel against itself, whose ratio is the spread a ratio of this job can be told from.

  (a) the LINEAR generator's rect 8 / 1 cell (amcx_synth_c64, 16QAM) over the same rows and samples, in the same run;
  (b) the complete stock-PyTorch formulation: torch.randint symbols, 2 idx - (M - 1), cumsum, the window's symbols and the
      prefix gathered through index tensors made once outside the timing, torch.polar of phase + carrier ramp, normal_ noise;
  (c) the floor: torch.empty(...).normal_() over the same bytes, torch's own Philox Gaussian and nothing else.

Reported per cell: G samples/s, the fraction of 8 TB/s that the 8 bytes written per sample are, each yardstick's rate and the
ratio, and the spread.  No ratio is promised: where the kernel loses, the row says so.  bench.py is not involved."""
import argparse
import json
import math
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

HBM_BYTES_PER_S = 8.0e12
CELLS = [("MSK 8/1", "MSK", 8, 1, False), ("GMSK 8/1", "GMSK", 8, 1, False), ("4FSK 8/3", "4FSK", 8, 3, False),
         ("GMSK 8/1 one row", "GMSK", 8, 1, True)]
SIGMA, CFO = 0.3, 0.01


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 14)
    ap.add_argument("--row-samples", type=int, default=1 << 12)
    ap.add_argument("--long-row", type=int, default=1 << 22)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _lib, waveform as wf

    rows = []

    def timed(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    for name, mod, U, V, long_row in CELLS:
        R, S = (1, a.long_row) if long_row else (a.rows, a.row_samples)
        out = torch.empty((R, S), dtype=torch.complex64, device="cuda")
        ramp = torch.arange(S, device="cuda", dtype=torch.float32)[None, :]
        pulse = wf.cpm_pulse(mod, U)
        order, T = wf.cpm_order(mod), int(pulse.phase_taps.shape[0])
        P = -(-T // U)
        pulse_dev = wf.CpmPulse(torch.from_numpy(pulse.phase_taps.view(np.int32)).cuda(), pulse.phase_full)
        sigma_dev = torch.full((1,), SIGMA, dtype=torch.float32, device="cuda")
        rect = torch.from_numpy(wf.design_rect(8)).cuda()
        table = torch.from_numpy(wf.constellation_table("16QAM")).cuda()
        # the window of every sample at timing 0, as index tensors: made once, outside the timing
        n = np.arange(S, dtype=np.int64)
        p, top = (n * V) % U, (P - 1) + (n * V) // U
        cnt = P - (p >= T - (P - 1) * U)
        n_sym = int(top.max()) + 2
        lo = torch.from_numpy(top - cnt + 1).cuda()
        turns = pulse.phase_taps.astype(np.float64) / 2.0 ** 32
        window = [(torch.from_numpy(np.where(q < cnt, top - q, 0)).cuda(),
                   torch.from_numpy(np.where(q < cnt, turns[np.where(q < cnt, p + q * U, 0)], 0.0).astype(np.float32)).cuda()[None, :])
                  for q in range(P)]
        full = pulse.phase_full / 2.0 ** 32

        def ours():
            return wf.generate(mod, R, S, sps=(U, V), taps=pulse_dev, sigma=sigma_dev, cfo=CFO, seed=1, out=out)

        def linear():
            return wf.generate(table, R, S, sps=(8, 1), taps=rect, sigma=sigma_dev, cfo=CFO, seed=1, out=out)

        def stock():
            alpha = (2 * torch.randint(order, (R, n_sym), device="cuda") - (order - 1)).to(torch.float32)
            prefix = torch.cumsum(alpha, dim=1) - alpha                               # A(K) at K: the sum below K
            phase = full * prefix[:, lo]
            for at, tap in window:
                phase = phase + alpha[:, at] * tap
            phase0 = torch.rand((R, 1), device="cuda")
            step = (torch.rand((R, 1), device="cuda") * 2.0 - 1.0) * CFO
            angle = (phase + phase0 + step * ramp) * (2.0 * math.pi)
            v = torch.polar(torch.ones_like(angle), angle)
            noise = torch.view_as_complex(torch.empty((R, S, 2), dtype=torch.float32, device="cuda").normal_())
            return v.add_(noise, alpha=SIGMA * math.sqrt(0.5))

        def floor():
            return torch.view_as_real(out).normal_()

        ours()
        torch.cuda.synchronize()
        power = float((out.abs() ** 2).mean())
        stock_power = float((stock().abs() ** 2).mean())
        order_of_runs = ["cpm", "linear", "torch", "floor", "cpm_again"]
        funcs = {"cpm": (ours, a.launches), "cpm_again": (ours, a.launches), "linear": (linear, a.launches),
                 "torch": (stock, a.torch_launches), "floor": (floor, a.launches)}
        t = {k: [] for k in order_of_runs}
        for _ in range(a.rounds):
            for key in order_of_runs:
                t[key].append(timed(*funcs[key]))
        sec = {k: np.array(v) for k, v in t.items()}
        med = float(np.median(sec["cpm"]))
        tile, lds, segments = _lib.synth_cpm_plan(T, U, V, R, S)
        rate = lambda k: R * S / float(np.median(sec[k])) / 1e9                   # noqa: E731
        row = {"cell": name, "mod": mod, "order": order, "U": U, "V": V, "T": T, "P": P, "rows": R, "row_samples": S,
               "kernel": _lib.kernel_name_synth_cpm(), "tile_outputs": tile, "lds_bytes": lds, "segments": segments, "mean_power": power,
               "torch_mean_power": stock_power, "cpm_G_samples_per_s": R * S / med / 1e9,
               "cpm_fraction_of_8TBps": R * S * 8 / med / HBM_BYTES_PER_S,
               "cpm_vs_itself_spread": float(np.abs(sec["cpm"] / sec["cpm_again"] - 1.0).max()),
               "linear_rect_8_1_G_samples_per_s": rate("linear"), "torch_G_samples_per_s": rate("torch"), "floor_G_samples_per_s": rate("floor"),
               "ratio_cpm_over_linear_median": float(np.median(sec["linear"] / sec["cpm"])),
               "ratio_cpm_over_torch_median": float(np.median(sec["torch"] / sec["cpm"])),
               "ratio_cpm_over_floor_median": float(np.median(sec["floor"] / sec["cpm"])),
               **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in order_of_runs}}
        rows.append(row)
        print(f"{name:17s} cpm {row['cpm_G_samples_per_s']:7.2f} G samples/s ({100 * row['cpm_fraction_of_8TBps']:5.1f} % of 8 TB/s)  "
              f"linear {row['linear_rect_8_1_G_samples_per_s']:7.2f} x{row['ratio_cpm_over_linear_median']:.2f}  "
              f"torch {row['torch_G_samples_per_s']:7.2f} x{row['ratio_cpm_over_torch_median']:.2f}  floor {row['floor_G_samples_per_s']:7.2f} "
              f"x{row['ratio_cpm_over_floor_median']:.2f}  spread {row['cpm_vs_itself_spread']:.4f}  segments {segments}  "
              f"power {power:.3f} / {stock_power:.3f}", flush=True)
        if a.out:                                          # after every cell: a cut-off run keeps what it measured
            doc = {"what": "tools/cpm_bench.py", "rounds": a.rounds, "launches_per_round": a.launches,
                   "torch_launches_per_round": a.torch_launches, "sigma": SIGMA, "cfo": CFO, "device": torch.cuda.get_device_name(0), "rows": rows}
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
        del out, ramp, lo, window
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
