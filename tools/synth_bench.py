#!/usr/bin/env python3
"""The waveform generator (amcx_synth_c64) against two yardsticks, same box, alternating runs timed with HIP events.

    python tools/synth_bench.py [--rows 16384] [--row-samples 4096] [--rounds 5] [--launches 20] [--torch-launches 2] [--out profiles/NAME.json]

64 Mi output samples by default.  Cells: (rect, 8 / 1), (rrc over 16 symbols, 2 / 1), (rrc over 16 symbols, 8 / 3), all 16QAM at
sigma = 0.3 with a drawn phase, timing and carrier offset, and the noise class alone.  A round is `launches` calls of the
generator between two events, the yardsticks, and the generator ONCE MORE: the kernel against itself, whose ratio is the spread a
ratio of this job can be told from.

  (a) the complete stock-PyTorch formulation: amcpy_amd.synth.device_frames' operations -- torch.randint symbols, the table,
      a row's phase, normal_ noise -- with the pulse as one conv1d per polyphase class (the outputs fall into U / gcd(U, V)
      classes of one branch each) and the carrier as torch.polar of a per-row phase ramp.  The noise cell: normal_ and a scale.
  (b) the floor: torch.empty(...).normal_() over the same bytes, torch's own Philox Gaussian and nothing else.

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
CELLS = [("rect 8/1", "16QAM", 8, 1, "rect"), ("rrc16 2/1", "16QAM", 2, 1, "rrc"), ("rrc16 8/3", "16QAM", 8, 3, "rrc"),
         ("noise only", "WGN", 8, 1, "rect")]
SIGMA, CFO = 0.3, 0.01


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 14)
    ap.add_argument("--row-samples", type=int, default=1 << 12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _lib, waveform as wf

    R, S = a.rows, a.row_samples
    conv1d = torch.nn.functional.conv1d
    out = torch.empty((R, S), dtype=torch.complex64, device="cuda")
    ramp = torch.arange(S, device="cuda", dtype=torch.float32)[None, :]
    rows = []

    def timed(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    def floor():
        return torch.view_as_real(out).normal_()

    for name, mod, U, V, pulse in CELLS:
        h = wf.design_rrc(U, 16) if pulse == "rrc" else wf.design_rect(U)
        taps = torch.from_numpy(h).cuda()
        table = wf.constellation_table(mod)
        T, order = int(h.shape[0]), int(table.shape[0])
        P = -(-T // U)
        gcd = math.gcd(U, V)
        classes, stride = U // gcd, V // gcd
        hp = np.zeros((U, P), np.float32)
        for k in range(T):
            hp[k % U, k // U] = h[k]
        w_class = [torch.from_numpy(hp[(c * V) % U, ::-1].copy()).cuda().reshape(1, 1, P).repeat(2, 1, 1).contiguous()
                   for c in range(classes)]
        n_sym = P + ((S - 1) * V + U - 1) // U + 1
        table_c64 = torch.from_numpy(table).cuda()
        table_dev = torch.view_as_real(table_c64) if order else None
        sigma_dev = torch.full((1,), SIGMA, dtype=torch.float32, device="cuda")

        def ours():
            return wf.generate(table_c64, R, S, sps=(U, V), taps=taps, sigma=sigma_dev, cfo=CFO, seed=1, out=out)

        def stock():
            if order == 0:
                return torch.view_as_real(out).normal_().mul_(SIGMA * math.sqrt(0.5))
            idx = torch.randint(order, (R, n_sym), device="cuda")
            planes = table_dev[idx].permute(0, 2, 1).contiguous()                     # (R, 2, n_sym)
            y = torch.empty((R, 2, S), dtype=torch.float32, device="cuda")
            for c in range(classes):
                n_c = (S - c + classes - 1) // classes
                yc = conv1d(planes[:, :, (c * V) // U:], w_class[c], stride=stride, groups=2)
                y[:, :, c::classes] = yc[:, :, :n_c]
            phase = torch.rand((R, 1), device="cuda") * (2.0 * math.pi)
            step = (torch.rand((R, 1), device="cuda") * 2.0 - 1.0) * (2.0 * math.pi * CFO)
            angle = phase + step * ramp
            v = torch.view_as_complex(y.permute(0, 2, 1).contiguous()) * torch.polar(torch.ones_like(angle), angle)
            noise = torch.view_as_complex(torch.empty((R, S, 2), dtype=torch.float32, device="cuda").normal_())
            return v.add_(noise, alpha=SIGMA * math.sqrt(0.5))

        ours()
        torch.cuda.synchronize()
        power = float((out.abs() ** 2).mean())
        stock_power = float((stock().abs() ** 2).mean()) if order else float(torch.view_as_complex(stock()).abs().pow(2).mean())
        order_of_runs = ["synth", "torch", "floor", "synth_again"]
        funcs = {"synth": (ours, a.launches), "synth_again": (ours, a.launches), "torch": (stock, a.torch_launches), "floor": (floor, a.launches)}
        t = {k: [] for k in order_of_runs}
        for _ in range(a.rounds):
            for key in order_of_runs:
                t[key].append(timed(*funcs[key]))
        sec = {k: np.array(v) for k, v in t.items()}
        med = float(np.median(sec["synth"]))
        tile, lds, grid = _lib.synth_plan(order, T, U, V)
        row = {"cell": name, "mod": mod, "order": order, "U": U, "V": V, "T": T, "P": P, "rows": R, "row_samples": S, "kernel": _lib.kernel_name_synth(),
               "tile_outputs": tile, "lds_bytes": lds, "max_workgroups": grid, "mean_power": power, "torch_mean_power": stock_power,
               "synth_G_samples_per_s": R * S / med / 1e9, "synth_fraction_of_8TBps": R * S * 8 / med / HBM_BYTES_PER_S,
               "synth_vs_itself_spread": float(np.abs(sec["synth"] / sec["synth_again"] - 1.0).max()),
               "torch_G_samples_per_s": R * S / float(np.median(sec["torch"])) / 1e9,
               "floor_G_samples_per_s": R * S / float(np.median(sec["floor"])) / 1e9,
               "ratio_synth_over_torch_median": float(np.median(sec["torch"] / sec["synth"])),
               "ratio_synth_over_floor_median": float(np.median(sec["floor"] / sec["synth"])),
               **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in order_of_runs}}
        rows.append(row)
        print(f"{name:11s} synth {row['synth_G_samples_per_s']:7.2f} G samples/s ({100 * row['synth_fraction_of_8TBps']:5.1f} % of 8 TB/s)  "
              f"torch {row['torch_G_samples_per_s']:7.2f} x{row['ratio_synth_over_torch_median']:.2f}  floor {row['floor_G_samples_per_s']:7.2f} "
              f"x{row['ratio_synth_over_floor_median']:.2f}  spread {row['synth_vs_itself_spread']:.4f}  power {power:.3f} / {stock_power:.3f}", flush=True)
        if a.out:                                          # after every cell: a cut-off run keeps what it measured
            doc = {"what": "tools/synth_bench.py", "rounds": a.rounds, "launches_per_round": a.launches,
                   "torch_launches_per_round": a.torch_launches, "sigma": SIGMA, "cfo": CFO, "device": torch.cuda.get_device_name(0), "rows": rows}
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
