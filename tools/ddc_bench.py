#!/usr/bin/env python3
"""The down-converter (amcx_tune_decimate) on resident data against the stock PyTorch formulation, same box, alternating runs
timed with HIP events.

    python tools/ddc_bench.py [--samples 67108864] [--rounds 5] [--launches 20] [--torch-launches 3] [--out profiles/NAME.json]

Per format (cf32, sc16, ci8, cu8) one resident stream of `samples` inputs; per (T, D) in (1, 1), (33, 2), (65, 4), (129, 8),
(257, 16) -- T = 16 D + 1, design_lowpass's default, and the pure mixer -- a round is `launches` calls of tune_decimate between
two events, `torch-launches` of the PyTorch formulation (widen, torch.polar of the float64 phase ramp rounded to float32,
complex product, conv1d with stride D over the two planes; the ramp itself is made once, outside the clock), and tune_decimate
ONCE MORE: the kernel against itself, whose ratio is the spread a ratio of this job can be told from.  Reported per cell: G
input samples/s, the fraction of 8 TB/s that bytes in + bytes out over the time is, PyTorch's rate, the ratio, the spread, and
the largest |difference| between the two results relative to the criterion's bound (tests/ddc_ref.py).  bench.py is not involved."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

SHAPES = [(1, 1), (33, 2), (65, 4), (129, 8), (257, 16)]
BYTES = {"cf32": 8, "sc16": 4, "ci8": 2, "cu8": 2}
HBM_BYTES_PER_S = 8.0e12
SHIFT = -0.1234567


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--torch-launches", type=int, default=3)
    ap.add_argument("--formats", default="cf32,sc16,ci8,cu8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _lib, ddc

    S = a.samples
    g = torch.Generator(device="cuda").manual_seed(2026)
    step = ddc.phase_step_of(SHIFT)
    # the yardstick's phase ramp: exact turns in float64 (the step's top 53 bits), wrapped, as radians in float32
    turns = (torch.arange(S, device="cuda", dtype=torch.float64) * (step / 2.0 ** 64)).frac_()
    angle = (turns * (2.0 * np.pi)).to(torch.float32)
    del turns
    rows = []
    for fmt in a.formats.split(","):
        scale = ddc._DEFAULT_SCALE[fmt]
        if fmt == "cf32":
            x = torch.view_as_complex(torch.randn((S, 2), device="cuda", generator=g))
        else:
            q = (torch.randn((S, 2), device="cuda", generator=g) * 30.0).round_().clamp_(-128, 127)
            x = {"sc16": lambda: (q * 200.0).to(torch.int16), "ci8": lambda: q.to(torch.int8),
                 "cu8": lambda: (q + 128.0).to(torch.uint8)}[fmt]()
            del q
        for T, D in SHAPES:
            taps = torch.from_numpy(ddc.design_lowpass(D, T)).cuda()
            M = ddc.out_samples(S, T, D)
            out = torch.empty(M, dtype=torch.complex64, device="cuda")
            weight = taps.flip(0).reshape(1, 1, T).repeat(2, 1, 1).contiguous()       # conv1d correlates: the taps reversed

            def ours():
                return ddc.tune_decimate(x, taps, D, shift=SHIFT, out=out)

            def stock():
                c = x if fmt == "cf32" else torch.view_as_complex((x.to(torch.float32) - (128.0 if fmt == "cu8" else 0.0)) * scale)
                v = c * torch.polar(torch.ones_like(angle), angle)
                planes = torch.view_as_real(v).t().unsqueeze(0)                        # (1, 2, S)
                y = torch.nn.functional.conv1d(planes, weight, stride=D, groups=2)     # (1, 2, M)
                return torch.view_as_complex(y[0].t().contiguous())

            ours()
            torch.cuda.synchronize()
            try:
                ref = stock()
                torch.cuda.synchronize()
                # |difference| against the criterion's bound, on a sample of the outputs
                n_pick = min(M, 4096)                      # (integer arithmetic: a float32 linspace rounds M - 1 up to M at 2^26)
                pick = torch.arange(n_pick, device="cuda", dtype=torch.int64) * (M - 1) // max(n_pick - 1, 1)
                win = (pick[:, None] * D + torch.arange(T, device="cuda")[None, :]).reshape(-1)
                assert int(pick.max()) < M and int(win.min()) >= 0 and int(win.max()) < S
                mag = (x[win] if fmt == "cf32" else torch.view_as_complex(x[win].to(torch.float32) * scale
                                                                         - (128.0 * scale if fmt == "cu8" else 0.0))).abs()
                bound = (T + 8) * 2.0 ** -24 * (mag.reshape(-1, T).double() @ taps.flip(0).abs().double())
                diff = (out[pick] - ref[pick]).abs().double()
                # (an output over nothing but zero samples has bound 0: there any difference at all is infinitely many bounds)
                agree = float(torch.where(bound > 0, diff / bound, torch.where(diff > 0, float("inf"), 0.0).double()).max())
                del diff
                del ref, pick, win, mag, bound
                have_stock = True
            except Exception as exc:                                                   # the yardstick, not the product
                agree, have_stock = f"unavailable: {exc}", False
            order = ("ddc", "torch", "ddc_again") if have_stock else ("ddc", "ddc_again")
            t = {k: [] for k in order}
            for _ in range(a.rounds):
                for key in order:
                    n = a.torch_launches if key == "torch" else a.launches
                    f = stock if key == "torch" else ours
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    t[key].append(e0.elapsed_time(e1) * 1e-3 / n)
            sec = {k: np.array(v) for k, v in t.items()}
            med = float(np.median(sec["ddc"]))
            traffic = S * BYTES[fmt] + M * 8
            row = {"format": fmt, "T": T, "D": D, "samples": S, "outputs": M, "kernel": _lib.kernel_name_ddc(ddc._KINDS[fmt]),
                   "ddc_G_samples_per_s": S / med / 1e9, "ddc_fraction_of_8TBps": traffic / med / HBM_BYTES_PER_S,
                   "ddc_vs_itself_spread": float(np.abs(sec["ddc"] / sec["ddc_again"] - 1.0).max()),
                   "difference_over_bound_max": agree,
                   **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in order}}
            if have_stock:
                row["torch_G_samples_per_s"] = S / float(np.median(sec["torch"])) / 1e9
                row["ratio_ddc_over_torch_median"] = float(np.median(sec["torch"] / sec["ddc"]))
            rows.append(row)
            print(f"{fmt:4s} T={T:4d} D={D:3d}  ddc {row['ddc_G_samples_per_s']:7.2f} G samples/s "
                  f"({100 * row['ddc_fraction_of_8TBps']:5.1f} % of 8 TB/s)  torch {row.get('torch_G_samples_per_s', float('nan')):7.2f}"
                  f"  x{row.get('ratio_ddc_over_torch_median', float('nan')):.2f}  spread {row['ddc_vs_itself_spread']:.4f}  "
                  f"diff/bound {agree if isinstance(agree, str) else round(agree, 4)}", flush=True)
            if a.out:                                      # after every cell: a cut-off run keeps what it measured
                doc = {"what": "tools/ddc_bench.py", "rounds": a.rounds, "launches_per_round": a.launches,
                       "torch_launches_per_round": a.torch_launches, "shift": SHIFT, "device": torch.cuda.get_device_name(0),
                       "rows": rows}
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
            del out, taps, weight
        del x
    return 0


if __name__ == "__main__":
    sys.exit(main())
