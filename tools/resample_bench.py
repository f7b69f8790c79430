#!/usr/bin/env python3
"""The rational resampler (amcx_resample) on resident data against two yardsticks, same box, alternating runs timed with HIP
events.

    python tools/resample_bench.py [--samples 67108864] [--rounds 5] [--launches 20] [--torch-launches 2] [--out profiles/NAME.json]

Per format (cf32, sc16, ci8, cu8) one resident stream of `samples` inputs; per (T, L, D) in (129, 1, 8), (161, 10, 7),
(257, 3, 16), (2561, 160, 147), (4096, 256, 255) a round is `launches` calls of resample between two events, the yardsticks,
and resample ONCE MORE: the kernel against itself, whose ratio is the spread a ratio of this job can be told from.

  (a) L = 1 only: tune_decimate on the same data and taps -- the same arithmetic, the same bits: what the generalisation costs.
  (b) every cell: stock PyTorch.  Widen, torch.polar of the float64 phase ramp rounded to float32 (the ramp itself is made
      once, outside the clock), complex product, and then the FASTER of two formulations, chosen by one timed trial each:
      "phases" -- the outputs fall into L' = L / gcd(L, D) classes of one polyphase branch each; per class one conv1d with that
      branch's P taps and stride D / gcd(L, D) over the two planes, written into its place of the result -- and "stuffed" --
      the mixed stream zero-stuffed by L and one conv1d with all T taps and stride D (skipped where the stuffed stream alone
      would take more than --stuff-bytes).

Reported per cell: G input samples/s, the fraction of 8 TB/s that bytes in + bytes out over the time is, each yardstick's rate
and ratio, the spread, and the largest |difference| between resample and (b) relative to the criterion's bound
(tests/resample_ref.py).  bench.py is not involved."""
import argparse
import json
import math
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

SHAPES = [(129, 1, 8), (161, 10, 7), (257, 3, 16), (2561, 160, 147), (4096, 256, 255)]
BYTES = {"cf32": 8, "sc16": 4, "ci8": 2, "cu8": 2}
HBM_BYTES_PER_S = 8.0e12
SHIFT = -0.1234567


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--formats", default="cf32,sc16,ci8,cu8")
    ap.add_argument("--stuff-bytes", type=int, default=16 << 30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _lib, ddc, resample as rs

    S = a.samples
    g = torch.Generator(device="cuda").manual_seed(2026)
    step = ddc.phase_step_of(SHIFT)
    turns = (torch.arange(S, device="cuda", dtype=torch.float64) * (step / 2.0 ** 64)).frac_()
    angle = (turns * (2.0 * np.pi)).to(torch.float32)
    del turns
    conv1d = torch.nn.functional.conv1d
    rows = []

    def timed(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    for fmt in a.formats.split(","):
        scale = ddc._DEFAULT_SCALE[fmt]
        if fmt == "cf32":
            x = torch.view_as_complex(torch.randn((S, 2), device="cuda", generator=g))
        else:
            q = (torch.randn((S, 2), device="cuda", generator=g) * 30.0).round_().clamp_(-128, 127)
            x = {"sc16": lambda: (q * 200.0).to(torch.int16), "ci8": lambda: q.to(torch.int8),
                 "cu8": lambda: (q + 128.0).to(torch.uint8)}[fmt]()
            del q
        for T, L, D in SHAPES:
            h = rs.design_resample_lowpass(L, D, T)
            taps = torch.from_numpy(h).cuda()
            P = -(-T // L)
            M = rs.out_samples(S, T, L, D)
            out = torch.empty(M, dtype=torch.complex64, device="cuda")
            gcd = math.gcd(L, D)
            classes, stride = L // gcd, D // gcd
            # class c: outputs c, c + L', ...: branch (c D) mod L, window from sample (c D) // L on, `stride` apart
            hp = np.zeros((L, P), np.float32)
            for k in range(T):
                hp[k % L, k // L] = h[k]
            w_class = [torch.from_numpy(np.ascontiguousarray(hp[(c * D) % L, ::-1])).cuda().reshape(1, 1, P).repeat(2, 1, 1).contiguous()
                       for c in range(classes)]
            w_full = taps.flip(0).reshape(1, 1, T).repeat(2, 1, 1).contiguous()

            def ours():
                return rs.resample(x, taps, L, D, shift=SHIFT, out=out)

            def mixed_planes():
                c = x if fmt == "cf32" else torch.view_as_complex((x.to(torch.float32) - (128.0 if fmt == "cu8" else 0.0)) * scale)
                v = c * torch.polar(torch.ones_like(angle), angle)
                return torch.view_as_real(v).t().unsqueeze(0)                          # (1, 2, S)

            def stock_phases():
                planes = mixed_planes()
                y = torch.empty((M, 2), dtype=torch.float32, device="cuda")
                for c in range(classes):
                    n_c = (M - c + classes - 1) // classes
                    if n_c <= 0:
                        continue
                    yc = conv1d(planes[:, :, (c * D) // L:], w_class[c], stride=stride, groups=2)      # (1, 2, >= n_c)
                    y[c::classes] = yc[0, :, :n_c].t()
                return torch.view_as_complex(y)

            def stock_stuffed():
                planes = mixed_planes()
                up = torch.zeros((1, 2, S * L), dtype=torch.float32, device="cuda")
                up[:, :, ::L] = planes
                # output m reads the stuffed samples (P - 1) L + m D - (T - 1) ... (P - 1) L + m D: pad in front where that is < 0
                front = (P - 1) * L - (T - 1)
                y = conv1d(up[:, :, front:] if front >= 0 else torch.nn.functional.pad(up, (-front, 0)), w_full, stride=D, groups=2)
                return torch.view_as_complex(y[0, :, :M].t().contiguous())

            ours()
            torch.cuda.synchronize()
            stock, chosen, trial, agree = None, None, {}, None
            for name, f in (("phases", stock_phases), ("stuffed", stock_stuffed)):
                if name == "stuffed" and S * L * 8 > a.stuff_bytes:
                    trial[name] = f"not run: the stuffed stream alone is {S * L * 8 / 2 ** 30:.0f} GiB"
                    continue
                try:
                    ref = f()
                    torch.cuda.synchronize()
                    n_pick = min(M, 4096)
                    pick = torch.arange(n_pick, device="cuda", dtype=torch.int64) * (M - 1) // max(n_pick - 1, 1)
                    t = pick * D
                    qs = torch.arange(P, device="cuda", dtype=torch.int64)[None, :]
                    tap_i = (t % L)[:, None] + qs * L
                    live = tap_i < T
                    samp = ((P - 1) + t // L)[:, None] - qs
                    xs = x[samp.reshape(-1)]
                    mag = (xs if fmt == "cf32" else torch.view_as_complex(xs.to(torch.float32) * scale
                                                                           - (128.0 * scale if fmt == "cu8" else 0.0))).abs()
                    hw = torch.where(live, taps[torch.where(live, tap_i, 0)].abs().double(), 0.0)
                    bound = (P + 8) * 2.0 ** -24 * (mag.reshape(-1, P).double() * hw).sum(dim=1)
                    diff = (out[pick] - ref[pick]).abs().double()
                    this = float(torch.where(bound > 0, diff / bound, torch.where(diff > 0, float("inf"), 0.0).double()).max())
                    del ref, xs, mag, hw, bound, diff
                    trial[name] = timed(f, 1)
                    if chosen is None or trial[name] < trial[chosen]:
                        stock, chosen, agree = f, name, this
                except (torch.cuda.OutOfMemoryError, RuntimeError) as exc:            # the yardstick, not the product ...
                    text = str(exc)
                    if not isinstance(exc, torch.cuda.OutOfMemoryError) and not any(
                            w in text for w in ("out of memory", "miopen", "MIOpen", "shape", "size")):
                        raise                                                          # ... but a device error ends the job
                    trial[name] = f"unavailable: {type(exc).__name__}: {text}"[:200]
                torch.cuda.empty_cache()
            taps_ddc = taps if L == 1 and T <= ddc.MAX_TAPS else None

            def ddc_same():
                return ddc.tune_decimate(x, taps_ddc, D, shift=SHIFT, out=out)

            order = ["resample"] + (["ddc"] if taps_ddc is not None else []) + (["torch"] if stock is not None else []) + ["resample_again"]
            funcs = {"resample": (ours, a.launches), "resample_again": (ours, a.launches), "ddc": (ddc_same, a.launches),
                     "torch": (stock, a.torch_launches)}
            t = {k: [] for k in order}
            for _ in range(a.rounds):
                for key in order:
                    t[key].append(timed(*funcs[key]))
            sec = {k: np.array(v) for k, v in t.items()}
            med = float(np.median(sec["resample"]))
            traffic = S * BYTES[fmt] + M * 8
            tile, span, grid, lds = _lib.resample_plan(T, L, D)
            row = {"format": fmt, "T": T, "L": L, "D": D, "P": P, "samples": S, "outputs": M,
                   "kernel": _lib.kernel_name_resample(ddc._KINDS[fmt]), "tile_outputs": tile, "max_span": span, "lds_bytes": lds,
                   "resample_G_samples_per_s": S / med / 1e9, "resample_G_outputs_per_s": M / med / 1e9,
                   "resample_fraction_of_8TBps": traffic / med / HBM_BYTES_PER_S,
                   "resample_vs_itself_spread": float(np.abs(sec["resample"] / sec["resample_again"] - 1.0).max()),
                   "torch_formulation": chosen, "torch_trials_seconds": trial, "difference_over_bound_max": agree,
                   **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in order}}
            if "ddc" in sec:
                row["ddc_G_samples_per_s"] = S / float(np.median(sec["ddc"])) / 1e9
                row["ratio_resample_over_ddc_median"] = float(np.median(sec["ddc"] / sec["resample"]))
            if "torch" in sec:
                row["torch_G_samples_per_s"] = S / float(np.median(sec["torch"])) / 1e9
                row["ratio_resample_over_torch_median"] = float(np.median(sec["torch"] / sec["resample"]))
            rows.append(row)
            print(f"{fmt:4s} T={T:4d} L={L:3d} D={D:3d}  resample {row['resample_G_samples_per_s']:7.2f} G samples/s "
                  f"({100 * row['resample_fraction_of_8TBps']:5.1f} % of 8 TB/s)  ddc x{row.get('ratio_resample_over_ddc_median', float('nan')):.3f}"
                  f"  torch[{chosen}] {row.get('torch_G_samples_per_s', float('nan')):7.2f} x{row.get('ratio_resample_over_torch_median', float('nan')):.2f}"
                  f"  spread {row['resample_vs_itself_spread']:.4f}  diff/bound {agree if agree is None else round(agree, 4)}", flush=True)
            if a.out:                                      # after every cell: a cut-off run keeps what it measured
                doc = {"what": "tools/resample_bench.py", "rounds": a.rounds, "launches_per_round": a.launches,
                       "torch_launches_per_round": a.torch_launches, "shift": SHIFT, "device": torch.cuda.get_device_name(0),
                       "rows": rows}
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
            del out, taps, w_class, w_full
        del x
    return 0


if __name__ == "__main__":
    sys.exit(main())
