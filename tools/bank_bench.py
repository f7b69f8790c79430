#!/usr/bin/env python3
"""The polyphase filter bank (amcx_filter_bank) on resident data against today's route -- C calls of amcx_tune_decimate -- and
against the stock PyTorch formulation, same box, alternating runs timed with HIP events.

    python tools/bank_bench.py [--samples 67108864] [--rounds 5] [--launches 20] [--route-launches 1] [--torch-launches 2]
                               [--formats cf32,sc16,ci8,cu8] [--out profiles/NAME.json]

Per format one resident stream of `samples` inputs; per (C, T, D) in (8, 128, 8), (8, 128, 4), (64, 1024, 64), (64, 1024, 32),
(256, 2048, 256), (256, 2048, 128) -- critically sampled and 2x oversampled, T <= 2048 because the route's kernel takes no more
-- a round is `launches` calls of filter_bank between two events, `route-launches` times the C calls of tune_decimate on the
same data and taps (shift - c / C, into the same (C, M) buffer), `torch-launches` of the PyTorch formulation (widen, torch.polar
of the float64 phase ramp, the polyphase reshape, einsum over the taps of a branch, torch.fft.ifft; the ramp is made once,
outside the clock), and filter_bank ONCE MORE: the kernel against itself, whose ratio is the spread a ratio of this job can be
told from.  Reported per cell: G input samples/s, the fraction of 8 TB/s that bytes in + bytes out over the time is, the two
ratios, the spread, and the largest |difference| between the bank and either yardstick on a sample of the outputs, relative to
the largest output.  bench.py is not involved."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

SHAPES = [(8, 128, 8), (8, 128, 4), (64, 1024, 64), (64, 1024, 32), (256, 2048, 256), (256, 2048, 128)]
BYTES = {"cf32": 8, "sc16": 4, "ci8": 2, "cu8": 2}
HBM_BYTES_PER_S = 8.0e12
SHIFT = -0.1234567


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--route-launches", type=int, default=1)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--formats", default="cf32,sc16,ci8,cu8")
    ap.add_argument("--shapes", default=None, help="C:T:D,... instead of the six cells")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from fractions import Fraction
    from amcpy_amd import _lib, bank, ddc

    shapes = SHAPES if a.shapes is None else [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
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
        for Cn, T, D in shapes:
            P = T // Cn
            assert P * Cn == T and Cn % D == 0, "the PyTorch formulation here wants whole branches and D | C"
            taps_host = bank.design_bank_lowpass(Cn, P)
            taps = torch.from_numpy(taps_host).cuda()
            M = bank.out_samples(S, T, Cn, D)
            out = torch.empty((Cn, M), dtype=torch.complex64, device="cuda")
            route_out = torch.empty((Cn, M), dtype=torch.complex64, device="cuda")
            # H[p, i] = h[p + (P - 1 - i) C]: the taps of branch p in the order a window of the reshaped stream holds its samples
            hflip = torch.from_numpy(np.ascontiguousarray(taps_host.reshape(P, Cn)[::-1].T)).cuda()

            def ours():
                return bank.filter_bank(x, taps, Cn, D, shift=SHIFT, out=out)

            def route():
                for c in range(Cn):
                    ddc.tune_decimate(x, taps, D, shift=Fraction(SHIFT) - Fraction(c, Cn), out=route_out[c])
                return route_out

            def stock():
                c = x if fmt == "cf32" else torch.view_as_complex((x.to(torch.float32) - (128.0 if fmt == "cu8" else 0.0)) * scale)
                v = c * torch.polar(torch.ones_like(angle), angle)
                R = Cn // D
                y = torch.empty((M, Cn), dtype=torch.complex64, device="cuda")
                for s in range(R):                                          # the instants m = s mod (C / D): windows D samples on
                    vs = v[s * D:]
                    K = vs.shape[0] // Cn
                    vr = torch.view_as_real(vs[:K * Cn].view(K, Cn).flip(1))       # [j, p] = v[j C + C - 1 - p]
                    win = vr.unfold(0, P, 1)                                # (K - P + 1, C, 2, P): [m, p, :, i] = vr[m + i, p]
                    u = torch.view_as_complex(torch.einsum("mpci,pi->mpc", win, hflip).contiguous())
                    rot = (s * D + T - 1) % Cn                              # a(n_m): g[r] = u[(r + a) mod C]
                    y[s::R] = torch.fft.ifft(torch.roll(u, -rot, dims=1), dim=1, norm="forward")[:(M - s + R - 1) // R]
                return y.t().contiguous()

            ours()
            torch.cuda.synchronize()
            pick = torch.arange(min(M, 4096), device="cuda", dtype=torch.int64) * (M - 1) // max(min(M, 4096) - 1, 1)
            top = float(out[:, pick].abs().max())
            route()
            torch.cuda.synchronize()
            agree_route = float((out[:, pick] - route_out[:, pick]).abs().max()) / top
            try:
                ref = stock()
                torch.cuda.synchronize()
                assert ref.shape == out.shape, (ref.shape, out.shape)
                agree_stock = float((out[:, pick] - ref[:, pick]).abs().max()) / top
                del ref
                have_stock = True
            except Exception as exc:                                                   # the yardstick, not the product
                agree_stock, have_stock = f"unavailable: {exc}", False
            order = ("bank", "route", "torch", "bank_again") if have_stock else ("bank", "route", "bank_again")
            per = {"bank": a.launches, "bank_again": a.launches, "route": a.route_launches, "torch": a.torch_launches}
            fn = {"bank": ours, "bank_again": ours, "route": route, "torch": stock}
            t = {k: [] for k in order}
            for _ in range(a.rounds):
                for key in order:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(per[key]):
                        fn[key]()
                    e1.record()
                    torch.cuda.synchronize()
                    t[key].append(e0.elapsed_time(e1) * 1e-3 / per[key])
            sec = {k: np.array(v) for k, v in t.items()}
            med = float(np.median(sec["bank"]))
            traffic = S * BYTES[fmt] + Cn * M * 8
            tile, grid, lds = _lib.filter_bank_plan(T, Cn, D)
            row = {"format": fmt, "C": Cn, "T": T, "D": D, "samples": S, "outputs_per_channel": M,
                   "kernel": _lib.kernel_name_bank(ddc._KINDS[fmt]), "tile": tile, "workgroups": grid, "lds_bytes": lds,
                   "bank_G_samples_per_s": S / med / 1e9, "bank_fraction_of_8TBps": traffic / med / HBM_BYTES_PER_S,
                   "bank_vs_itself_spread": float(np.abs(sec["bank"] / sec["bank_again"] - 1.0).max()),
                   "route_G_samples_per_s": S / float(np.median(sec["route"])) / 1e9,
                   "ratio_bank_over_route_median": float(np.median(sec["route"] / sec["bank"])),
                   "difference_route_over_largest_output": agree_route, "difference_torch_over_largest_output": agree_stock,
                   **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in order}}
            if have_stock:
                row["torch_G_samples_per_s"] = S / float(np.median(sec["torch"])) / 1e9
                row["ratio_bank_over_torch_median"] = float(np.median(sec["torch"] / sec["bank"]))
            rows.append(row)
            print(f"{fmt:4s} C={Cn:3d} T={T:4d} D={D:3d}  bank {row['bank_G_samples_per_s']:7.2f} G samples/s "
                  f"({100 * row['bank_fraction_of_8TBps']:5.1f} % of 8 TB/s)  x{row['ratio_bank_over_route_median']:.1f} the {Cn} calls"
                  f"  x{row.get('ratio_bank_over_torch_median', float('nan')):.1f} torch  spread {row['bank_vs_itself_spread']:.4f}  "
                  f"diff {agree_route:.2e} / {agree_stock if isinstance(agree_stock, str) else format(agree_stock, '.2e')}", flush=True)
            if a.out:                                      # after every cell: a cut-off run keeps what it measured
                doc = {"what": "tools/bank_bench.py", "rounds": a.rounds, "launches_per_round": a.launches,
                       "route_launches_per_round": a.route_launches, "torch_launches_per_round": a.torch_launches, "shift": SHIFT,
                       "device": torch.cuda.get_device_name(0), "rows": rows}
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
            del out, route_out, taps, hflip
        del x
    return 0


if __name__ == "__main__":
    sys.exit(main())
