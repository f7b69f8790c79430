#!/usr/bin/env python3
"""Blind carrier recovery (amcx_carrier_c64) against three yardsticks, same box, alternating runs timed with HIP events.

    python tools/carrier_bench.py [--samples 33554432] [--rounds 5] [--launches 20] [--torch-launches 2] [--out profiles/NAME.json]

32 Mi samples of resident QPSK-like rows by default.  Cells: N = 128, 1024, 2048, 4096; M = 1 and 4; estimate only (the records
alone) and full (records and the recovered rows); the search covers N / 16 bins.  A round is `launches` calls of the kernel
between two events, the yardsticks, and the kernel ONCE MORE: the kernel against itself, whose ratio is the spread a ratio of
this job can be told from.

  (a) the stock-PyTorch formulation on the same data: the row power, x * rsqrt(power), the M-th power by squaring, torch.fft.fft,
      |.|^2, a masked argmax over the range, three gathers, the complex interpolation, torch.polar of the phase ramp and the
      product (the last two in the full cells only).
  (b) the floor: amcx_probe_read_bw over the bytes the kernel reads and writes (8 N per row in, 32 per record, 8 N out when full).
  (c) psd.spectrogram at (nfft, hop, averages) = (N, N, 1) with a rectangular window over the same samples: the same transform
      without the power tree, the M-th power, the search and the second pass -- the ratio says what the rest costs.

Reported per cell: G samples/s, the fraction of 8 TB/s its bytes are, each yardstick's rate and the ratio, and the spread.  No
ratio is promised: where the kernel loses, the row says so.  bench.py is not involved."""
import argparse
import json
import math
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

HBM_BYTES_PER_S = 8.0e12
SIZES = (128, 1024, 2048, 4096)
ORDERS = (1, 4)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _lib, carrier, psd

    lib = _lib.load()
    partial = torch.empty(1 << 16, dtype=torch.float32, device="cuda")
    rows = []

    def timed(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    for N in SIZES:
        R = a.samples // N
        sb = N // 16
        # QPSK at 4 samples per symbol, a drawn offset inside the range of x^4, a drawn phase, noise at 20 dB, an odd level
        sym = torch.randint(0, 4, (R, N // 4), device="cuda")
        ang = (sym.repeat_interleave(4, dim=1).float() * 0.25 + 0.125 + torch.rand((R, 1), device="cuda")
               + (torch.rand((R, 1), device="cuda") - 0.5) * (0.8 * sb / (4 * N)) * torch.arange(N, device="cuda")[None, :]) * (2.0 * math.pi)
        x = torch.polar(torch.full_like(ang, 0.37), ang)
        x = (x + 0.037 * math.sqrt(0.5) * torch.view_as_complex(torch.randn((R, N, 2), device="cuda"))).contiguous()
        del sym, ang
        out = torch.empty((R, N), dtype=torch.complex64, device="cuda")
        raw = torch.empty((R, 32), dtype=torch.uint8, device="cuda")
        P = torch.empty((R, N), dtype=torch.float32, device="cuda")
        rect = torch.ones(N, dtype=torch.float32, device="cuda")
        flat = x.view(-1)
        k_signed = torch.arange(N, device="cuda")
        k_signed = torch.where(k_signed >= N // 2, k_signed - N, k_signed)
        in_range = (k_signed.abs() <= sb)[None, :]
        n_ramp = torch.arange(N, device="cuda", dtype=torch.float32)[None, :]
        stream = torch.cuda.current_stream().cuda_stream

        for M in ORDERS:
            for full in (False, True):
                flags = 7 if full else 0
                moved = (R * (8 * N + 32 + (8 * N if full else 0))) // 16 * 16
                both = torch.empty(moved // 8, dtype=torch.complex64, device="cuda")

                def ours():
                    _lib.check(lib.amcx_carrier_c64(x.data_ptr(), R, N, N, M, sb, flags, raw.data_ptr(), out.data_ptr() if full else None,
                                                    N, stream))

                def stock():
                    power = (x.real * x.real + x.imag * x.imag).mean(dim=1, keepdim=True)
                    u = x * torch.rsqrt(power)
                    z = u
                    for _ in range(int(math.log2(M))):
                        z = z * z
                    Z = torch.fft.fft(z, dim=1)
                    Pz = Z.real * Z.real + Z.imag * Z.imag
                    at = torch.where(in_range, Pz, -1.0).argmax(dim=1, keepdim=True)
                    b = torch.gather(Z, 1, at)
                    lo, hi = torch.gather(Z, 1, (at - 1) % N), torch.gather(Z, 1, (at + 1) % N)
                    frac = -((hi - lo) / ((b - lo) + (b - hi))).real
                    f = (torch.gather(k_signed[None, :].expand(R, N), 1, at) + frac) / (M * N)
                    ph = (torch.angle(b) / (2.0 * math.pi) - frac * ((N - 1) / N)) / M
                    if full:
                        rot = torch.polar(torch.ones((R, N), device="cuda"), (ph + f * n_ramp) * (-2.0 * math.pi))
                        torch.mul(u, rot, out=out)
                    return f

                def floor():
                    _lib.check(lib.amcx_probe_read_bw(both.data_ptr(), moved, partial.data_ptr(), stream))

                def spectrum():
                    psd.spectrogram(flat, N, hop=N, averages=1, window=rect, out=P)

                ours()
                torch.cuda.synchronize()
                est = carrier.Estimates(raw.clone(), N, M)
                ours_cycles = est.cycles
                agree = float((stock().reshape(-1).double() - ours_cycles).abs().median() * M * N)      # bins of x^M between the two
                order_of_runs = ["carrier", "torch", "floor", "spectrogram", "carrier_again"]
                funcs = {"carrier": (ours, a.launches), "carrier_again": (ours, a.launches), "torch": (stock, a.torch_launches),
                         "floor": (floor, a.launches), "spectrogram": (spectrum, a.launches)}
                t = {k: [] for k in order_of_runs}
                for _ in range(a.rounds):
                    for key in order_of_runs:
                        t[key].append(timed(*funcs[key]))
                sec = {k: np.array(v) for k, v in t.items()}
                med = float(np.median(sec["carrier"]))
                per_wg, lds = _lib.carrier_plan(N)
                row = {"cell": f"N={N} M={M} {'full' if full else 'estimate'}", "n": N, "order": M, "full": full, "rows": R,
                       "search_bins": sb, "kernel": _lib.kernel_name_carrier(), "rows_per_workgroup": per_wg, "lds_bytes": lds,
                       "median_bins_between_kernel_and_torch": agree,
                       "carrier_G_samples_per_s": R * N / med / 1e9, "carrier_fraction_of_8TBps": moved / med / HBM_BYTES_PER_S,
                       "carrier_vs_itself_spread": float(np.abs(sec["carrier"] / sec["carrier_again"] - 1.0).max()),
                       "torch_G_samples_per_s": R * N / float(np.median(sec["torch"])) / 1e9,
                       "read_bw_G_samples_per_s": R * N / float(np.median(sec["floor"])) / 1e9,
                       "read_bw_TB_per_s": moved / float(np.median(sec["floor"])) / 1e12,
                       "spectrogram_G_samples_per_s": R * N / float(np.median(sec["spectrogram"])) / 1e9,
                       "ratio_carrier_over_torch_median": float(np.median(sec["torch"] / sec["carrier"])),
                       "ratio_carrier_over_read_bw_median": float(np.median(sec["floor"] / sec["carrier"])),
                       "ratio_carrier_over_spectrogram_median": float(np.median(sec["spectrogram"] / sec["carrier"])),
                       **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in order_of_runs}}
                rows.append(row)
                print(f"{row['cell']:24s} carrier {row['carrier_G_samples_per_s']:7.2f} G samples/s ({100 * row['carrier_fraction_of_8TBps']:5.1f} % of 8 TB/s)  "
                      f"torch {row['torch_G_samples_per_s']:6.2f} x{row['ratio_carrier_over_torch_median']:.2f}  read {row['read_bw_G_samples_per_s']:7.2f} "
                      f"x{row['ratio_carrier_over_read_bw_median']:.2f}  spectrogram {row['spectrogram_G_samples_per_s']:7.2f} "
                      f"x{row['ratio_carrier_over_spectrogram_median']:.2f}  spread {row['carrier_vs_itself_spread']:.4f}  bins apart {agree:.3f}", flush=True)
                if a.out:                                          # after every cell: a cut-off run keeps what it measured
                    doc = {"what": "tools/carrier_bench.py", "rounds": a.rounds, "launches_per_round": a.launches,
                           "torch_launches_per_round": a.torch_launches, "samples": a.samples, "library": str(_lib.LIB_PATH.name),
                           "device": torch.cuda.get_device_name(0), "rows": rows}
                    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
                del both
        del x, out, raw, P, flat
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
