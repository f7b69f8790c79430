#!/usr/bin/env python3
"""The Welch spectrogram (amcx_spectrogram) on resident data against the read-bandwidth probe and the stock PyTorch
formulation, same box, alternating runs timed with HIP events.

    python tools/psd_bench.py [--samples 67108864] [--rounds 5] [--launches 20] [--torch-launches 2]
                              [--formats cf32,sc16,ci8,cu8] [--cells 256:128:16,...] [--out profiles/NAME.json]

Per format one resident stream of `samples` inputs; per (nfft, hop, A) in (256, 128, 16), (1024, 512, 16), (4096, 2048, 8),
(1024, 1024, 1), (64, 32, 32) a round is `launches` calls of psd.spectrogram between two events, `launches` of
amcx_probe_read_bw over the same input bytes, `torch-launches` of the PyTorch formulation (widen, torch.stft(..., window,
hop_length, center=False, return_complex=True), abs() ** 2, reshape, sum over A), and the spectrogram ONCE MORE: the kernel
against itself, whose ratio is the spread a ratio of this job can be told from.  Reported per cell: G input samples/s, the
fraction of 8 TB/s that bytes in once + bytes out over the time is, the ratios to the probe and to PyTorch, the spread, and the
largest |difference| to PyTorch relative to the largest output.  bench.py is not involved."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

CELLS = [(256, 128, 16), (1024, 512, 16), (4096, 2048, 8), (1024, 1024, 1), (64, 32, 32)]
BYTES = {"cf32": 8, "sc16": 4, "ci8": 2, "cu8": 2}
HBM_BYTES_PER_S = 8.0e12


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--formats", default="cf32,sc16,ci8,cu8")
    ap.add_argument("--cells", default=None, help="nfft:hop:A,... instead of the five cells")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from amcpy_amd import _formats, _lib, psd

    cells = CELLS if a.cells is None else [tuple(int(v) for v in s.split(":")) for s in a.cells.split(",")]
    S = a.samples
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(2026)
    partial = torch.empty((4096,), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for fmt in a.formats.split(","):
        scale = _formats.get(fmt).scale
        if fmt == "cf32":
            x = torch.view_as_complex(torch.randn((S, 2), device="cuda", generator=g))
        else:
            q = (torch.randn((S, 2), device="cuda", generator=g) * 30.0).round_().clamp_(-128, 127)
            x = {"sc16": lambda: (q * 200.0).to(torch.int16), "ci8": lambda: q.to(torch.int8),
                 "cu8": lambda: (q + 128.0).to(torch.uint8)}[fmt]()
            del q
        n_bytes = S * BYTES[fmt] // 16 * 16
        for nfft, hop, A in cells:
            w = torch.from_numpy(psd.window(nfft, "hann")).cuda()
            R = psd.out_rows(S, nfft, hop, A)
            out = torch.empty((R, nfft), dtype=torch.float32, device="cuda")

            def ours():
                return psd.spectrogram(x, nfft, hop=hop, averages=A, window=w, out=out)

            def probe():
                _lib.check(lib.amcx_probe_read_bw(x.data_ptr(), n_bytes, partial.data_ptr(), stream))

            def stock():
                c = x if fmt == "cf32" else torch.view_as_complex((x.to(torch.float32) - (128.0 if fmt == "cu8" else 0.0)) * scale)
                X = torch.stft(c, nfft, hop_length=hop, window=w, center=False, return_complex=True)      # (nfft, nseg)
                p = X.abs() ** 2
                return p[:, :R * A].reshape(nfft, R, A).sum(-1).t()

            ours()
            torch.cuda.synchronize()
            try:
                ref = stock()
                torch.cuda.synchronize()
                assert ref.shape == out.shape, (ref.shape, out.shape)
                agree = float((out - ref).abs().max() / ref.abs().max())
                del ref
                have_stock = True
            except Exception as exc:                                                   # the yardstick, not the product
                agree, have_stock = f"unavailable: {exc}", False
            torch.cuda.empty_cache()
            order = ("psd", "probe", "torch", "psd_again") if have_stock else ("psd", "probe", "psd_again")
            per = {"psd": a.launches, "psd_again": a.launches, "probe": a.launches, "torch": a.torch_launches}
            fn = {"psd": ours, "psd_again": ours, "probe": probe, "torch": stock}
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
            med = float(np.median(sec["psd"]))
            traffic = S * BYTES[fmt] + R * nfft * 4
            segs, lds, grid = _lib.spectrogram_plan(nfft, hop, A)
            row = {"format": fmt, "nfft": nfft, "hop": hop, "averages": A, "samples": S, "rows": R,
                   "kernel": _lib.kernel_name_psd(_formats.get(fmt).kind), "segments_per_pass": segs, "workgroups": grid,
                   "lds_bytes": lds, "psd_G_samples_per_s": S / med / 1e9, "psd_fraction_of_8TBps": traffic / med / HBM_BYTES_PER_S,
                   "psd_vs_itself_spread": float(np.abs(sec["psd"] / sec["psd_again"] - 1.0).max()),
                   "probe_G_bytes_per_s": n_bytes / float(np.median(sec["probe"])) / 1e9,
                   "ratio_probe_time_over_psd_time_median": float(np.median(sec["probe"] / sec["psd"])),
                   "difference_torch_over_largest_output": agree,
                   **{f"seconds_{k}": [round(float(v), 7) for v in sec[k]] for k in order}}
            if have_stock:
                row["torch_G_samples_per_s"] = S / float(np.median(sec["torch"])) / 1e9
                row["ratio_psd_over_torch_median"] = float(np.median(sec["torch"] / sec["psd"]))
            rows.append(row)
            print(f"{fmt:4s} nfft={nfft:4d} hop={hop:4d} A={A:2d}  psd {row['psd_G_samples_per_s']:7.2f} G samples/s "
                  f"({100 * row['psd_fraction_of_8TBps']:5.1f} % of 8 TB/s)  {row['ratio_probe_time_over_psd_time_median']:.3f} of the "
                  f"probe's rate  x{row.get('ratio_psd_over_torch_median', float('nan')):.2f} torch  spread "
                  f"{row['psd_vs_itself_spread']:.4f}  diff {agree if isinstance(agree, str) else format(agree, '.2e')}", flush=True)
            if a.out:                                      # after every cell: a cut-off run keeps what it measured
                doc = {"what": "tools/psd_bench.py", "rounds": a.rounds, "launches_per_round": a.launches,
                       "torch_launches_per_round": a.torch_launches, "device": torch.cuda.get_device_name(0), "rows": rows}
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
            del out, w
        del x
    return 0


if __name__ == "__main__":
    sys.exit(main())
