#!/usr/bin/env python3
"""Timing of the fixed-point launches on 638 976 x 18 resident rows, default network (6 -> 26 -> 29 -> 30 -> 6, relu):

    python tools/quantize_bench.py [--rounds 5] [--launches 20] [--out profiles/NAME.json]

* `classify_q15` (labels + counts, one amcx_mlp_classify_q15 call) against `classify` (amcx_mlp_classify_f32, the same
  outputs) on the same rows, and against STOCK PYTORCH doing the integer arithmetic of include/amcx.h on the same device:
  the scaler, clamp and rint, per layer an exact matrix product (int64 where torch has one on the device, float64 otherwise:
  exact below 2^53, the sums stay below 2^37), the bias shift, the rounding shift, the clamps, argmax and a bincount per group.
* `calibrate` (one amcx_mlp_range_f32 call) against stock PyTorch's `aminmax` over the same float32 forward pass.

All are timed between device events, --launches per window, in one process, alternating round by round; the medians over
the rounds are reported with every round's figure, and the spread of each kernel against itself (max - min) / median.
What the stock versions compute is compared first: every label, and the ranges to float32 GEMM noise.

Needs a GPU; there is no host path."""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from amcpy_amd import _lib  # noqa: E402
from amcpy_amd import quantize as qz  # noqa: E402
from amcpy_amd.classifier import MlpModel, classify  # noqa: E402

ROWS, GROUPS, USED = 638_976, 6 * 26, (2, 4, 6, 8, 12, 14)
WIDTHS = (6, 26, 29, 30, 6)


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quantize_bench.py needs a GPU"
    g = torch.Generator().manual_seed(0)
    parts = []
    for l in range(4):
        parts += [torch.randn(WIDTHS[l + 1] * WIDTHS[l], generator=g) * (1.3 / WIDTHS[l] ** 0.5), torch.randn(WIDTHS[l + 1], generator=g) * 0.3]
    model = MlpModel(WIDTHS, "relu", torch.cat(parts).numpy())
    x = torch.randn((ROWS, 18), device="cuda") * torch.linspace(0.2, 4.0, 18, device="cuda") + 1.0
    cols = torch.tensor(USED, device="cuda")
    mean64, scale64 = x[:, cols].double().mean(0), x[:, cols].double().std(0)
    per_group = ROWS // GROUPS
    offsets = (torch.arange(ROWS, device="cuda") // per_group) * 6
    ranges, skipped = qz.calibrate(x, model, cols=USED, mean=mean64, scale=scale64)
    q = qz.QuantizedMlp.from_model(model, ranges)
    assert skipped == 0

    layers32 = [(torch.from_numpy(w.copy()).cuda(), torch.from_numpy(b.copy()).cuda()) for w, b in qz._layers(WIDTHS, model.params)]
    try:
        torch.ones((2, 2), dtype=torch.int64, device="cuda") @ torch.ones((2, 2), dtype=torch.int64, device="cuda")
        acc_dtype = torch.int64
    except RuntimeError:
        acc_dtype = torch.float64
    layers16 = [(torch.from_numpy(w.copy()).cuda().to(acc_dtype), torch.from_numpy(b.copy()).cuda().long()) for w, b in q.layers()]

    def standardized():
        c = (x[:, cols].double() - mean64).float()
        return (c.double() / scale64).float()

    def ours_q15():
        return qz.classify_q15(x, q, cols=USED, mean=mean64, scale=scale64, rows_per_group=per_group, want=("labels", "counts"))

    def ours_f32():
        return classify(x, model, cols=USED, mean=mean64, scale=scale64, rows_per_group=per_group, want=("labels", "counts"))

    def stock_q15():
        act = torch.clamp(standardized() * float(2 ** q.frac_input), -16384.0, 16383.0).round().to(acc_dtype)
        na = q.frac_input
        for l, (w, b) in enumerate(layers16):
            p = q.frac_weights[l] + na
            s = p - q.frac_outputs[l]
            acc = (act @ w.T).long() + (b << (p - q.frac_biases[l]))
            v = torch.clamp((acc + (1 << (s - 1))) >> s, -32768, 32767)
            act = (torch.clamp(v, min=0) if l < 3 else v).to(acc_dtype)
            na = q.frac_outputs[l]
        pred = act.argmax(1)
        return pred, torch.bincount(pred + offsets, minlength=GROUPS * 6).reshape(GROUPS, 6)

    def ours_range():
        return qz.calibrate(x, model, cols=USED, mean=mean64, scale=scale64)

    def stock_range():
        h = standardized()
        out = [torch.stack(torch.aminmax(h))]
        for l, (w, b) in enumerate(layers32):
            pre = torch.nn.functional.linear(h, w, b)
            out.append(torch.stack(torch.aminmax(pre)))
            h = torch.relu(pre)
        return torch.stack(out).cpu()          # calibrate() returns host values too

    lab, counts = ours_q15()
    pred, cnt = stock_q15()
    lab_f, _ = ours_f32()
    torch.cuda.synchronize()
    differ = int((lab.long() != pred).sum())
    assert differ == 0 and torch.equal(counts[:, :6], cnt), f"{differ} labels differ from stock PyTorch's integer network"
    agree = float((lab == lab_f).double().mean())
    assert torch.allclose(torch.from_numpy(ours_range()[0]), stock_range(), rtol=1e-4, atol=1e-5)

    fns = {"q15": ours_q15, "f32": ours_f32, "stock_q15": stock_q15, "range": ours_range, "stock_range": stock_range}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    names = list(fns)
    for r in range(a.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            t[name].append(window(fns[name], a.launches if not name.startswith("stock") else max(3, a.launches // 4)))
    med = {k: statistics.median(v) for k, v in t.items()}
    rec = {"rows": ROWS, "groups": GROUPS, "widths": list(WIDTHS), "device": torch.cuda.get_device_name(0),
           "kernels": [_lib.kernel_name_mlp_q15(0), _lib.kernel_name_mlp_q15(1)], "launches_per_window": a.launches, "rounds": a.rounds,
           "formats": q.info(), "stock_accumulator": str(acc_dtype).replace("torch.", ""),
           "labels_differing_from_stock_q15": differ, "q15_labels_agreeing_with_f32": agree,
           **{f"{k}_ms": med[k] for k in fns}, **{f"{k}_ms_all": t[k] for k in fns},
           **{f"{k}_spread": (max(t[k]) - min(t[k])) / med[k] for k in fns},
           "q15_over_f32": med["q15"] / med["f32"], "speedup_over_stock_q15": med["stock_q15"] / med["q15"],
           "range_speedup_over_stock": med["stock_range"] / med["range"], "abi": _lib.ABI_VERSION}
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
