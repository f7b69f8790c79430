#!/usr/bin/env python3
"""Timing of the classifier launch on 638 976 x 18 resident rows, default network (6 -> 26 -> 29 -> 30 -> 6, relu):

    python tools/bench_classify.py [--rounds 5] [--launches 20] [--out profiles/NAME.json]

* `classify` (labels + counts, one amcx_mlp_classify_f32 call) against STOCK PYTORCH on the same device doing what the
  reference's evaluate_by_snr does: rows[:, cols], (x - mean) / scale, the eval-mode nn.Sequential built from the same
  weights, .argmax(1), and a bincount per group.  Both are timed between device events, >= 20 launches per window,
  in the same process, the two alternating round by round; the medians over the rounds are reported with the spread.
* the same call as a fraction of one N = 2048 extraction launch (features18) of as many frames.
* what the two compute is compared first: labels equal on all but rows closer than the float32 noise.

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
from amcpy_amd.classifier import MlpModel, classify  # noqa: E402
from amcpy_amd.features import features18  # noqa: E402

ROWS, GROUPS, USED = 638_976, 6 * 26, (2, 4, 6, 8, 12, 14)


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
    ap.add_argument("--frames-2048", type=int, default=ROWS, help="frames of the extraction launch it is compared with")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_classify.py needs a GPU"
    torch.manual_seed(0)
    nn = torch.nn
    seq = nn.Sequential(nn.Linear(6, 26), nn.BatchNorm1d(26), nn.ReLU(), nn.Dropout(0.4),
                        nn.Linear(26, 29), nn.BatchNorm1d(29), nn.ReLU(), nn.Dropout(0.4),
                        nn.Linear(29, 30), nn.BatchNorm1d(30), nn.ReLU(), nn.Dropout(0.4),
                        nn.Linear(30, 6), nn.Softmax(dim=1))
    for m in seq:                                        # running statistics and affine terms that are not the identity
        if isinstance(m, nn.BatchNorm1d):
            m.running_mean.normal_(0.0, 0.5)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0.0, 0.3)
    seq.eval()
    model = MlpModel.from_state_dict({f"layers.{k}": v for k, v in seq.state_dict().items()}, "relu")
    seq = seq.cuda()
    x = torch.randn((ROWS, 18), device="cuda") * torch.linspace(0.2, 4.0, 18, device="cuda") + 1.0
    cols = torch.tensor(USED, device="cuda")
    mean64 = x[:, cols].double().mean(0)
    scale64 = x[:, cols].double().std(0)
    mean32, scale32 = mean64.float(), scale64.float()
    per_group = ROWS // GROUPS
    offsets = (torch.arange(ROWS, device="cuda") // per_group) * 6

    def ours():
        return classify(x, model, cols=USED, mean=mean64, scale=scale64, rows_per_group=per_group, want=("labels", "counts"))

    def stock():
        with torch.no_grad():
            pred = seq((x[:, cols] - mean32) / scale32).argmax(1)
            return pred, torch.bincount(pred + offsets, minlength=GROUPS * 6).reshape(GROUPS, 6)

    lab, counts = ours()
    pred, cnt = stock()
    torch.cuda.synchronize()
    differ = int((lab.long() != pred).sum())
    assert differ <= ROWS // 10_000, f"{differ} labels differ from stock PyTorch"
    assert int((counts[:, :6] - cnt).abs().sum()) <= 2 * differ and int(counts[:, 6].sum()) == 0

    iq = torch.randn((a.frames_2048, 2048), device="cuda", dtype=torch.complex64)
    feats = torch.empty((a.frames_2048, 18), device="cuda")

    def extract():
        return features18(iq, out=feats)

    for fn in (ours, stock, extract):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {"classify": [], "stock": [], "extract": []}
    for r in range(a.rounds):
        order = (("classify", ours), ("stock", stock)) if r % 2 == 0 else (("stock", stock), ("classify", ours))
        for name, fn in order:
            t[name].append(window(fn, a.launches))
        t["extract"].append(window(extract, max(3, a.launches // 4)))
    med = {k: statistics.median(v) for k, v in t.items()}
    widths = model.widths
    fma = sum(-(-widths[l + 1] // 8) * 8 * -(-widths[l] // 8) * 8 for l in range(len(widths) - 1))
    rec = {"rows": ROWS, "groups": GROUPS, "widths": list(widths), "kernel": "amcx_mlp_classify_kernel",
           "device": torch.cuda.get_device_name(0), "launches_per_window": a.launches, "rounds": a.rounds,
           "classify_ms": med["classify"], "classify_ms_all": t["classify"],
           "stock_pytorch_ms": med["stock"], "stock_pytorch_ms_all": t["stock"],
           "speedup_over_stock_pytorch": med["stock"] / med["classify"],
           "labels_differing_from_stock": differ,
           "extract_2048_frames": a.frames_2048, "extract_2048_ms": med["extract"], "extract_2048_ms_all": t["extract"],
           "classify_fraction_of_extract_2048": med["classify"] / med["extract"] * a.frames_2048 / ROWS,
           "fma_per_row_padded": fma, "fma_per_s": fma * ROWS / (med["classify"] * 1e-3),
           "matrix_GBps": ROWS * 18 * 4 / (med["classify"] * 1e-3) / 1e9,
           "abi": _lib.ABI_VERSION}
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    assert med["classify"] <= med["stock"], "the classifier launch is slower than stock PyTorch"


if __name__ == "__main__":
    main()
