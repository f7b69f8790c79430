#!/usr/bin/env python3
"""Timing of the training kernel, default network (6 -> 26 -> 29 -> 30 -> 6, relu, BatchNorm, dropout 0.4), batch 128, rmsprop:

    python tools/train_bench.py [--rounds 5] [--steps 37] [--out profiles/NAME.json]

Rows as the training split of BASELINE configs[0]: 6 modulations x 2 SNRs x 500 frames = 6000 rows, 80 % of them = 4800, so an
epoch is 37 full steps and a ragged one; the 37 full steps are timed.

* (a) time per step at ONE model -- one amcx_mlp_train_f32 launch of `steps` steps -- against STOCK PYTORCH on the same device
  running the same steps: the reference's module built from torch.nn in train(), CrossEntropyLoss on its softmax output,
  torch.optim.RMSprop, the batch gathered by index.  Device events, the two alternating round by round, medians with the spread.
* (b) time per launch of the same steps at n_models = 1, 16, 64, 256, 512.

Needs a GPU; there is no host path."""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from amcpy_amd import _lib  # noqa: E402
from amcpy_amd.train import Trainer, TrainState  # noqa: E402

WIDTHS, ROWS, BATCH, LR, DROPOUT = (6, 26, 29, 30, 6), 4800, 128, 0.001418378071933655, 0.4
USED = (2, 4, 6, 8, 12, 14)
MODELS = (1, 16, 64, 256, 512)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=ROWS // BATCH)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "train_bench.py needs a GPU"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    y = rng.integers(0, 6, ROWS)
    x = torch.randn((ROWS, 18), device="cuda") + torch.from_numpy(y).cuda()[:, None] * 0.5
    cols = torch.tensor(USED, device="cuda")
    mean64, scale64 = x[:, cols].double().mean(0), x[:, cols].double().std(0)
    order = rng.permutation(ROWS)

    def trainer(n):
        st = TrainState.init(WIDTHS, 7, "rmsprop", range(n))
        tr = Trainer(x, y, st, cols=USED, mean=mean64, scale=scale64, batch_size=BATCH, activation="relu", lr=LR, dropout=DROPOUT,
                     seed=list(range(n)))
        return tr, tr.device_order(order)

    nn = torch.nn
    seq = nn.Sequential(nn.Linear(6, 26), nn.BatchNorm1d(26), nn.ReLU(), nn.Dropout(DROPOUT),
                        nn.Linear(26, 29), nn.BatchNorm1d(29), nn.ReLU(), nn.Dropout(DROPOUT),
                        nn.Linear(29, 30), nn.BatchNorm1d(30), nn.ReLU(), nn.Dropout(DROPOUT),
                        nn.Linear(30, 6), nn.Softmax(dim=1)).cuda().train()
    opt = torch.optim.RMSprop(seq.parameters(), lr=LR)
    loss_fn = nn.CrossEntropyLoss()
    xs = ((x[:, cols] - mean64.float()) / scale64.float()).contiguous()
    yt, perm = torch.from_numpy(y).cuda(), torch.from_numpy(order).cuda()

    def stock():
        for i in range(0, a.steps * BATCH, BATCH):                   # the reference's loop body, without its .item() calls
            idx = perm[i:i + BATCH]
            opt.zero_grad(set_to_none=True)
            loss_fn(seq(xs[idx]), yt[idx]).backward()
            opt.step()

    runs = {n: trainer(n) for n in MODELS}

    def ours(n):
        tr, (order_dev, n_idx, stride) = runs[n]
        return lambda: tr.launch(order_dev, n_idx, stride, 0, a.steps)

    for fn in [stock] + [ours(n) for n in MODELS]:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {"stock": [], **{n: [] for n in MODELS}}
    for r in range(a.rounds):
        names = ["stock", *MODELS] if r % 2 == 0 else [*reversed(MODELS), "stock"]
        for name in names:
            t[name].append(timed(stock if name == "stock" else ours(name)))
    med = {k: statistics.median(v) for k, v in t.items()}
    rec = {"widths": list(WIDTHS), "rows": ROWS, "batch": BATCH, "steps_per_launch": a.steps, "optimizer": "rmsprop", "dropout": DROPOUT,
           "kernel": _lib.kernel_name_mlp_train("relu", "rmsprop"), "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "step_us_one_model": med[1] / a.steps * 1e3, "step_us_one_model_spread": spread(t[1]),
           "stock_pytorch_step_us": med["stock"] / a.steps * 1e3, "stock_pytorch_spread": spread(t["stock"]),
           "speedup_over_stock_pytorch_one_model": med["stock"] / med[1],
           "launch_ms_by_models": {str(n): med[n] for n in MODELS}, "launch_ms_all": {str(k): v for k, v in t.items()},
           "launch_spread_by_models": {str(n): spread(t[n]) for n in MODELS},
           "launch_time_over_one_model": {str(n): med[n] / med[1] for n in MODELS},
           "model_steps_per_s": {str(n): n * a.steps / (med[n] * 1e-3) for n in MODELS},
           "speedup_over_stock_pytorch_per_model": {str(n): n * med["stock"] / med[n] for n in MODELS}, "abi": _lib.ABI_VERSION}
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
