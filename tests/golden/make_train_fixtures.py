#!/usr/bin/env python3
"""Writes the training fixtures (arrays only, .npz) from the REFERENCE's own model class and torch.optim, on the CPU:

    python tests/golden/make_train_fixtures.py --reference /path/to/reference/src

* train_steps_<case>.npz -- per case of CASES: raw feature rows `raw`, the scaler (`mean`, `scale`, `cols`), the network's
  inputs `x` (the classifier's two float32 roundings of the scaler), labels `y`, the epoch's `order`, the hyperparameters, the
  initial state dict ('sd0:<key>'), and the state after K = 4 steps of the reference's module in train() mode with dropout 0
  -- in double() ('sd64:', optimizer slots 'opt64:<slot>:<key>') and as the reference runs it, in float32 ('sd32:', 'opt32:') --
  with err32:<name> = max |theta32 - theta64| per tensor and the `cmp:<key>` masks of the elements that are compared.
  The default-shape cases are built from the reference's AMCClassifier; the others from torch.nn with its layer numbering.
* the cases of DROP_CASES also hold 'drop64:' / 'dropopt64:' / 'dropcmp:': K steps with dropout 0.4 by tests/train_ref.py
  (which tests/test_train_host.py pins to the double() states above) under the Philox masks of include/amcx.h.
* the cases of CLASS_CASES also hold 'cls64:' / 'clsopt64:' / 'clscmp:' with `y_cls` and `cls_rows`: K steps without dropout by
  tests/train_ref.py on labels of which three rows of every batch carry -1, the number of classes and 2^31 - 1.  This block has
  NO counterpart in the reference (torch raises on such a label): it states the header's sentence "a class outside
  0 ... classes - 1 matches no class" -- an all-zero one-hot, no loss term, never counted right -- and nothing else.
* train_learning.npz -- held-out accuracies of five runs (seeds 0 ... 4) of the reference's training loop, default
  hyperparameters, 3 epochs on the six Gaussian clusters of make_classifier_fixtures.clusters(6, 6, 7680, 0, seed=31): the first
  6144 rows train, the last 1536 are held out.

The generator asserts what tests/test_gpu_train.py relies on, and searches the data seed of each case until the float64 run
satisfies it: every batch variance above 1e-3; no relu pre-activation within 1e-4 of zero; the elements whose float64 gradient
is below 1e-4 of their tensor's largest at any step (unstable under rmsprop / adam in ANY float32 implementation: both divide a
gradient by about its own magnitude) are at most 1 % of each tensor, and `cmp` leaves them out.  One kind of tensor cannot
meet the 1 %: the bias of a Linear in front of a BatchNorm has a gradient that is identically zero, so its float64 gradient is
rounding noise (1e-18) with no largest element to speak of.  The rule is applied to it as to any tensor, the 1 % is not asked of it.
"""
import argparse
import copy
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
K = 4
LR = 0.001418378071933655                   # TrainingConfig.learning_rate
DEFAULT = (6, 26, 29, 30, 6)
N_ROWS = 600

# name: widths, bn_mask, activation, optimizer, batch, n_idx (None: K * batch)
CASES = {
    "default_relu_rmsprop": (DEFAULT, 7, "relu", "rmsprop", 128, None),
    "default_tanh_rmsprop": (DEFAULT, 7, "tanh", "rmsprop", 128, None),
    "default_sigmoid_rmsprop": (DEFAULT, 7, "sigmoid", "rmsprop", 128, None),
    "default_relu_adam": (DEFAULT, 7, "relu", "adam", 128, None),
    "default_tanh_adam": (DEFAULT, 7, "tanh", "adam", 128, None),
    "w_1_1_2": ((1, 1, 2), 1, "relu", "rmsprop", 128, None),
    "w_3_8_2": ((3, 8, 2), 1, "relu", "rmsprop", 128, None),
    "w_4_32_7_3": ((4, 32, 7, 3), 1, "relu", "adam", 128, None),
    "six_by_32": ((32,) * 7, 31, "tanh", "rmsprop", 128, None),      # (tanh: 82 000 relu inputs leave no seed with the margin)
    "w_7_8_9": ((6, 7, 8, 9, 6), 7, "relu", "rmsprop", 128, None),
    # (two rows: without BatchNorm.  With it every seed has a unit whose two values nearly coincide -- batch variances of 1e-6,
    #  gradients spread over many decades -- and none of 400 seeds meets the margins below;
    #  and tanh: of two rows a relu unit is often dead in both, which zeroes whole rows of a gradient)
    "batch_2": (DEFAULT, 0, "tanh", "rmsprop", 2, None),
    "batch_63": (DEFAULT, 7, "relu", "rmsprop", 63, None),
    "batch_64": (DEFAULT, 7, "relu", "rmsprop", 64, None),
    "batch_65": (DEFAULT, 7, "relu", "rmsprop", 65, None),
    "batch_256": (DEFAULT, 7, "tanh", "rmsprop", 256, None),        # (tanh: as above)
    "ragged_2": (DEFAULT, 0, "tanh", "rmsprop", 128, 3 * 128 + 2),    # (a last batch of two rows: as batch_2)
    "ragged_127": (DEFAULT, 7, "relu", "adam", 128, 3 * 128 + 127),
    # two rows THROUGH a BatchNorm: a small network (8 units, 32 unit-steps), where the seed search can meet the margins
    "batch_2_bn": ((4, 8, 3), 1, "tanh", "rmsprop", 2, None),
    "ragged_2_bn": ((4, 8, 3), 1, "tanh", "rmsprop", 128, 3 * 128 + 2),
    # the sixth kernel: sigmoid with adam
    "default_sigmoid_adam": (DEFAULT, 7, "sigmoid", "adam", 128, None),
    # mixed masks: a BatchNorm's gamma / beta, statistics and slots behind a layer that has none, a Linear bias with a real
    # gradient next to one in front of a BatchNorm, the BatchNorm backward skipped between two layers that take it.
    # (tanh on the default shape: with relu neither mask 5 nor mask 2 has a seed among 400 that meets the margins below)
    "mask_5": (DEFAULT, 0b101, "tanh", "adam", 64, None),
    "mask_2": (DEFAULT, 0b010, "tanh", "rmsprop", 65, None),
    # widths 32 (bit 31 of a dropout word, quad 7), 7 and 9 (no multiple of 4), a ragged last batch of 31 rows
    # (tanh: sigmoid with mask 9 on this shape has no seed among 400 at batch 256 or 128)
    "mask_6": ((5, 32, 7, 32, 9, 3), 0b0110, "tanh", "rmsprop", 128, 3 * 128 + 31),
    "mask_9": ((5, 32, 7, 32, 9, 3), 0b1001, "tanh", "adam", 128, None),
    # relu through a hidden layer without BatchNorm (mask 0b10; with mask 1 this shape has no seed among 400)
    "small_relu_2": ((4, 8, 8, 3), 0b10, "relu", "adam", 64, None),
}
SEEDS = {"batch_2_bn": 40000, "ragged_2_bn": 40000}          # data seeds tried per case (default 400)
DROP_P, DROP_SEED = 0.4, 0x123456789ABCDEF
# the cases that also hold a dropout run, and those that also hold a run on labels outside the classes
DROP_CASES = {"default_relu_rmsprop", "default_sigmoid_adam", "mask_5", "mask_2", "mask_6", "mask_9", "small_relu_2"}
CLASS_CASES = {"small_relu_2"}
OUTSIDE = (-1, None, 2 ** 31 - 1)                              # None: the number of classes


def outside_labels(y, order, batch, n_classes):
    """(labels, planted rows): three rows of every batch of the epoch -- its second, its middle and its last -- carry OUTSIDE."""
    y_cls, planted = np.array(y, dtype=np.int32), []
    for first in range(0, K * batch, batch):
        rows = order[first:first + batch]
        for at, label in zip((1, len(rows) // 2, len(rows) - 1), OUTSIDE):
            y_cls[rows[at]] = n_classes if label is None else label
            planted.append(rows[at])
    assert len(set(planted)) == len(planted), "the order visits a planted row twice"
    return y_cls, np.asarray(planted, dtype=np.int32)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_module(widths, bn_mask, act):
    """torch.nn with the reference's layer numbering: Linear, BatchNorm1d where the layer has one, activation, Dropout."""
    import torch.nn as nn
    act_cls = {"relu": nn.ReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid}[act]
    mods = []
    for l in range(len(widths) - 2):
        mods.append(nn.Linear(widths[l], widths[l + 1]))
        if (bn_mask >> l) & 1:
            mods.append(nn.BatchNorm1d(widths[l + 1]))
        mods += [act_cls(), nn.Dropout(0.0)]
    mods += [nn.Linear(widths[-2], widths[-1]), nn.Softmax(dim=1)]

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = nn.Sequential(*mods)

        def forward(self, x):
            return self.layers(x)

    return Net()


def run_reference(model, x, y, order, batch, optimizer, watch):
    """K steps of the reference's loop body.  Returns (state dict, optimizer slots by key, per-step gradients by key); with
    `watch` the smallest batch variance and the smallest |relu pre-activation| seen go into it."""
    import torch
    opt = (torch.optim.RMSprop if optimizer == "rmsprop" else torch.optim.Adam)(model.parameters(), lr=LR)
    loss_fn = torch.nn.CrossEntropyLoss()
    hooks = []
    if watch is not None:
        for mod in model.layers:
            if isinstance(mod, torch.nn.BatchNorm1d):
                hooks.append(mod.register_forward_hook(lambda m, i, o: watch["var"].append(float(i[0].detach().var(dim=0, unbiased=False).min()))))
            if isinstance(mod, torch.nn.ReLU):
                hooks.append(mod.register_forward_hook(lambda m, i, o: watch["act"].append(float(i[0].detach().abs().min()))))
    model.train()
    names = dict(model.named_parameters())
    grads = []
    for s in range(K):
        idx = torch.from_numpy(order[s * batch:(s + 1) * batch])
        opt.zero_grad(set_to_none=True)
        loss_fn(model(x[idx]), y[idx]).backward()
        grads.append({k: p.grad.detach().clone().numpy() for k, p in names.items()})
        opt.step()
    for h in hooks:
        h.remove()
    slots = {}
    for k, p in names.items():
        st = opt.state[p]
        for slot in (("square_avg",) if optimizer == "rmsprop" else ("exp_avg", "exp_avg_sq")):
            slots[f"{slot}:{k}"] = st[slot].detach().numpy()
    return {k: v.detach().numpy() for k, v in model.state_dict().items()}, slots, grads


def compare_masks(grads):
    out = {}
    for k in grads[0]:
        keep = np.ones(grads[0][k].shape, dtype=bool)
        for g in grads:
            keep &= np.abs(g[k]) >= 1e-4 * np.abs(g[k]).max()
        out[k] = keep
    return out


def ref_state(tref, sd, widths, bn_mask, optimizer, indices):
    """A tests/train_ref.py state of a state dict."""
    W, b, gamma, beta, rm, rv = [], [], [], [], [], []
    for l, (li, bi) in enumerate(indices):
        W.append(sd[f"layers.{li}.weight"])
        b.append(sd[f"layers.{li}.bias"])
        if l < len(indices) - 1:
            has = bi is not None
            gamma.append(sd[f"layers.{bi}.weight"] if has else None)
            beta.append(sd[f"layers.{bi}.bias"] if has else None)
            rm.append(sd[f"layers.{bi}.running_mean"] if has else None)
            rv.append(sd[f"layers.{bi}.running_var"] if has else None)
    return tref.new_state(W, b, gamma, beta, rm, rv, optimizer)


def ref_arrays(state, indices, prefix, slot_prefix, optimizer):
    """The arrays of a tests/train_ref.py state under the fixtures' key names."""
    out = {}
    slot_names = ("square_avg",) if optimizer == "rmsprop" else ("exp_avg", "exp_avg_sq")

    def put(key, part, l):
        out[f"{prefix}{key}"] = state[part][l]
        for name, slot in zip(slot_names, state["slots"]):
            out[f"{slot_prefix}{name}:{key}"] = slot[part][l]

    for l, (li, bi) in enumerate(indices):
        put(f"layers.{li}.weight", "W", l)
        put(f"layers.{li}.bias", "b", l)
        if l < len(indices) - 1 and bi is not None:
            put(f"layers.{bi}.weight", "gamma", l)
            put(f"layers.{bi}.bias", "beta", l)
            out[f"{prefix}layers.{bi}.running_mean"], out[f"{prefix}layers.{bi}.running_var"] = state["rm"][l], state["rv"][l]
    return out


def standardize(raw, cols, mean, scale):
    c = (raw[:, cols].astype(np.float64) - mean).astype(np.float32)
    return (c.astype(np.float64) / scale).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's src/ directory (holds amcpy/)")
    ap.add_argument("--only", nargs="+", default=None, metavar="CASE", help="write these cases alone (and not train_learning.npz)")
    a = ap.parse_args()
    import torch
    torch.set_num_threads(4)
    sys.path.insert(0, str(Path(a.reference).resolve()))
    sys.path.insert(0, str(REPO))
    try:
        import seaborn  # noqa: F401
    except ImportError:
        sys.modules["seaborn"] = types.ModuleType("seaborn")
    from amcpy.nn_model import AMCClassifier
    from amcpy_amd.train import layer_indices
    cf = _load("make_classifier_fixtures", HERE / "make_classifier_fixtures.py")
    tref = _load("train_ref", REPO / "tests" / "train_ref.py")

    for name, (widths, bn_mask, act, optimizer, batch, n_idx) in CASES.items():
        if a.only is not None and name not in a.only:
            continue
        n_idx = K * batch if n_idx is None else n_idx
        indices = layer_indices(widths, bn_mask)
        for seed in range(1000, 1000 + SEEDS.get(name, 400)):
            rng = np.random.default_rng(seed)
            xc, y, _ = cf.clusters(widths[-1], widths[0], N_ROWS, 0, seed=seed)
            n_cols = widths[0] + 2 if widths[0] <= 30 else widths[0]
            cols = np.arange(n_cols - widths[0], n_cols, dtype=np.int32)
            mean, scale = rng.uniform(-3.0, 3.0, widths[0]), rng.uniform(0.5, 4.0, widths[0])
            raw = rng.standard_normal((N_ROWS, n_cols)).astype(np.float32)
            raw[:, cols] = (xc.astype(np.float64) * scale + mean).astype(np.float32)
            x = standardize(raw, cols, mean, scale)
            order = (rng.permutation(N_ROWS)[:n_idx] if n_idx <= N_ROWS else rng.integers(0, N_ROWS, n_idx)).astype(np.int32)
            torch.manual_seed(seed)
            if tuple(widths) == DEFAULT and bn_mask == 7:
                model = AMCClassifier(widths[0], widths[-1], *widths[1:4], dropout=0.0, activation=act)
                assert list(model.state_dict()) == list(make_module(widths, bn_mask, act).state_dict())
            else:
                model = make_module(widths, bn_mask, act)
            sd0 = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
            watch = {"var": [], "act": []}
            sd64, opt64, grads = run_reference(copy.deepcopy(model).double(), torch.from_numpy(x.astype(np.float64)),
                                               torch.from_numpy(y.astype(np.int64)), order, batch, optimizer, watch)
            cmp = compare_masks(grads)
            # the bias of a Linear in front of a BatchNorm: its gradient is identically zero (the batch mean is subtracted), the
            # float64 run's is rounding noise of 1e-18 and no seed gives it a largest element to be measured against
            zero_grad = {f"layers.{li}.bias" for li, bi in indices if bi is not None}
            few = lambda masks: all(1.0 - m.mean() <= 0.01 for k, m in masks.items() if k not in zero_grad)
            ok = min(watch["var"], default=1.0) > 1e-3 and min(watch["act"], default=1.0) > 1e-4 and few(cmp)
            extra = {}
            st0 = ref_state(tref, sd0, widths, bn_mask, optimizer, indices)

            def restated(prefix, slot_prefix, cmp_prefix, labels, thr, keep):
                """K steps of tests/train_ref.py from sd0 under the fixtures' key names, and whether the 1 % holds for them."""
                st, sgrads = copy.deepcopy(st0), []
                for s in range(K):
                    rows = order[s * batch:(s + 1) * batch]
                    masks = tref.dropout_masks(DROP_SEED, st["t"], widths[1:-1], len(rows), thr) if thr else None
                    _, _, g = tref.step(st, x[rows].astype(np.float64), labels[rows], activation=act, optimizer=optimizer, lr=LR, masks=masks,
                                        keep_scale=keep)
                    sgrads.append(ref_arrays({**g, "slots": [], "rm": st["rm"], "rv": st["rv"]}, indices, "", "", optimizer))
                scmp = compare_masks([{k: v for k, v in g.items() if "running" not in k} for g in sgrads])
                return few(scmp), {**ref_arrays(st, indices, prefix, slot_prefix, optimizer), **{f"{cmp_prefix}{k}": v for k, v in scmp.items()}}

            if ok and name in DROP_CASES:                                 # the dropout run, by the restatement
                thr, keep = tref.drop_params(DROP_P)
                ok, arrays = restated("drop64:", "dropopt64:", "dropcmp:", y, thr, keep)
                extra.update(arrays, drop_p=DROP_P, drop_seed=np.uint64(DROP_SEED))
            if ok and name in CLASS_CASES:                                # labels outside the classes: the header's rule, not torch's
                y_cls, planted = outside_labels(y, order, batch, widths[-1])
                ok, arrays = restated("cls64:", "clsopt64:", "clscmp:", y_cls, 0, 1.0)
                extra.update(arrays, y_cls=y_cls, cls_rows=planted)
            if ok:
                break
        else:
            raise AssertionError(f"{name}: no data seed satisfies the margins")
        sd32, opt32, _ = run_reference(model, torch.from_numpy(x), torch.from_numpy(y.astype(np.int64)), order, batch, optimizer, None)
        arrays = {}
        for k in sd64:
            arrays[f"sd0:{k}"], arrays[f"sd64:{k}"], arrays[f"sd32:{k}"] = sd0[k], sd64[k], sd32[k]
            if not k.endswith("num_batches_tracked"):
                arrays[f"err32:{k}"] = np.abs(sd32[k].astype(np.float64) - sd64[k]).max()
        for k in opt64:
            arrays[f"opt64:{k}"], arrays[f"opt32:{k}"] = opt64[k], opt32[k]
            arrays[f"err32:{k}"] = np.abs(opt32[k].astype(np.float64) - opt64[k]).max()
        left_out = {**{f"cmp:{k}": m for k, m in cmp.items()}, **{k: m for k, m in extra.items() if "cmp:" in k}}
        worst = max(float(1.0 - m.mean()) for k, m in left_out.items() if k.split(":", 1)[1] not in zero_grad)
        assert worst <= 0.01, (name, worst)                         # the cap, over the plain, the dropout and the outside-class run
        print(f"{name}: data seed {seed}, smallest batch variance {min(watch['var'], default=float('nan')):.3e}, smallest |relu input| "
              f"{min(watch['act'], default=float('nan')):.3e}, most elements left out of a tensor {100 * worst:.2f} %")
        np.savez_compressed(HERE / f"train_steps_{name}.npz", raw=raw, cols=cols, mean=mean, scale=scale, x=x, y=y.astype(np.int32),
                            order=order, widths=np.asarray(widths, np.int32), bn_mask=bn_mask, activation=act, optimizer=optimizer,
                            batch=batch, lr=LR, steps=K, data_seed=seed, **arrays, **{f"cmp:{k}": v for k, v in cmp.items()}, **extra)

    if a.only is not None:
        return
    # ---- learning: the reference's loop, five seeds
    xa, ya, _ = cf.clusters(6, 6, 7680, 0, seed=31)
    xt, yt = torch.from_numpy(xa[:6144]), torch.from_numpy(ya[:6144].astype(np.int64))
    xh, yh = torch.from_numpy(xa[6144:]), ya[6144:]
    accs = []
    for seed in range(5):
        torch.manual_seed(seed)
        model = AMCClassifier(6, 6)                                          # the reference's defaults: dropout 0.4, relu
        opt = torch.optim.RMSprop(model.parameters(), lr=LR)
        loss_fn = torch.nn.CrossEntropyLoss()
        for _ in range(3):
            model.train()
            perm = torch.randperm(6144)
            for i in range(0, 6144, 128):
                idx = perm[i:i + 128]
                opt.zero_grad(set_to_none=True)
                loss_fn(model(xt[idx]), yt[idx]).backward()
                opt.step()
        model.eval()
        with torch.no_grad():
            accs.append(float((model(xh).argmax(1).numpy() == yh).mean()))
    print(f"learning: held-out accuracies {np.round(accs, 4)}")
    np.savez_compressed(HERE / "train_learning.npz", accuracies=np.asarray(accs), minimum=min(accs), spread=max(accs) - min(accs),
                        cluster_seed=31, n_train=6144, n_heldout=1536, epochs=3, batch=128, lr=LR, dropout=0.4)


if __name__ == "__main__":
    main()
