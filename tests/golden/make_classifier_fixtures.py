#!/usr/bin/env python3
"""Writes the classifier fixtures (arrays only, .npz) from the REFERENCE's own model class, on the CPU:

    python tests/golden/make_classifier_fixtures.py --reference /path/to/reference/src

* classifier_ref_{relu,tanh,sigmoid}.npz -- the reference's AMCClassifier(6, 6, activation=...) trained by the short
  loop below (train() mode, so BatchNorm's running statistics are real) on six separated Gaussian clusters: its
  state_dict as arrays ('sd:<key>'), 8192 input rows `x` (cluster points and points between clusters), `p32` = the
  module as the reference runs it (float32, eval()), `p64` = the same module in double(), ref32_err = max|p32 - p64|.
* classifier_ref_odd.npz -- the same for a network of other widths (4 -> 32 -> 7 -> 3, tanh, the second block
  without BatchNorm), built from torch.nn with the reference's layer numbering.
* classifier_synth6.npz -- a default-shape model trained the same way on the CPU checker's features (columns
  FeatureConfig.used) of amcpy_amd.synth.host_block frames of MODS6, N = 1024, SNR 10 ... 20 dB, with the fitted
  scaler and, for held-out seeds, the CPU chain's probabilities, labels and accuracy.

The generator asserts what the tests rely on: every class wins >= 5 % of the rows, at most 0.05 % of the rows have a
p64 top-two margin below 8 x ref32_err, held-out accuracy > 0.5.  The reference imports seaborn at module level
(plots only); an empty stand-in module is registered when it is not installed.
"""
import argparse
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
USED = (2, 4, 6, 8, 12, 14)                       # FeatureConfig.used, taken as 0-based columns
SNRS = (10.0, 12.0, 14.0, 16.0, 18.0, 20.0)
N_FRAME, TRAIN_FRAMES, HELD_FRAMES = 1024, 60, 30


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def train(model, x, y, steps=400, lr=1e-2, batch=256, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    loss_fn = torch.nn.CrossEntropyLoss()           # on the softmax output, as the reference's train_model does
    xt, yt = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.int64))
    model.train()
    for _ in range(steps):
        idx = torch.randint(0, xt.shape[0], (batch,), generator=g)
        opt.zero_grad(set_to_none=True)
        loss_fn(model(xt[idx]), yt[idx]).backward()
        opt.step()
    model.eval()
    return model


def run_both(model, x):
    """(p32 as the reference runs it, p64 of the same module in double())."""
    import copy
    import torch
    with torch.no_grad():
        p32 = model(torch.from_numpy(x.astype(np.float32))).numpy()
        p64 = copy.deepcopy(model).double()(torch.from_numpy(x.astype(np.float64))).numpy()
    return p32, p64


def clusters(n_classes, dim, n_cluster, n_between, seed):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((n_classes, dim)) * 2.0
    y = rng.integers(0, n_classes, n_cluster)
    x = centers[y] + 0.6 * rng.standard_normal((n_cluster, dim))
    a, b = rng.integers(0, n_classes, n_between), rng.integers(0, n_classes, n_between)
    t = rng.uniform(0.0, 1.0, (n_between, 1))
    between = t * centers[a] + (1 - t) * centers[b] + 0.3 * rng.standard_normal((n_between, dim))
    return x.astype(np.float32), y, between.astype(np.float32)


def checks(name, p32, p64, href):
    err = float(np.abs(p32.astype(np.float64) - p64).max())
    wins = np.bincount(p64.argmax(1), minlength=p64.shape[1]) / p64.shape[0]
    close = float((href.top_two_margin(p64) < 8 * err).mean())
    print(f"{name}: ref32_err {err:.3e}, class shares {np.round(wins, 3)}, rows under the margin {close:.5f}")
    assert wins.min() >= 0.05, f"{name}: a class wins under 5 % of the rows"
    assert close <= 0.0005, f"{name}: {close} of the rows are closer than 8 x ref32_err"
    return err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's src/ directory (holds amcpy/)")
    a = ap.parse_args()
    import torch
    torch.manual_seed(1234)
    torch.set_num_threads(4)
    sys.path.insert(0, str(Path(a.reference).resolve()))
    sys.path.insert(0, str(REPO))
    try:
        import seaborn  # noqa: F401
    except ImportError:
        sys.modules["seaborn"] = types.ModuleType("seaborn")
    from amcpy.nn_model import AMCClassifier
    href = _load("classifier_host_ref", REPO / "tests" / "classifier_host_ref.py")
    from amcpy_amd.classifier import MlpModel

    def fold_report(name, model, act, x, p64, err):
        m = MlpModel.from_state_dict(model.state_dict(), act)
        d32 = np.abs(href.forward64(x, m.widths, m.params, act) - p64).max()
        d64 = np.abs(href.forward64(x, m.widths, m.params64, act) - p64).max()
        print(f"{name}: fold rounded to float32 moves p by {d32:.3e} = {d32 / err:.2f} x ref32_err; "
              f"un-rounded float64 fold {d64:.2e}")

    def sd_arrays(model):
        return {f"sd:{k}": v.detach().numpy() for k, v in model.state_dict().items()}

    for i, act in enumerate(("relu", "tanh", "sigmoid")):
        xc, y, xb = clusters(6, 6, 6144, 2048, seed=10 + i)
        model = train(AMCClassifier(6, 6, activation=act), xc, y, seed=i)
        x = np.concatenate([xc, xb])
        p32, p64 = run_both(model, x)
        err = checks(f"ref_{act}", p32, p64, href)
        fold_report(f"ref_{act}", model, act, x, p64, err)
        np.savez_compressed(HERE / f"classifier_ref_{act}.npz", x=x, p32=p32, p64=p64, ref32_err=err,
                            activation=act, **sd_arrays(model))

    nn = torch.nn

    class Odd(nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = nn.Sequential(nn.Linear(4, 32), nn.BatchNorm1d(32), nn.Tanh(), nn.Dropout(0.4),
                                        nn.Linear(32, 7), nn.Tanh(), nn.Dropout(0.4), nn.Linear(7, 3), nn.Softmax(dim=1))

        def forward(self, x):
            return self.layers(x)

    xc, y, xb = clusters(3, 4, 6144, 2048, seed=20)
    model = train(Odd(), xc, y, seed=5)
    x = np.concatenate([xc, xb])
    p32, p64 = run_both(model, x)
    err = checks("ref_odd", p32, p64, href)
    fold_report("ref_odd", model, "tanh", x, p64, err)
    np.savez_compressed(HERE / "classifier_ref_odd.npz", x=x, p32=p32, p64=p64, ref32_err=err, activation="tanh",
                        **sd_arrays(model))

    # ---- end to end: synthetic frames -> CPU checker features -> scaler -> the reference's model
    from amcpy_amd import synth
    from oracle import iq_features_oracle as orc

    def frames(seed_base, n):
        xs, ys, seeds = [], [], []
        for mi, mod in enumerate(synth.MODS6):
            for si, snr in enumerate(SNRS):
                seed = seed_base + 100 * mi + si
                xs.append(synth.host_block(mod, snr, n, N_FRAME, seed=seed))
                ys.append(np.full(n, mi))
                seeds.append((mi, snr, seed))
        return np.concatenate(xs).astype(np.complex64), np.concatenate(ys), np.asarray(seeds, dtype=np.float64)

    iq_tr, y_tr, _ = frames(5000, TRAIN_FRAMES)
    iq_ho, y_ho, seeds_ho = frames(9000, HELD_FRAMES)
    f_tr = np.asarray(orc.features18_batch(iq_tr), dtype=np.float64)[:, list(USED)]
    f_ho = np.asarray(orc.features18_batch(iq_ho), dtype=np.float64)
    mean, scale = f_tr.mean(axis=0), f_tr.std(axis=0)
    model = train(AMCClassifier(6, 6), ((f_tr - mean) / scale).astype(np.float32), y_tr, seed=7)
    x_ho = href.standardize64(f_ho, USED, mean, scale)
    p32, p64 = run_both(model, x_ho)
    err = float(np.abs(p32.astype(np.float64) - p64).max())
    labels = p64.argmax(1)
    acc = float((labels == y_ho).mean())
    per_mod = [float((labels[y_ho == k] == k).mean()) for k in range(6)]
    close = float((href.top_two_margin(p64) < 8 * err).mean())
    print(f"synth6: held-out accuracy {acc:.4f} per modulation {np.round(per_mod, 3)}, ref32_err {err:.3e}, "
          f"rows under the margin {close:.5f} of {len(labels)}")
    assert acc > 0.5 and close <= 0.0005
    np.savez_compressed(HERE / "classifier_synth6.npz", mean=mean, scale=scale, cols=np.asarray(USED, np.int32),
                        heldout_seeds=seeds_ho, heldout_frames=HELD_FRAMES, frame_size=N_FRAME, true=y_ho.astype(np.int32),
                        labels=labels.astype(np.int32), p64=p64, ref32_err=err, accuracy=acc, activation="relu",
                        **sd_arrays(model))


if __name__ == "__main__":
    main()
