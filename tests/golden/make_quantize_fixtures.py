#!/usr/bin/env python3
"""Writes the fixed-point fixtures (arrays only, .npz) from the REFERENCE's own ``quantize`` (nn_quantization.py), on the CPU:

    python tests/golden/make_quantize_fixtures.py --reference /path/to/reference/src

It imports the reference's ``nn_quantization`` and ``config`` and nothing else of it (``nn_model`` needs seaborn), builds
``torch.nn.Sequential`` networks of its own with ``requires_grad_(False)`` -- the reference's ``quantize`` calls ``.numpy()`` on
the parameters and raises on a model as ``load_model`` leaves it -- and calls ``quantize`` with a ``Config`` rooted in a
temporary directory.  Each ``quantize_ref_{name}.npz`` holds the state_dict arrays ('sd:<key>'), the sample input ``x``, the
reference's int16 ``weights`` and ``biases``, its ``info`` strings (``info_keys`` / ``info_values``), the shapes and dtypes
``loadmat`` sees in the ``w_and_b.mat`` it wrote (``mat_names`` / ``mat_shapes`` / ``mat_dtypes``), and ``ranges``: (min, max)
of the input and of every ``Linear``'s output along the chain ``quantize`` walks (the ``Linear`` layers alone), by its torch calls.

* ``default``: the reference's 6-26-29-30-6 with BatchNorm1d (its layer numbering), random parameters and statistics.
* ``spread``: 5-9-7-4 whose weights, biases and inputs spread the formats from Q0.15 to Q6.9 and go beyond +-32, so the
  fallback and its clamp are hit.
* ``ties``: 4-8-3 with values exactly on half steps of their format (ties to even) and exactly at a format's two ends.

The script asserts that no recorded range lies within 1e-4 (relative) of a format boundary: float32 sums taken in another
order (a GEMM, the device's FMAs) then cannot disagree with these about a format.
"""
import argparse
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


def block(n_in, n_out, norm):
    import torch
    mods = [torch.nn.Linear(n_in, n_out)]
    if norm:
        mods += [torch.nn.BatchNorm1d(n_out), torch.nn.ReLU(), torch.nn.Dropout(0.1)]
    else:
        mods += [torch.nn.ReLU()]
    return mods


def default_net(gen):
    import torch
    widths = (6, 26, 29, 30, 6)
    mods = []
    for l in range(3):
        mods += block(widths[l], widths[l + 1], True)
    mods += [torch.nn.Linear(widths[3], widths[4]), torch.nn.Softmax(dim=1)]
    net = torch.nn.Sequential(*mods)
    for m in net.modules():
        if isinstance(m, torch.nn.Linear):
            m.weight.data = torch.randn(m.weight.shape, generator=gen) * (1.2 / np.sqrt(m.weight.shape[1]))
            m.bias.data = torch.randn(m.bias.shape, generator=gen) * 0.3
        if isinstance(m, torch.nn.BatchNorm1d):
            m.weight.data = 0.5 + torch.rand(m.weight.shape, generator=gen)
            m.bias.data = torch.randn(m.bias.shape, generator=gen) * 0.2
            m.running_mean = torch.randn(m.running_mean.shape, generator=gen) * 0.4
            m.running_var = 0.3 + torch.rand(m.running_var.shape, generator=gen) * 2.0
    x = (torch.randn((512, 6), generator=gen) * 1.5).numpy()
    return net, x


def spread_net(gen):
    import torch
    net = torch.nn.Sequential(torch.nn.Linear(5, 9), torch.nn.ReLU(), torch.nn.Linear(9, 7), torch.nn.ReLU(), torch.nn.Linear(7, 4))
    u = lambda shape, a: (torch.rand(shape, generator=gen) * 2 - 1) * a      # noqa: E731
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    # weights: Q0.15, Q3.12, beyond +-32 (fallback, clamped); biases: Q1.14, beyond +-32, Q5.10; input: Q2.13
    for m, aw, ab in zip(lin, (0.4, 3.5, 50.0), (0.9, 40.0, 12.0)):
        m.weight.data, m.bias.data = u(m.weight.shape, aw), u(m.bias.shape, ab)
    lin[1].bias.data[0], lin[1].bias.data[1] = 39.0, -37.5
    lin[2].weight.data[0, 0], lin[2].weight.data[1, 1] = 49.0, -48.0
    x = u((300, 5), 1.7).numpy()
    return net, x


def ties_net(gen):
    import torch
    net = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.ReLU(), torch.nn.Linear(8, 3))
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    # layer 1 weights in Q0.15: both ends, and odd multiples of 2^-16 (exact halves of a step: ties go to even)
    k = torch.randint(-16384, 16383, (8, 4), generator=gen).to(torch.float64)
    w = (k + 0.5) * 2.0 ** -15
    w[0, 0], w[0, 1], w[1, 0], w[1, 1] = -0.5, 0.5 - 2.0 ** -15, 0.5 * 2.0 ** -15, -0.5 * 2.0 ** -15
    lin[0].weight.data = w.to(torch.float32)
    # layer 1 biases in Q2.13: both ends and halves of a step
    kb = torch.randint(-16384, 16383, (8,), generator=gen).to(torch.float64)
    b = (kb + 0.5) * 2.0 ** -13
    b[0], b[1], b[2], b[3] = -2.0, 2.0 - 2.0 ** -13, 1.5 * 2.0 ** -13, 2.5 * 2.0 ** -13
    lin[0].bias.data = b.to(torch.float32)
    # layer 2 weights in Q4.11 (ends and halves), biases in Q6.9 (its ends: the widest format's own)
    k2 = torch.randint(-16384, 16383, (3, 8), generator=gen).to(torch.float64)
    w2 = (k2 + 0.5) * 2.0 ** -11
    w2[0, 0], w2[0, 1] = -8.0, 8.0 - 2.0 ** -11
    lin[1].weight.data = w2.to(torch.float32)
    lin[1].bias.data = torch.tensor([-32.0, 32.0 - 2.0 ** -9, 0.5 * 2.0 ** -9], dtype=torch.float32)
    x = ((torch.rand((257, 4), generator=gen) * 2 - 1) * 0.9).numpy()
    return net, x


def boundaries():
    out = []
    for m in range(7):
        n = 15 - m
        out += [-(2.0 ** (m - 1)), 2.0 ** (m - 1) - 2.0 ** (-n)]
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, type=Path, help="the reference's src/ directory")
    a = ap.parse_args()
    sys.path.insert(0, str(a.reference))
    import scipy.io
    import torch
    from amcpy import nn_quantization as nq
    from amcpy.config import Config, Paths

    gen = torch.Generator().manual_seed(20240607)
    for name, make in (("default", default_net), ("spread", spread_net), ("ties", ties_net)):
        net, x = make(gen)
        net.eval()
        net.requires_grad_(False)
        x = np.ascontiguousarray(x, dtype=np.float32)
        with tempfile.TemporaryDirectory() as tmp:
            cfg = Config(paths=Paths(root=Path(tmp)))
            cfg.paths.arm_data.mkdir(parents=True, exist_ok=True)
            save, info = nq.quantize(net, x, cfg)
            mat = {k: v for k, v in scipy.io.loadmat(str(cfg.paths.arm_data / "w_and_b.mat")).items() if not k.startswith("__")}
        assert all(np.array_equal(mat[k].reshape(-1), save[k]) for k in save)
        ranges = [(float(np.min(x)), float(np.max(x)))]
        t = torch.from_numpy(x).float()
        with torch.no_grad():
            for layer in [m for m in net.modules() if isinstance(m, torch.nn.Linear)]:
                t = layer(t)
                ranges.append((float(t.min()), float(t.max())))
        ranges = np.asarray(ranges, dtype=np.float32)
        # what decides a format: the input's two ends, every layer's maximum
        deciding = [ranges[0][0], ranges[0][1]] + [r[1] for r in ranges[1:]]
        for v in deciding:
            for bnd in boundaries():
                assert abs(v - bnd) > 1e-4 * abs(bnd), (name, v, bnd)
        keys = sorted(info)
        sd = {f"sd:{k}": v.detach().cpu().numpy() for k, v in net.state_dict().items()}
        mat_names = sorted(mat)
        np.savez(HERE / f"quantize_ref_{name}.npz", x=x, weights=save["weights"], biases=save["biases"],
                 info_keys=np.asarray(keys), info_values=np.asarray([info[k] for k in keys]), ranges=ranges,
                 mat_names=np.asarray(mat_names), mat_shapes=np.asarray([mat[k].shape for k in mat_names], dtype=np.int64),
                 mat_dtypes=np.asarray([str(mat[k].dtype) for k in mat_names]), **sd)
        print(name, {k: info[k] for k in keys}, (HERE / f"quantize_ref_{name}.npz").stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
