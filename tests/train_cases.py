"""What tests/test_train_host.py and tests/test_gpu_train.py share: the fixtures of tests/golden/make_train_fixtures.py as
:class:`amcpy_amd.train.TrainState` blocks and tests/train_ref.py states, and the comparison of a trained block with a fixture's
float64 state under the issue's bound."""
from functools import lru_cache
from pathlib import Path

import numpy as np

from amcpy_amd.train import TrainState, layer_indices
from tests import train_ref

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = ("default_relu_rmsprop", "default_tanh_rmsprop", "default_sigmoid_rmsprop", "default_relu_adam", "default_tanh_adam",
         "w_1_1_2", "w_3_8_2", "w_4_32_7_3", "six_by_32", "w_7_8_9", "batch_2", "batch_63", "batch_64", "batch_65", "batch_256",
         "ragged_2", "ragged_127", "batch_2_bn", "ragged_2_bn", "default_sigmoid_adam", "mask_5", "mask_2", "mask_6", "mask_9",
         "small_relu_2")
DROP_CASES = ("default_relu_rmsprop", "default_sigmoid_adam", "mask_5", "mask_2", "mask_6", "mask_9", "small_relu_2")   # hold drop64:
CLASS_CASES = ("small_relu_2",)                                                                                        # hold cls64:
SLOTS = {"rmsprop": ("square_avg",), "adam": ("exp_avg", "exp_avg_sq")}


@lru_cache(maxsize=None)
def load(name):
    with np.load(GOLDEN / f"train_steps_{name}.npz") as z:
        case = {k: z[k] for k in z.files}
    case["name"] = name
    for k in ("activation", "optimizer"):
        case[k] = str(case[k])
    for k in ("bn_mask", "batch", "steps"):
        case[k] = int(case[k])
    case["widths"] = tuple(int(w) for w in case["widths"])
    case["lr"] = float(case["lr"])
    return case


def state_dict(case, prefix="sd0:"):
    return {k[len(prefix):]: v for k, v in case.items() if k.startswith(prefix)}


def initial_state(case, n_models=1) -> TrainState:
    return TrainState.from_state_dict([state_dict(case)] * n_models, case["optimizer"], steps=0)


def ref_state(case, prefix="sd0:"):
    """The tests/train_ref.py state of a fixture's state dict (fresh slots)."""
    sd, idx = state_dict(case, prefix), layer_indices(case["widths"], case["bn_mask"])
    hidden = idx[:-1]
    pick = lambda name: [None if bi is None else sd[f"layers.{bi}.{name}"] for _, bi in hidden]
    return train_ref.new_state([sd[f"layers.{li}.weight"] for li, _ in idx], [sd[f"layers.{li}.bias"] for li, _ in idx], pick("weight"),
                               pick("bias"), pick("running_mean"), pick("running_var"), case["optimizer"])


def ref_tensors(case, state) -> dict:
    """A tests/train_ref.py state under the fixtures' names: ``<key>`` and ``<slot>:<key>``."""
    idx, out = layer_indices(case["widths"], case["bn_mask"]), {}
    for l, (li, bi) in enumerate(idx):
        parts = [(f"layers.{li}.weight", "W"), (f"layers.{li}.bias", "b")]
        if bi is not None:
            parts += [(f"layers.{bi}.weight", "gamma"), (f"layers.{bi}.bias", "beta")]
            out[f"layers.{bi}.running_mean"], out[f"layers.{bi}.running_var"] = state["rm"][l], state["rv"][l]
        for key, part in parts:
            out[key] = state[part][l]
            for name, slot in zip(SLOTS[case["optimizer"]], state["slots"]):
                out[f"{name}:{key}"] = slot[part][l]
    return out


def block_tensors(case, st: TrainState, m=0) -> dict:
    """Model m of a TrainState under the same names."""
    out = dict(st.views(m))
    for s, name in enumerate(SLOTS[case["optimizer"]]):
        out.update({f"{name}:{k}": v for k, v in st.views(m, 1 + s).items()})
    return out


def expected(case, prefix="sd64:", slot_prefix="opt64:") -> dict:
    out = {k[len(prefix):]: v for k, v in case.items() if k.startswith(prefix) and not k.endswith("num_batches_tracked")}
    out.update({k[len(slot_prefix):]: v for k, v in case.items() if k.startswith(slot_prefix)})
    return out


def worst_ratio(case, got: dict, want: dict, cmp_prefix="cmp:") -> tuple:
    """The largest |got - want| / (4 max(err32, 2^-24 max |want|)) over the compared elements of every tensor, and its tensor.
    err32 is the tensor's in the fixture: max |theta32 - theta64| of the reference's own float32 run."""
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    worst = (0.0, None)
    for key, w in want.items():
        param = key.split(":")[-1]
        mask = case.get(cmp_prefix + param)
        mask = np.ones(w.shape, dtype=bool) if mask is None else mask
        bound = 4.0 * max(float(case[f"err32:{key}"]), 2.0 ** -24 * float(np.abs(w).max()))
        diff = np.abs(np.asarray(got[key], dtype=np.float64) - w)[mask]
        if diff.size and (worst[1] is None or float(diff.max()) / bound > worst[0]):
            worst = (float(diff.max()) / bound, key)
    return worst
