"""Training, the host side (no GPU): the float64 restatement tests/train_ref.py against the reference's own module (through the
fixtures of tests/golden/make_train_fixtures.py), the dropout generator against its published answer, the state block and its
round trips, the split, the ABI and the command line."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib, train
from amcpy_amd._mlp import i32s
from amcpy_amd.classifier import MlpModel
from amcpy_amd.config import Config
from tests import train_cases as tc
from tests import train_ref

REPO = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("name", tc.CASES)
def test_restatement_equals_the_reference_in_double(name):
    """K steps of tests/train_ref.py from the fixture's initial state against the reference's module in double() with torch.optim
    (dropout 0): every tensor, running statistics and optimizer slots included, to 1e-10."""
    case = tc.load(name)
    state, losses, _ = train_ref.run(tc.ref_state(case), case["x"].astype(np.float64), case["y"], case["order"], case["batch"],
                                     case["steps"], activation=case["activation"], optimizer=case["optimizer"], lr=case["lr"])
    got, want = tc.ref_tensors(case, state), tc.expected(case)
    assert set(got) == set(want)
    for key in want:
        assert np.abs(got[key] - want[key]).max() <= 1e-10, key
    assert state["t"] == case["steps"]
    assert all(np.isfinite(losses))


@pytest.mark.parametrize("name", tc.DROP_CASES)
def test_dropout_blocks_are_the_restatement_under_the_philox_masks(name):
    """`drop64:` / `dropopt64:` of a fixture: K steps of tests/train_ref.py with p = 0.4 and the fixture's seed; `dropcmp:` leaves
    out 1 % of a tensor at the most (the bias in front of a BatchNorm apart, as in `cmp:`)."""
    case = tc.load(name)
    thr, keep = train_ref.drop_params(float(case["drop_p"]))
    state, _, _ = train_ref.run(tc.ref_state(case), case["x"].astype(np.float64), case["y"], case["order"], case["batch"], case["steps"],
                                activation=case["activation"], optimizer=case["optimizer"], lr=case["lr"], seed=int(case["drop_seed"]),
                                threshold=thr, keep_scale=keep)
    got, want = tc.ref_tensors(case, state), tc.expected(case, "drop64:", "dropopt64:")
    assert set(got) == set(want) and all(np.abs(got[k] - want[k]).max() <= 1e-12 for k in want)
    zero_grad = {f"layers.{li}.bias" for li, bi in train.layer_indices(case["widths"], case["bn_mask"]) if bi is not None}
    for prefix in ("cmp:", "dropcmp:") + (("clscmp:",) if name in tc.CLASS_CASES else ()):
        masks = {k[len(prefix):]: v for k, v in case.items() if k.startswith(prefix)}
        assert masks and all(1.0 - m.mean() <= 0.01 for k, m in masks.items() if k not in zero_grad), prefix


def test_fixture_inputs_are_the_scaler_of_the_raw_rows():
    case = tc.load("default_relu_rmsprop")
    c = (case["raw"][:, case["cols"]].astype(np.float64) - case["mean"]).astype(np.float32)
    assert np.array_equal((c.astype(np.float64) / case["scale"]).astype(np.float32), case["x"])


def test_philox_known_answer():
    """Philox4x32-10, counter 0 and key 0 (Random123's kat_vectors); and the all-ones and pi vectors of the same file."""
    assert [f"{int(v):08x}" for v in train_ref.philox4x32_10((0, 0, 0, 0), (0, 0))] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = train_ref.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF))
    assert [f"{int(v):08x}" for v in ones] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    pi = train_ref.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    assert [f"{int(v):08x}" for v in pi] == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_dropout_masks_follow_the_counter_layout():
    masks = train_ref.dropout_masks(seed=(7 << 32) | 5, t=3, hidden_widths=[26, 9], rows=4, threshold=1 << 31)
    assert [m.shape for m in masks] == [(4, 26), (4, 9)]
    words = train_ref.philox4x32_10((3, 1, 2, 1), (5, 7))                    # layer 1, row 2, units 4 ... 7
    assert [bool(int(w) >= 1 << 31) for w in words] == list(masks[1][2, 4:8])
    assert train_ref.dropout_masks(1, 0, [5], 3, 0)[0].all()


def test_drop_threshold_and_keep_scale_rule():
    assert train.drop_params(0.0) == (0, np.float32(1.0))
    thr, keep = train.drop_params(0.4)
    assert thr == int(np.rint(0.4 * 2.0 ** 32)) == 1717986918 and keep == np.float32(1.0 / 0.6) and keep.dtype == np.float32
    assert train.drop_params(0.5) == (1 << 31, np.float32(2.0))
    assert train.drop_params(0.4) == train_ref.drop_params(0.4)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            train.drop_params(bad)


def test_state_block_layout_and_size_function():
    lib = _lib.load()
    w = (6, 26, 29, 30, 6)
    P, A = 2051, 2 * (26 + 29 + 30)
    assert train.state_floats(w, 7, "rmsprop") == (P + A) * 2 + A == lib.amcx_mlp_train_state_floats(i32s(w), 4, 7, _lib.OPT_RMSPROP)
    assert train.state_floats(w, 7, "adam") == (P + A) * 3 + A
    assert train.state_floats(w, 0, "rmsprop") == 2 * P and train.state_floats((4, 32, 7, 3), 1, "adam") == 3 * (415 + 64) + 64
    for widths, n_linear, mask, opt in ((w, 4, 8, 0), (w, 4, 7, 2), ((6, 33, 6), 2, 0, 0), (w, 0, 0, 0), ((6, 6), 1, 1, 0)):
        assert lib.amcx_mlp_train_state_floats(i32s(widths), n_linear, mask, opt) == -1
    assert lib.amcx_mlp_train_workspace_floats(i32s(w), 4, 128) == 8 + 128 * 32 * 10
    assert lib.amcx_mlp_train_workspace_floats(i32s(w), 4, 1) == lib.amcx_mlp_train_workspace_floats(i32s(w), 4, 257) == -1
    st = train.TrainState.init(w, 7, "adam", [3, 4])
    assert st.block.shape == (2, train.state_floats(w, 7, "adam")) and st.steps.tolist() == [0, 0]
    v = st.views(0)
    assert v["layers.0.weight"].shape == (26, 6) and np.abs(v["layers.0.weight"]).max() <= 1 / np.sqrt(6) and v["layers.0.weight"].std() > 0.1
    assert (v["layers.1.weight"] == 1).all() and (v["layers.1.bias"] == 0).all() and (v["layers.1.running_var"] == 1).all()
    assert not (st.block[0, P + A + A:]).any() and not np.array_equal(st.block[0], st.block[1])
    assert np.array_equal(train.TrainState.init(w, 7, "adam", [3]).block[0], st.block[0])
    # the header's order: parameters, then gamma / beta, then the running statistics, then the slots
    st.block[0] = np.arange(st.state_floats)
    assert st.views(0)["layers.0.weight"][0, 0] == 0 and st.views(0)["layers.1.weight"][0] == P and st.views(0)["layers.1.bias"][0] == P + 26
    assert st.views(0)["layers.1.running_mean"][0] == P + A and st.views(0)["layers.1.running_var"][0] == P + A + 26
    assert st.views(0, 1)["layers.0.weight"][0, 0] == P + 2 * A and st.views(0, 2)["layers.12.bias"][-1] == st.state_floats - A - 1


def test_state_block_size_is_the_library_s_for_every_fixture_shape():
    """TrainState's own layout arithmetic against amcx_mlp_train_state_floats, over every shape, mask and optimizer of the fixtures."""
    shapes = {(tc.load(name)["widths"], tc.load(name)["bn_mask"], tc.load(name)["optimizer"]) for name in tc.CASES}
    assert len({w for w, _, _ in shapes}) >= 6 and {o for _, _, o in shapes} == {"rmsprop", "adam"} and len({m for _, m, _ in shapes}) >= 2
    # mixed masks, where the offsets of a BatchNorm are not those of a per-layer formula: three distinct ones at least
    assert len({m for w, m, _ in shapes if m != 0 and m != (1 << (len(w) - 2)) - 1}) >= 3
    for widths, bn_mask, optimizer in sorted(shapes):
        want = train.state_floats(widths, bn_mask, optimizer)
        for n_models in (1, 3):
            st = train.TrainState(widths, bn_mask, optimizer, np.zeros(n_models * want, np.float32), np.zeros(n_models, np.int64))
            assert st.state_floats == want == train.layout(widths, bn_mask, optimizer)["state_floats"] and st.block.shape == (n_models, want)
            assert st.n_train == st.n_params + st.n_affine and st.n_slots == (2 if optimizer == "adam" else 1)
        assert train.TrainState.init(widths, bn_mask, optimizer, [1, 2]).block.shape == (2, want)


def test_state_block_layout_under_a_mixed_mask():
    """(5, 32, 7, 32, 9, 3), BatchNorm behind the first and the fourth hidden layer only, adam: the first index of every view
    against the header's rule (THE STATE BLOCK) worked out here by hand, not by layer_indices or layout.
    Parameters W then b per layer: 5x32 at 0 / 160, 32x7 at 192 / 416, 7x32 at 423 / 647, 32x9 at 679 / 967, 9x3 at 976 / 1003,
    P = 1006.  BatchNorms (widths 32 and 9), gamma then beta each: 1006 / 1038, 1070 / 1079, T = 1088.  Running mean then variance
    each: 1088 / 1120, 1152 / 1161, T + R = 1170.  Slots of T values: exp_avg from 1170, exp_avg_sq from 2258; 3346 in all.
    In the reference's Sequential the Linears are modules 0, 4, 7, 10, 14 and the BatchNorms 1 and 11."""
    w, mask = (5, 32, 7, 32, 9, 3), 0b1001
    P, T, R = 1006, 1088, 82
    assert train.state_floats(w, mask, "adam") == 3 * T + R == 3346
    st = train.TrainState.init(w, mask, "adam", [1])
    assert st.block.shape == (1, 3346) and (st.n_params, st.n_affine, st.n_train) == (P, R, T)
    st.block[0] = np.arange(3346)
    trainable = {"layers.0.weight": (0, (32, 5)), "layers.0.bias": (160, (32,)), "layers.4.weight": (192, (7, 32)),
                 "layers.4.bias": (416, (7,)), "layers.7.weight": (423, (32, 7)), "layers.7.bias": (647, (32,)),
                 "layers.10.weight": (679, (9, 32)), "layers.10.bias": (967, (9,)), "layers.14.weight": (976, (3, 9)),
                 "layers.14.bias": (1003, (3,)), "layers.1.weight": (1006, (32,)), "layers.1.bias": (1038, (32,)),
                 "layers.11.weight": (1070, (9,)), "layers.11.bias": (1079, (9,))}
    running = {"layers.1.running_mean": (1088, (32,)), "layers.1.running_var": (1120, (32,)), "layers.11.running_mean": (1152, (9,)),
               "layers.11.running_var": (1161, (9,))}
    for part, base, want in ((0, 0, {**trainable, **running}), (1, 1170, trainable), (2, 2258, trainable)):
        views = st.views(0, part)
        assert set(views) == set(want), part
        for key, (first, shape) in want.items():
            at = first if key in running else base + first
            assert views[key].shape == shape and views[key].reshape(-1)[0] == at and views[key].reshape(-1)[-1] == at + np.prod(shape) - 1, (part, key)
    # every float of the block belongs to exactly one view
    seen = np.concatenate([v.reshape(-1) for part in range(3) for v in st.views(0, part).values()])
    assert np.array_equal(np.sort(seen), np.arange(3346))


@pytest.mark.parametrize("name", ("mask_5", "mask_2", "mask_6", "mask_9", "small_relu_2"))
def test_state_dict_round_trip_under_a_mixed_mask(name):
    """from_state_dict finds the mask in the keys of the reference's state dict; to_state_dict gives every tensor back."""
    case = tc.load(name)
    sd = tc.state_dict(case, "sd32:")
    st = train.TrainState.from_state_dict(sd, case["optimizer"])
    assert st.bn_mask == case["bn_mask"] and st.widths == case["widths"] and st.steps.tolist() == [case["steps"]]
    back = st.to_state_dict(0)
    assert set(back) == set(sd) and all(np.array_equal(back[k].numpy(), sd[k]) for k in sd)
    again = train.TrainState.from_state_dict(back, case["optimizer"])
    assert again.bn_mask == case["bn_mask"] and np.array_equal(again.block, st.block) and np.array_equal(again.steps, st.steps)
    assert train.TrainState.from_state_dict(sd, case["optimizer"], steps=2 ** 32 + 3).steps.tolist() == [2 ** 32 + 3]


def test_restatement_of_a_class_outside_the_classes():
    """The header: "a class outside 0 ... classes - 1 matches no class".  In tests/train_ref.py such a row adds nothing to the loss
    and nothing to the count, and its dp is q / rows (an all-zero one-hot): the gradients against a second, direct statement of
    a (4, 5, 3) tanh network without BatchNorm, written out here.  The reference has no such rule (torch raises)."""
    rng = np.random.default_rng(11)
    rows, labels = 6, np.array([0, -1, 2, 3, 2 ** 31 - 1, 1])
    x = rng.standard_normal((rows, 4))
    W0, b0, W1, b1 = rng.standard_normal((5, 4)), rng.standard_normal(5), rng.standard_normal((3, 5)), rng.standard_normal(3)
    state = train_ref.new_state([W0, W1], [b0, b1], [None], [None], [None], [None], "rmsprop")
    loss, right, g = train_ref.step(state, x, labels, activation="tanh", optimizer="rmsprop", lr=1e-3)
    # the direct statement, row by row
    inside = [r for r in range(rows) if 0 <= labels[r] < 3]
    assert inside == [0, 2, 5]
    dW0, db0, dW1, db1, want_loss, want_right = np.zeros_like(W0), np.zeros_like(b0), np.zeros_like(W1), np.zeros_like(b1), 0.0, 0
    for r in range(rows):
        a = np.tanh(W0 @ x[r] + b0)
        e = np.exp(W1 @ a + b1)
        p = e / e.sum()
        q = np.exp(p) / np.exp(p).sum()
        dp = q / rows
        if r in inside:
            dp[labels[r]] -= 1.0 / rows
            want_loss -= np.log(q[labels[r]])
            want_right += int(np.argmax(p) == labels[r])
        dz = (np.diag(p) - np.outer(p, p)) @ dp                     # the softmax's Jacobian
        da = (W1.T @ dz) * (1.0 - a * a)
        dW1, db1, dW0, db0 = dW1 + np.outer(dz, a), db1 + dz, dW0 + np.outer(da, x[r]), db0 + da
    assert abs(loss - want_loss) <= 1e-12 * want_loss and right == want_right
    for got, want in ((g["W"][0], dW0), (g["b"][0], db0), (g["W"][1], dW1), (g["b"][1], db1)):
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # the rows outside alone: no loss, none right -- and still a gradient
    alone = train_ref.new_state([W0, W1], [b0, b1], [None], [None], [None], [None], "rmsprop")
    loss, right, g = train_ref.step(alone, x[[1, 3, 4]], labels[[1, 3, 4]], activation="tanh", optimizer="rmsprop", lr=1e-3)
    assert loss == 0.0 and right == 0 and np.abs(g["W"][1]).max() > 0.0


def test_planted_rows_of_the_outside_class_fixture_add_nothing():
    """tests/golden/train_steps_small_relu_2.npz: three rows of every batch carry -1, the number of classes and 2^31 - 1; the
    restatement's loss and count over those rows alone are 0 at every step, so the history a kernel is held to in
    tests/test_gpu_train.py is that of the other rows.  And the `cls64:` block is the restatement's state."""
    case = tc.load("small_relu_2")
    y, y_cls, planted, batch = case["y"], case["y_cls"], case["cls_rows"], case["batch"]
    assert len(planted) == 3 * case["steps"] and sorted(set(y_cls[planted].tolist())) == [-1, len(set(y.tolist())), 2 ** 31 - 1]
    assert len(set(y.tolist())) == case["widths"][-1]
    others = np.setdiff1d(np.arange(len(y)), planted)
    assert np.array_equal(y_cls[others], y[others])
    for s in range(case["steps"]):
        rows = case["order"][s * batch:(s + 1) * batch]
        assert np.array_equal(np.flatnonzero(np.isin(rows, planted)), [1, batch // 2, batch - 1])
        assert y_cls[rows[[1, batch // 2, batch - 1]]].tolist() == [-1, case["widths"][-1], 2 ** 31 - 1]
    kw = dict(activation=case["activation"], optimizer=case["optimizer"], lr=case["lr"])
    state = tc.ref_state(case)
    for s in range(case["steps"]):
        rows = case["order"][s * batch:(s + 1) * batch]
        only = rows[np.isin(rows, planted)]
        probe = train_ref.copy.deepcopy(state)
        loss, right, _ = train_ref.step(probe, case["x"][only].astype(np.float64), y_cls[only], **kw)
        assert loss == 0.0 and right == 0, s
        train_ref.step(state, case["x"][rows].astype(np.float64), y_cls[rows], **kw)
    got, want = tc.ref_tensors(case, state), tc.expected(case, "cls64:", "clsopt64:")
    assert set(got) == set(want) and all(np.abs(got[k] - want[k]).max() <= 1e-12 for k in want)
    plain = tc.expected(case)
    assert max(np.abs(want[k] - plain[k]).max() / np.abs(plain[k]).max() for k in want if "running" not in k) > 1e-3      # and it matters


def test_state_dict_checkpoint_and_model_round_trip(tmp_path):
    case = tc.load("w_4_32_7_3")
    sd = tc.state_dict(case, "sd32:")
    st = train.TrainState.from_state_dict(sd, "adam")
    assert st.widths == (4, 32, 7, 3) and st.bn_mask == 1 and st.steps.tolist() == [4]
    back = st.to_state_dict(0)
    assert set(back) == set(sd) and all(np.array_equal(back[k].numpy(), sd[k]) for k in sd)
    want = MlpModel.from_state_dict(sd, "tanh")
    assert np.array_equal(st.model(0, "tanh").params, want.params)
    path = train.save_checkpoint(tmp_path / "ann" / "model-abc.pt", st, 0, "abc", {"training": {"activation": "tanh", "epochs": 3}})
    got = MlpModel.from_checkpoint(path, activation="tanh")
    assert got.model_id == "abc" and got.widths == want.widths and np.array_equal(got.params, want.params)
    import torch
    ck = torch.load(str(path), map_location="cpu", weights_only=True)          # plain: tensors, strings and dicts only
    assert ck["config"] == {"training": {"activation": "tanh", "epochs": 3}} and ck["model_id"] == "abc"
    assert int(ck["model_state_dict"]["layers.1.num_batches_tracked"]) == 4


def test_a_written_checkpoint_is_loaded_with_the_activation_it_was_trained_with(tmp_path):
    """`train --activation tanh` then `classify --model ID`: the id alone must bring the activation back, in both forms of the
    plain-dict config, and the command line's default must not replace it."""
    from amcpy_amd.classifier import load_model
    from amcpy_amd.config import Paths
    cfg = Config(paths=Paths(root=tmp_path))
    assert cfg.training.activation == "relu"
    st = train.TrainState.from_state_dict(tc.state_dict(tc.load("w_4_32_7_3"), "sd32:"), "adam")
    for model_id, act, settings in (("t1", "tanh", {"training": {"activation": "tanh"}}), ("s1", "sigmoid", {"activation": "sigmoid"}),
                                    ("r1", "relu", {"training": {"epochs": 3}})):
        train.save_checkpoint(cfg.paths.trained_ann / f"model-{model_id}.pt", st, 0, model_id, settings)
        model, got_id = load_model(cfg, model_id)
        assert (got_id, model.activation, model.widths) == (model_id, act, (4, 32, 7, 3))
    assert train._settings(cfg)["activation"] == "relu" and isinstance(train._settings(cfg)["training_snr"], list)


def test_stratified_split_keeps_every_class_share():
    rng = np.random.default_rng(0)
    y = np.repeat(np.arange(6), [600, 600, 300, 900, 50, 1200])[rng.permutation(3650)]
    tr, te = train.stratified_split(y, 0.2, 42)
    assert len(np.intersect1d(tr, te)) == 0 and np.array_equal(np.sort(np.concatenate([tr, te])), np.arange(3650))
    assert np.bincount(y[te]).tolist() == [120, 120, 60, 180, 10, 240]
    again = train.stratified_split(y, 0.2, 42)
    assert np.array_equal(again[1], te) and not np.array_equal(train.stratified_split(y, 0.2, 43)[1], te)


def test_abi_16_1_in_header_binding_and_library():
    """Training adds entries and constants and changes nothing that exists: the version stays 16 and the minor number counts the
    addition."""
    lib = _lib.load()
    assert (_lib.ABI_VERSION, _lib.ABI_MINOR) >= (16, 1) and (lib.amcx_abi_version(), lib.amcx_abi_minor()) >= (16, 1)
    header = (REPO / "include" / "amcx.h").read_text()
    assert re.search(r"^#define AMCX_ABI_MINOR (\d+)$", header, re.M) and "#define AMCX_OPT_RMSPROP 0" in header and "#define AMCX_OPT_ADAM 1" in header
    assert "ABI 16.1: AMCX_ABI_MINOR 1" in header and header.index("ABI 16.1: AMCX_ABI_MINOR 1") < header.index("ABI 16: the line above")
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ("amcx_mlp_train_f32", "amcx_mlp_train_state_floats", "amcx_mlp_train_workspace_floats", "amcx_kernel_name_mlp_train", "amcx_abi_minor"):
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header) and re.search(rf" T {name}$", exported, re.M), name
    assert _lib.kernel_name_mlp_train("relu", "rmsprop") == "amcx_mlp_train_kernel<0, 0>"
    assert _lib.kernel_name_mlp_train("sigmoid", "adam") == "amcx_mlp_train_kernel<2, 1>"
    with pytest.raises(ValueError):
        _lib.kernel_name_mlp_train("relu", "nadam")


def test_train_kernels_are_in_the_resource_table_without_scratch_and_older_kernels_kept_their_bytes():
    import json
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    names = [f"amcx_mlp_train_kernel<{a}, {o}>" for a in range(3) for o in range(2)] + ["amcx_mlp_train_hyper_kernel"]
    for name in names:
        assert table[name]["spill"] == 0 and table[name]["scratch"] == 0, name
    listing = (REPO / "profiles" / "r27_train_codeobj_kernels.txt").read_text()
    assert "DIFFERENT" not in listing and "ONLY IN A" not in listing and "93 kernels / device functions identical" in listing
    assert sorted(re.findall(r"ONLY IN B\s+amcx::(.+)", listing)) == sorted(names)


def test_train_command_in_the_parser():
    from amcpy_amd.main import build_parser
    a = build_parser().parse_args(["train", "--root", "/r", "--epochs", "3", "--batch-size", "64", "--lr", "0.01", "--dropout", "0.1",
                                   "--optimizer", "adam", "--activation", "tanh", "--seed", "5", "--sweep-lr", "0.01,0.02",
                                   "--sweep-dropout", "0.1,0.2", "--device", "0"])
    assert (a.command, a.epochs, a.batch_size, a.lr, a.dropout, a.optimizer, a.activation, a.seed) == ("train", 3, 64, 0.01, 0.1, "adam", "tanh", 5)
    assert a.sweep_lr == "0.01,0.02" and a.sweep_dropout == "0.1,0.2" and a.device == 0
    d = build_parser().parse_args(["train"])
    assert d.epochs is None and d.optimizer is None and d.sweep_lr is None


def test_nadam_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="nadam"):
        train.TrainState.init((6, 8, 6), 1, "nadam", [0])
    with pytest.raises(NotImplementedError, match="nadam"):
        train.check_optimizer("nadam")
    from dataclasses import replace
    cfg = Config()
    with pytest.raises(NotImplementedError, match="nadam"):
        train.train_model(replace(cfg, training=replace(cfg.training, optimizer="nadam")))
    with pytest.raises(ValueError):
        train.check_optimizer("sgd")
