"""Training on the device: the reference's ``train`` stage (``nn_model.train_model``: its ``AMCClassifier`` in ``train()``
mode, ``CrossEntropyLoss`` on the softmax output, RMSprop or Adam) as ONE workgroup per model and a bounded number of steps per
launch (amcpy_amd/csrc/amcx_mlp_train_kernel.h behind ``amcx_mlp_train_f32``, ABI 16.1).  Several models -- a sweep over learning
rate, dropout and seed -- train side by side in one launch.

* :class:`TrainState` -- the state blocks of ``n_models`` models of one shape (parameters, BatchNorm, optimizer slots, step
  counts), to and from the reference's ``state_dict``.
* :class:`Trainer` -- the device side: features resident, one call per epoch.
* :func:`train_model` -- the reference's loop; :func:`save_checkpoint` -- the file its ``load_model`` reads.

Differences from the reference, all deliberate: the train / validation split is this module's own stratified split from a seeded
numpy generator (not sklearn's permutation); dropout draws from Philox4x32-10 as include/amcx.h states (not torch's generator);
``nadam`` is not built.  Nothing here trains on the host: without the library or a GPU these functions raise.
"""
from __future__ import annotations

import ctypes
import uuid
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._mlp import check_widths, i32s, params_floats, row_plan

OPTIMIZERS = {"rmsprop": _lib.OPT_RMSPROP, "adam": _lib.OPT_ADAM}
MAX_BATCH = 256
MAX_MODELS_PER_LAUNCH = 256
DEFAULT_STEPS_PER_LAUNCH = 64          # a launch of 64 steps of the default shape stays in the milliseconds


def check_optimizer(name: str) -> str:
    if name == "nadam":
        raise NotImplementedError("optimizer 'nadam' is not built on the device: rmsprop or adam")
    if name not in OPTIMIZERS:
        raise ValueError(f"optimizer {name!r}: one of {sorted(OPTIMIZERS)}")
    return name


def drop_params(p: float) -> tuple:
    """``(drop_threshold, keep_scale)`` of a dropout probability: ``rint(p * 2^32)`` and ``float32(1 / (1 - p))``."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout {p}: 0 <= p < 1")
    return min(int(np.rint(p * 2.0 ** 32)), 2 ** 32 - 1), np.float32(1.0 / (1.0 - p))


def layer_indices(widths, bn_mask: int) -> list:
    """``[(index of the Linear, index of its BatchNorm1d or None)]`` in the reference's Sequential: Linear, BatchNorm where the
    layer has one, activation, Dropout per hidden layer, then the last Linear."""
    out, at = [], 0
    for l in range(len(widths) - 1):
        hidden = l + 1 < len(widths) - 1
        bn = hidden and (bn_mask >> l) & 1
        out.append((at, at + 1 if bn else None))
        at += 1 + (1 if bn else 0) + 2
    return out


def check_bn_mask(widths, bn_mask: int) -> int:
    bn_mask = int(bn_mask)
    if bn_mask < 0 or bn_mask >> (len(widths) - 2):
        raise ValueError(f"bn_mask {bn_mask:#x}: one bit per hidden layer ({len(widths) - 2})")
    return bn_mask


def layout(widths, bn_mask: int, optimizer: str) -> dict:
    """The sizes of a state block (include/amcx.h): ``n_params`` packed parameters, ``n_affine`` gammas and betas (as many running
    statistics), ``n_train`` = both; ``n_slots`` optimizer slots of ``n_train`` values each; ``state_floats`` in all."""
    widths = check_widths(widths)
    n_params = params_floats(widths)
    n_affine = sum(2 * widths[l + 1] for l in range(len(widths) - 2) if (bn_mask >> l) & 1)
    n_train, n_slots = n_params + n_affine, 2 if check_optimizer(optimizer) == "adam" else 1
    return dict(n_params=n_params, n_affine=n_affine, n_train=n_train, n_slots=n_slots, state_floats=n_train * (1 + n_slots) + n_affine)


class TrainState:
    """``n_models`` models of one shape as ``amcx_mlp_train_f32`` takes them: ``block`` float32 ``(n_models, state_floats)`` in the
    header's layout -- the packed parameters ``[0, P)``, gamma and beta of every BatchNorm ``[P, T)``, running mean and variance
    ``[T, T + R)``, then the optimizer's slots of ``T`` values each -- and ``steps`` int64 ``(n_models,)``."""

    def __init__(self, widths, bn_mask: int, optimizer: str, block, steps):
        self.widths = check_widths(widths)
        self.bn_mask = check_bn_mask(self.widths, bn_mask)
        self.optimizer = check_optimizer(optimizer)
        self.bn_layers = [l for l in range(len(self.widths) - 2) if (self.bn_mask >> l) & 1]
        vars(self).update(layout(self.widths, self.bn_mask, self.optimizer))      # n_params, n_affine, n_train, n_slots, state_floats
        self.block = np.ascontiguousarray(block, dtype=np.float32).reshape(-1, self.state_floats)
        self.steps = np.ascontiguousarray(steps, dtype=np.int64).reshape(-1)
        if self.steps.shape[0] != self.block.shape[0] or not self.block.shape[0]:
            raise ValueError("one step count per model, one model at least")

    n_models = property(lambda self: self.block.shape[0])
    n_linear = property(lambda self: len(self.widths) - 1)

    def views(self, m: int, part: int = 0) -> dict:
        """Views into model m's block by the reference's key names: ``part`` 0 the values themselves (with the running statistics),
        1 ... the optimizer's slots of the trainable ones."""
        row, out, at = self.block[m], {}, 0
        base = 0 if part == 0 else self.n_train + self.n_affine + (part - 1) * self.n_train
        idx = layer_indices(self.widths, self.bn_mask)
        for l, (li, _) in enumerate(idx):
            n_in, n_out = self.widths[l], self.widths[l + 1]
            out[f"layers.{li}.weight"] = row[base + at:base + at + n_out * n_in].reshape(n_out, n_in)
            out[f"layers.{li}.bias"] = row[base + at + n_out * n_in:base + at + n_out * n_in + n_out]
            at += n_out * n_in + n_out
        run = self.n_train
        for l in self.bn_layers:
            bi, n = idx[l][1], self.widths[l + 1]
            out[f"layers.{bi}.weight"], out[f"layers.{bi}.bias"] = row[base + at:base + at + n], row[base + at + n:base + at + 2 * n]
            if part == 0:
                out[f"layers.{bi}.running_mean"], out[f"layers.{bi}.running_var"] = row[run:run + n], row[run + n:run + 2 * n]
            at, run = at + 2 * n, run + 2 * n
        return out

    @classmethod
    def init(cls, widths, bn_mask: int, optimizer: str, seeds: Sequence[int]) -> "TrainState":
        """One model per seed, initialised as torch initialises ``Linear`` (weights and biases uniform in +- 1 / sqrt(inputs)) and
        ``BatchNorm1d`` (gamma 1, beta 0, running mean 0, running variance 1), drawn from a CPU generator seeded with it."""
        import torch
        seeds = [int(s) for s in seeds]
        st = cls(widths, bn_mask, optimizer, np.zeros((len(seeds), layout(widths, bn_mask, optimizer)["state_floats"]), np.float32),
                 np.zeros(len(seeds), np.int64))
        for m, seed in enumerate(seeds):
            g = torch.Generator(device="cpu").manual_seed(seed)
            for key, v in st.views(m).items():
                if key.endswith("running_mean"):
                    v[...] = 0.0
                elif key.endswith("running_var") or (v.ndim == 1 and key.endswith("weight")):
                    v[...] = 1.0
            for l, (li, _) in enumerate(layer_indices(st.widths, st.bn_mask)):
                bound = 1.0 / np.sqrt(st.widths[l])
                for name in ("weight", "bias"):
                    v = st.views(m)[f"layers.{li}.{name}"]
                    v[...] = ((torch.rand(v.shape, generator=g, dtype=torch.float32) * 2.0 - 1.0) * bound).numpy()
        return st

    @classmethod
    def from_state_dict(cls, sds, optimizer: str = "rmsprop", steps=None) -> "TrainState":
        """From one ``state_dict`` of the reference's layout or a list of them (one model each, one shape): fresh optimizer slots;
        the step counts from ``num_batches_tracked`` unless ``steps`` gives them.  A model has ONE count, BatchNorm's and the
        optimizer's: to go on training a loaded model with adam pass ``steps=0`` -- its moments start at zero, and a bias
        correction for step t + 1 on zero moments makes the first updates about ten times too small."""
        from .classifier import _KEY, _array
        if isinstance(sds, dict):
            sds = [sds]
        first = {str(k): _array(v) for k, v in sds[0].items()}
        lin = sorted(int(_KEY.match(k).group(1)) for k, v in first.items() if k.endswith("weight") and v.ndim == 2)
        norms = sorted(int(_KEY.match(k).group(1)) for k in first if k.endswith("running_mean"))
        widths = [first[f"layers.{lin[0]}.weight"].shape[1]] + [first[f"layers.{i}.weight"].shape[0] for i in lin]
        bn_mask = sum(1 << l for l, i in enumerate(lin) if i + 1 in norms)
        st = cls(widths, bn_mask, optimizer, np.zeros((len(sds), layout(widths, bn_mask, optimizer)["state_floats"]), np.float32), np.zeros(len(sds), np.int64))
        for m, sd in enumerate(sds):
            sd = {str(k): _array(v) for k, v in sd.items()}
            views = st.views(m)
            if set(views) != {k for k in sd if not k.endswith("num_batches_tracked")}:
                raise ValueError("state_dict: the keys do not describe the shape of the first one")
            for key, v in views.items():
                v[...] = sd[key].reshape(v.shape)
            tracked = [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")]
            st.steps[m] = tracked[0] if tracked and steps is None else 0
        if steps is not None:
            st.steps[:] = steps
        return st

    def to_state_dict(self, m: int = 0) -> dict:
        """Model m as the reference's ``state_dict`` (torch tensors; ``num_batches_tracked`` = the step count)."""
        import torch
        out = {}
        for key, v in self.views(m).items():
            out[key] = torch.from_numpy(np.array(v))
            if key.endswith("running_var"):
                out[key[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(int(self.steps[m]), dtype=torch.long)
        return out

    def model(self, m: int = 0, activation: str = "relu", model_id: Optional[str] = None):
        """The :class:`amcpy_amd.classifier.MlpModel` of model m: every BatchNorm folded with its running statistics."""
        from .classifier import MlpModel
        return MlpModel.from_state_dict(self.to_state_dict(m), activation, model_id)


def state_floats(widths, bn_mask: int, optimizer: str) -> int:
    """``amcx_mlp_train_state_floats``: what the library says (ValueError for a shape it refuses)."""
    widths = [int(w) for w in widths]
    n = _lib.load().amcx_mlp_train_state_floats(i32s(widths), len(widths) - 1, int(bn_mask), OPTIMIZERS[check_optimizer(optimizer)])
    if n < 0:
        raise ValueError(f"amcx: no state block for widths {tuple(widths)}, bn_mask {bn_mask:#x}")
    return int(n)


def _per_model(v, n: int, dtype, name: str):
    a = np.asarray(v, dtype=dtype).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, n)
    if a.size != n:
        raise ValueError(f"{name}: one value, or one per model ({n})")
    return np.ascontiguousarray(a)


class Trainer:
    """The device side of a training run.  ``feats``: float32 CUDA tensor ``(..., rows, C)``, resident; ``y``: the class of every
    row of the flattened matrix; ``state``: a :class:`TrainState`, uploaded here and brought back by :meth:`download`; ``cols``,
    ``mean``, ``scale`` as :func:`amcpy_amd.classifier.classify` takes them; ``lr``, ``dropout``, ``seed``: one value or one per
    model; ``idx``: the rows that are the training set (default: all), which an epoch's ``order`` indexes."""

    def __init__(self, feats, y, state: TrainState, *, cols, mean=None, scale=None, batch_size: int = 128, activation: str = "relu",
                 lr=1e-3, dropout=0.0, seed=0, idx=None):
        import torch
        if activation not in _lib.ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: one of {sorted(_lib.ACTIVATIONS)}")
        if not 2 <= int(batch_size) <= MAX_BATCH:
            raise ValueError(f"batch_size {batch_size}: 2 ... {MAX_BATCH}")
        self.state, self.activation, self.batch = state, activation, int(batch_size)
        self.rows = row_plan(feats, state.widths[0], cols, mean, scale)
        dev, n = self.rows.device, state.n_models
        self.y = torch.as_tensor(np.asarray(y.cpu() if hasattr(y, "cpu") else y).astype(np.int32).reshape(-1)).to(dev)
        if self.y.shape[0] != self.rows.n_rows:
            raise ValueError(f"y: one class per row ({self.rows.n_rows}), got {self.y.shape[0]}")
        self.idx = None if idx is None else np.asarray(idx, dtype=np.int64).reshape(-1)
        self.lr = _per_model(lr, n, np.float32, "lr")
        drops = [drop_params(p) for p in _per_model(dropout, n, np.float64, "dropout")]
        self.threshold = np.ascontiguousarray([d[0] for d in drops], dtype=np.uint32)
        self.keep_scale = np.ascontiguousarray([d[1] for d in drops], dtype=np.float32)
        self.seed = _per_model(seed, n, np.uint64, "seed")
        lib = _lib.load()
        ws = lib.amcx_mlp_train_workspace_floats(i32s(state.widths), state.n_linear, self.batch)
        self.block = torch.from_numpy(state.block.copy()).to(dev)
        self.steps = torch.from_numpy(state.steps.copy()).to(dev)
        self.ws = torch.zeros((n, ws), dtype=torch.float32, device=dev)
        self.history = torch.zeros((n, 2), dtype=torch.float64, device=dev)

    def launch(self, order_dev, n_idx: int, model_stride: int, step0: int, n_steps: int) -> None:
        """One call of ``amcx_mlp_train_f32`` on the current stream: steps ``step0 ... step0 + n_steps - 1`` of the epoch whose order
        ``order_dev`` (int32, on the device) holds."""
        from . import _stream
        s, f, u = self.state, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
        _stream.launch(self.rows.flat, lambda lib, stream: lib.amcx_mlp_train_f32(
            *self.rows.entry_args(), self.y.data_ptr(), order_dev.data_ptr(), int(n_idx), int(model_stride), i32s(s.widths), s.n_linear,
            _lib.ACTIVATIONS[self.activation], s.bn_mask, OPTIMIZERS[s.optimizer], self.batch, s.n_models, self.block.data_ptr(),
            self.steps.data_ptr(), self.ws.data_ptr(), self.lr.ctypes.data_as(f), self.threshold.ctypes.data_as(u),
            self.keep_scale.ctypes.data_as(f), self.seed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(step0), int(n_steps),
            self.history.data_ptr(), stream))

    def device_order(self, order):
        """An epoch's order -- positions in ``idx`` (rows, without it), ``(n,)`` for every model or ``(n_models, n)`` -- as the
        entry takes it: ``(int32 device tensor, n_idx, model stride)``."""
        import torch
        order = np.asarray(order.cpu() if hasattr(order, "cpu") else order, dtype=np.int64)
        if order.ndim not in (1, 2) or (order.ndim == 2 and order.shape[0] != self.state.n_models):
            raise ValueError("order: (n,) or (n_models, n)")
        limit = self.rows.n_rows if self.idx is None else self.idx.size
        if order.size and (order.min() < 0 or order.max() >= limit):
            raise ValueError(f"order: positions 0 ... {limit - 1}")
        rows = order if self.idx is None else self.idx[order]
        if rows.size and (rows.min() < 0 or rows.max() >= self.rows.n_rows):
            raise ValueError(f"idx: rows 0 ... {self.rows.n_rows - 1}")
        dev = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(self.rows.device)
        return dev, order.shape[-1], (order.shape[-1] if order.ndim == 2 else 0)

    def run_epoch(self, order, steps_per_launch: int = DEFAULT_STEPS_PER_LAUNCH) -> tuple:
        """One epoch in launches of at most ``steps_per_launch`` steps.  Returns ``(loss, accuracy)``, float64 arrays with one
        entry per model: the mean row loss and the share of rows classified right, as the reference's ``history`` has them."""
        if steps_per_launch < 1:
            raise ValueError("steps_per_launch: 1 at least")
        order_dev, n_idx, stride = self.device_order(order)
        n_steps = (n_idx + self.batch - 1) // self.batch
        self.history.zero_()
        for step0 in range(0, n_steps, steps_per_launch):
            self.launch(order_dev, n_idx, stride, step0, min(steps_per_launch, n_steps - step0))
        h = self.history.cpu().numpy()
        return h[:, 0] / n_idx, h[:, 1] / n_idx

    def download(self) -> TrainState:
        """The state as it stands on the device, into ``state`` (and returned)."""
        self.state.block[...] = self.block.cpu().numpy()
        self.state.steps[...] = self.steps.cpu().numpy()
        return self.state


def stratified_split(y, test_size: float, random_state: int) -> tuple:
    """``(train rows, test rows)``, sorted: of every class ``round(test_size * its rows)`` rows, chosen by a numpy generator
    seeded with ``random_state``, go to the test set.  Not sklearn's permutation."""
    y = np.asarray(y).reshape(-1)
    rng = np.random.default_rng(int(random_state))
    test = []
    for cls in np.unique(y):
        members = np.flatnonzero(y == cls)
        test.append(rng.permutation(members)[:int(round(float(test_size) * members.size))])
    test = np.sort(np.concatenate(test))
    train = np.setdiff1d(np.arange(y.size), test)
    return train, test


def _settings(cfg) -> dict:
    t = cfg.training
    return {name: (list(v) if isinstance(v, tuple) else v) for name, v in ((n, getattr(t, n)) for n in t.__dataclass_fields__)}


def save_checkpoint(path, state: TrainState, m: int, model_id: str, settings: dict) -> Path:
    """The file the reference's ``train_model`` writes -- ``{"model_state_dict", "model_id", "config"}`` -- with the settings as a
    plain dict (``{"training": {...}}`` or the training settings themselves), so that nothing but torch is needed to load it."""
    import torch
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save({"model_state_dict": state.to_state_dict(m), "model_id": str(model_id), "config": dict(settings)}, str(path))
    return path


def train_model(cfg, feats_by_mod=None, *, device=None, sweep: Optional[dict] = None, verbose: bool = True,
                steps_per_launch: int = DEFAULT_STEPS_PER_LAUNCH) -> tuple:
    """The reference's ``train_model`` on the device.  The rows are those its ``preprocess_data(cfg, "training")`` stacks (every
    modulation, ``training_snr``; ``feats_by_mod`` ``(n_mods, n_snr, n_frames, 18)`` on the GPU, or read from the feature files by
    :func:`amcpy_amd.classifier.fit_scaler`), standardised by the scaler fitted on them, split by :func:`stratified_split`
    (``test_size``, ``random_state``).  Per epoch: a ``torch.randperm`` order, :meth:`Trainer.run_epoch`, validation through
    :func:`amcpy_amd.classifier.classify` on the folded model.  ``sweep``: lists ``lr`` / ``dropout`` / ``seed`` of one length, one
    model each, 256 at most.  Returns ``(state, model ids, histories)``, a history per model under the reference's four names."""
    import torch
    from .classifier import classify, fit_scaler
    from .postprocess import select_standardize
    t, sig = cfg.training, cfg.signals
    optimizer = check_optimizer(t.optimizer)
    sweep = dict(sweep or {})
    if set(sweep) - {"lr", "dropout", "seed"}:
        raise ValueError("sweep: lists under lr, dropout, seed")
    n = max([len(v) for v in sweep.values()] + [1])
    if n > MAX_MODELS_PER_LAUNCH or any(len(v) != n for v in sweep.values()):
        raise ValueError(f"sweep: lists of one length, {MAX_MODELS_PER_LAUNCH} models at most")
    lrs = list(sweep.get("lr", [t.learning_rate] * n))
    drops = list(sweep.get("dropout", [t.dropout] * n))
    seeds = [int(s) for s in sweep.get("seed", range(t.random_state, t.random_state + n))]
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device)) if not isinstance(device, torch.device) else device
    cols = [int(c) for c in cfg.features.used]
    snr_axis = list(t.training_snr)
    with torch.cuda.device(dev):
        if feats_by_mod is None:
            feats, mean, scale = fit_scaler(cfg, "training", dev)
        else:
            feats = feats_by_mod if isinstance(feats_by_mod, torch.Tensor) else torch.stack(list(feats_by_mod))
            feats = feats.to(dev)
            _, mean, scale = select_standardize(feats[:, torch.tensor(snr_axis, device=dev)].reshape(-1, feats.shape[-1]), cols)
        rows = feats[:, torch.tensor(snr_axis, device=dev)].reshape(-1, feats.shape[-1]).contiguous()
        n_mods, per_mod = feats.shape[0], len(snr_axis) * feats.shape[2]
        y = np.repeat(np.asarray([int(sig.labels[i]) for i in range(n_mods)]), per_mod)
        train_idx, test_idx = stratified_split(y, t.test_size, t.random_state)
        widths = (len(cols), t.layer_size_hl1, t.layer_size_hl2, t.layer_size_hl3, n_mods)
        state = TrainState.init(widths, 0b111, optimizer, seeds)
        trainer = Trainer(rows, y, state, cols=cols, mean=mean, scale=scale, batch_size=t.batch_size, activation=t.activation, lr=lrs,
                          dropout=drops, seed=seeds, idx=train_idx)
        x_val, y_val = rows[torch.from_numpy(test_idx).to(dev)], y[test_idx]
        histories = [{"loss": [], "accuracy": [], "val_loss": [], "val_accuracy": []} for _ in range(n)]
        gen = torch.Generator(device="cpu").manual_seed(int(t.random_state))
        for epoch in range(t.epochs):
            loss, acc = trainer.run_epoch(torch.randperm(train_idx.size, generator=gen), steps_per_launch)
            trainer.download()
            for m in range(n):
                labels, probs = classify(x_val, state.model(m, t.activation), cols=cols, mean=mean, scale=scale, want=("labels", "probs"))
                p = probs.double().cpu().numpy()
                q = np.exp(p - p.max(axis=1, keepdims=True))
                q /= q.sum(axis=1, keepdims=True)                       # CrossEntropyLoss on the softmax output, as the reference
                val_loss = float(-np.log(q[np.arange(y_val.size), y_val]).mean())
                val_acc = float((labels.cpu().numpy() == y_val).mean())
                h = histories[m]
                for key, v in (("loss", loss[m]), ("accuracy", acc[m]), ("val_loss", val_loss), ("val_accuracy", val_acc)):
                    h[key].append(float(v))
                if verbose:
                    print((f"[model {m}] " if n > 1 else "") + f"Epoch {epoch + 1:3d}/{t.epochs} | loss: {h['loss'][-1]:.4f} | "
                          f"acc: {h['accuracy'][-1]:.4f} | val_loss: {val_loss:.4f} | val_acc: {val_acc:.4f}")
    return state, [str(uuid.uuid4()).split("-")[0] for _ in range(n)], histories


def run_training(cfg, *, device=None, sweep: Optional[dict] = None, verbose: bool = True) -> list:
    """The `train` command: :func:`train_model` on the feature files under the root, then per model ``ann/model-{id}.pt``
    (:func:`save_checkpoint`) and ``figures/{id}_history.mat``.  Returns the model ids."""
    import scipy.io
    lib = _lib.load()
    if lib.amcx_device_count() < 1:
        raise _lib.AmcxError(_lib.ENODEV, lib.amcx_strerror(_lib.ENODEV).decode())
    state, ids, histories = train_model(cfg, device=device, sweep=sweep, verbose=verbose)
    cfg.paths.ensure_dirs()
    for m, (model_id, h) in enumerate(zip(ids, histories)):
        settings = _settings(cfg)
        for key, name in (("lr", "learning_rate"), ("dropout", "dropout")):
            if sweep and key in sweep:
                settings[name] = float(sweep[key][m])
        path = save_checkpoint(cfg.paths.trained_ann / f"model-{model_id}.pt", state, m, model_id, {"training": settings})
        scipy.io.savemat(str(cfg.paths.figures / f"{model_id}_history.mat"), {k: np.asarray(v) for k, v in h.items()})
        if verbose:
            print(f"Model saved -> {path}")
    return ids
