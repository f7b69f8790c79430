"""Classification on the device: what comes after ``features18`` / ``select_standardize`` in the reference --
its ``AMCClassifier`` in eval() mode (nn_model.py:28-75), the ``model(x_t).argmax(1)`` of ``evaluate_by_snr``
(nn_model.py:227-267) and the accuracy count per modulation and SNR -- as ONE HIP launch per call over the
device-resident feature matrix (amcpy_amd/csrc/amcx_mlp_kernel.h behind ``amcx_mlp_classify_f32``).

* :class:`MlpModel` holds a network as the library takes it: layer widths, the activation and the packed float32
  parameter block with every BatchNorm folded into the Linear before it.  It is built from a ``state_dict`` of the
  reference's layout, from the checkpoint file the reference's ``train_model`` writes (read WITHOUT the reference
  installed and without running any pickled global, :func:`load_checkpoint`), or from plain arrays (``.npz``).
* :func:`classify` -- rows in, labels / probabilities / per-group counts out.
* :func:`classify_frames` -- IQ frames in: ``features18`` on the needed feature ids, then :func:`classify`.
* :func:`evaluate_by_snr` -- the reference's accuracy table, plus the confusion matrix.

NaN rule (a deliberate difference from the reference): a row whose probabilities are not all finite gets label -1
and is counted in an extra last bin; the reference's argmax answers class 0 for it.

Nothing here computes a label on the host: without the library or a GPU these functions raise.
"""
from __future__ import annotations

import io
import pickle
import re
import types
import zipfile
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._mlp import MAX_LINEAR, MAX_WIDTH, OutputPlan, PackedMlp, accuracy_table, check_widths, params_floats, row_plan  # noqa: F401

BN_EPS = 1e-5           # torch.nn.BatchNorm1d's default, the reference's

_KEY = re.compile(r"^(?:.*\.)?(\d+)\.(weight|bias|running_mean|running_var|num_batches_tracked)$")


def _array(v) -> np.ndarray:
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.asarray(v, dtype=np.float64)


def fold_state_dict(sd) -> tuple:
    """(widths, float64 packed block) of a ``state_dict`` in the reference's layout: numbered entries of one
    Sequential (``layers.0.weight`` ...), a 2-D ``weight`` being a Linear and an entry with ``running_mean`` the
    BatchNorm1d that follows the Linear numbered just before it.  Any number of Linear(+BatchNorm) blocks within the
    limits, BatchNorm optional per block.  The fold, in float64:
    ``g = gamma / sqrt(var + eps); W' = W * g[:, None]; b' = (b - mean) * g + beta``."""
    entries = {}
    for key, val in sd.items():
        m = _KEY.match(str(key))
        if m is None:
            raise ValueError(f"state_dict key {key!r}: expected '<prefix>.<index>.<weight|bias|running_mean|running_var>'")
        if m.group(2) != "num_batches_tracked":
            entries.setdefault(int(m.group(1)), {})[m.group(2)] = _array(val)
    linear = sorted(i for i, e in entries.items() if "weight" in e and e["weight"].ndim == 2)
    norms = sorted(i for i, e in entries.items() if "running_mean" in e)
    if not linear or sorted(linear + norms) != sorted(entries):
        raise ValueError("state_dict: every numbered entry must be a Linear (2-D weight) or a BatchNorm1d (running_mean)")
    widths, blocks = [entries[linear[0]]["weight"].shape[1]], []
    for n, i in enumerate(linear):
        w = entries[i]["weight"]
        b = entries[i].get("bias", np.zeros(w.shape[0]))
        if w.shape[1] != widths[-1] or b.shape != (w.shape[0],):
            raise ValueError(f"state_dict: Linear {i} of shape {w.shape} does not follow a layer of width {widths[-1]}")
        nxt = linear[n + 1] if n + 1 < len(linear) else None
        mine = [j for j in norms if j > i and (nxt is None or j < nxt)]
        if len(mine) > 1:
            raise ValueError(f"state_dict: more than one BatchNorm behind Linear {i}")
        if mine:
            bn = entries[mine[0]]
            var, mu = bn["running_var"], bn["running_mean"]
            gamma, beta = bn.get("weight", np.ones_like(var)), bn.get("bias", np.zeros_like(var))
            if not (var.shape == mu.shape == gamma.shape == beta.shape == (w.shape[0],)):
                raise ValueError(f"state_dict: BatchNorm {mine[0]} does not match the {w.shape[0]} outputs of Linear {i}")
            g = gamma / np.sqrt(var + BN_EPS)
            w, b = w * g[:, None], (b - mu) * g + beta
        widths.append(w.shape[0])
        blocks += [w.reshape(-1), b]
    if any(j < linear[0] for j in norms):
        raise ValueError("state_dict: a BatchNorm before the first Linear")
    return check_widths(widths), np.concatenate(blocks)


def linear_state_dict(sd) -> dict:
    """The ``Linear`` entries of a state_dict alone (2-D ``weight`` and its ``bias``): the chain the reference quantises."""
    keep = {}
    for key, val in sd.items():
        m = _KEY.match(str(key))
        if m is not None and m.group(2) == "weight" and _array(val).ndim == 2:
            keep[str(key)] = val
            bias = str(key)[:-len("weight")] + "bias"
            if bias in sd:
                keep[bias] = sd[bias]
    return keep


class MlpModel(PackedMlp):
    """A dense network as ``amcx_mlp_classify_f32`` takes it.  ``params``: the packed float32 block (per layer
    ``W'[out][in]`` row-major, then ``b'[out]``); ``params64``: the same before its single rounding, when the model
    came from a state_dict (None otherwise).  One device copy of the block per device, made on first use."""

    def __init__(self, widths, activation: str, params, params64=None, model_id: Optional[str] = None):
        super().__init__(widths, params, np.float32)
        if activation not in _lib.ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: one of {sorted(_lib.ACTIVATIONS)}")
        self.activation = activation
        self.params64 = None if params64 is None else np.asarray(params64, dtype=np.float64).reshape(-1)
        self.model_id = model_id

    @classmethod
    def from_state_dict(cls, sd, activation: str = "relu", model_id: Optional[str] = None) -> "MlpModel":
        widths, p64 = fold_state_dict(sd)
        return cls(widths, activation, p64.astype(np.float32), p64, model_id)

    @classmethod
    def from_checkpoint(cls, path, activation: Optional[str] = None, default_activation: str = "relu") -> "MlpModel":
        """The file the reference's ``train_model`` writes (``{"model_state_dict", "model_id", "config"}``), read by
        :func:`load_checkpoint`.  The activation comes from the stored config's ``training.activation`` when it is
        there (the argument wins when both are given), ``default_activation`` otherwise.  The config may also be a plain dict,
        as :func:`amcpy_amd.train.save_checkpoint` writes it: ``{"training": {"activation": ...}}`` or the training settings
        themselves."""
        sd, ck = checkpoint_state_dict(path)
        config = ck.get("config") if isinstance(ck, dict) else None
        if isinstance(config, dict):
            training = config.get("training", config)
            stored = training.get("activation") if isinstance(training, dict) else getattr(training, "activation", None)
        else:
            stored = getattr(getattr(config, "training", None), "activation", None)
        act = activation or (stored if isinstance(stored, str) else None) or default_activation
        model_id = ck.get("model_id") if isinstance(ck, dict) else None
        return cls.from_state_dict(sd, act, model_id if isinstance(model_id, str) else None)

    @classmethod
    def from_npz(cls, path) -> "MlpModel":
        with np.load(str(path), allow_pickle=False) as z:
            mid = str(z["model_id"]) if "model_id" in z.files else None
            return cls(z["widths"], str(z["activation"]), z["params"], z["params64"] if "params64" in z.files else None,
                       mid or None)

    def save_npz(self, path) -> None:
        extra = {} if self.params64 is None else {"params64": self.params64}
        np.savez(str(path), widths=np.asarray(self.widths, np.int32), activation=np.asarray(self.activation),
                 params=self.params, model_id=np.asarray(self.model_id or ""), **extra)


# ---- the checkpoint, read without running what it names ------------------------------------------------------------
class _Inert:
    """Stands in for every global a checkpoint names that is not needed to rebuild a tensor: constructing, calling,
    filling or setting the state of one does nothing but keep the plain attributes."""

    def __new__(cls, *a, **k):
        return object.__new__(cls)

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Inert()

    def __setstate__(self, state):
        if isinstance(state, tuple) and len(state) == 2:          # (dict state, slots state)
            state = {**(state[0] or {}), **(state[1] or {})}
        if isinstance(state, dict):
            self.__dict__.update({k: v for k, v in state.items() if isinstance(k, str)})

    def append(self, item):
        pass

    def extend(self, items):
        pass

    def __setitem__(self, key, value):
        pass


_ALLOWED = {("collections", "OrderedDict"), ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_tensor"),
            ("torch._utils", "_rebuild_parameter"), ("torch", "Size"), ("torch", "device"),
            ("torch.serialization", "_get_layout"), ("torch._tensor", "_rebuild_from_type_v2"), ("torch", "Tensor"),
            ("torch.nn.parameter", "Parameter")}


class _RestrictedUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        import torch
        if (module, name) in _ALLOWED:
            return super().find_class(module, name)
        if module == "torch" and isinstance(getattr(torch, name, None), torch.dtype):
            return getattr(torch, name)
        return type(name, (_Inert,), {"__module__": "amcpy_amd.classifier", "_stands_for": f"{module}.{name}"})


def load_checkpoint(path):
    """The object a ``torch.save`` file holds, with tensors as tensors and EVERY other pickled global -- the
    reference's config dataclasses, paths, anything a hostile file names -- replaced by an inert stand-in that keeps
    plain attributes (so ``ck["config"].training.activation`` reads) and runs nothing.  ``torch.load`` cannot do this:
    ``weights_only=True`` refuses the config object, ``weights_only=False`` imports and calls whatever the file
    names (and needs the reference's package importable)."""
    import torch
    path = Path(path)
    if not zipfile.is_zipfile(path):
        raise ValueError(f"{path}: not a torch.save archive (the zip format torch has written since 1.6)")
    module = types.ModuleType("amcpy_amd_restricted_pickle")
    module.Unpickler = _RestrictedUnpickler
    module.load = lambda f, **kw: _RestrictedUnpickler(f, **kw).load()
    module.loads = lambda b, **kw: _RestrictedUnpickler(io.BytesIO(b), **kw).load()
    return torch.load(str(path), map_location="cpu", weights_only=False, pickle_module=module)


def checkpoint_state_dict(path) -> tuple:
    """``(state_dict, checkpoint)`` of a file :func:`load_checkpoint` reads: the reference's ``{"model_state_dict", ...}`` or a
    bare state_dict."""
    ck = load_checkpoint(path)
    return (ck["model_state_dict"] if isinstance(ck, dict) and "model_state_dict" in ck else ck), ck


# ---- classification --------------------------------------------------------------------------------------------------
_OUTPUTS = ("labels", "probs", "counts")


def classify(feats, model: MlpModel, *, cols: Sequence[int], mean=None, scale=None, rows_per_group: Optional[int] = None,
             want: Sequence[str] = ("labels",)):
    """feats: float32 CUDA tensor ``(..., rows, C)``.  Picks ``cols`` (0-based, as ``select_standardize``), applies
    ``(x - mean) / scale`` with the scaler's two float32 roundings (``mean`` / ``scale``: float64, device tensors -- as
    ``select_standardize`` returns them -- or host arrays; both None: the rows are standardised already), runs the
    network, and returns the outputs named in ``want`` in that order (the tensor itself when one is asked for):

    * ``"labels"``: int32 ``(..., rows)``, -1 where the probabilities are not all finite;
    * ``"probs"``: float32 ``(..., rows, n_classes)``;
    * ``"counts"``: int64 ``(n_groups, n_classes + 1)`` over consecutive groups of ``rows_per_group`` rows of the
      flattened matrix (default: the ``rows`` axis, giving ``(..., n_classes + 1)``), last bin = label -1.

    One C-ABI call on the current stream; nothing is allocated inside it."""
    import torch
    from . import _stream
    rows = row_plan(feats, model.n_inputs, cols, mean, scale)
    out = OutputPlan(want, _OUTPUTS, rows, model.n_classes, rows_per_group, torch.float32)
    _stream.launch(rows.flat, lambda lib, stream: lib.amcx_mlp_classify_f32(
        *rows.entry_args(), *model.entry_args(rows.device), _lib.ACTIVATIONS[model.activation], *out.entry_args, stream))
    return out.result()


def classify_frames(iq, model: MlpModel, *, cols: Sequence[int], mean, scale, frame_size: Optional[int] = None,
                    variant="auto", rows_per_group: Optional[int] = None, want: Sequence[str] = ("labels",)):
    """iq: complex64 CUDA tensor ``(..., n_frames, L)``.  ``features18`` restricted to the feature ids the columns
    stand for (``c + 1``: the cheapest plan kernel that yields them, none of the reference's six needs the FFT), then
    :func:`classify`, both on the current stream; the feature matrix never leaves the device."""
    from .features import features18
    from .postprocess import select_cols
    cols = select_cols(cols, _lib.NUM_FEATURES)
    feats = features18(iq, frame_size=frame_size, variant=variant, feature_ids=[c + 1 for c in cols])
    if feats.dim() == 1:
        feats = feats.reshape(1, -1)
    return classify(feats, model, cols=cols, mean=mean, scale=scale, rows_per_group=rows_per_group, want=want)


def evaluate_by_snr(feats_by_mod, model: MlpModel, *, cols: Sequence[int], mean, scale, labels: Sequence[int]):
    """The reference's ``nn_model.evaluate_by_snr`` table.  feats_by_mod: ``(n_mods, n_snr, n_frames, C)`` float32 on
    the GPU (or a sequence of ``(n_snr, n_frames, C)`` tensors); ``labels[i]``: the class of modulation i.  Returns
    ``(acc, confusion)``: ``acc[i][snr]`` float64, the share of frames of modulation i at that SNR labelled
    ``labels[i]``; ``confusion[true][predicted]`` int64 ``(n_classes, n_classes + 1)`` summed over SNR, the extra
    column counting the rows without a label.  (The reference indexes ``mod_data[snr, :, list(used)]``, which is
    ``(6, n_frames)`` and raises in its scaler; the evident intention, ``(n_frames, 6)``, is what is taken here, as
    ``select_standardize`` does.)  One launch, one group per (modulation, SNR)."""
    feats_by_mod, labels, n_frames = by_snr_args(feats_by_mod, model.n_classes, labels)
    counts = classify(feats_by_mod, model, cols=cols, mean=mean, scale=scale, want=("counts",)).cpu().numpy()
    return accuracy_table(counts, labels, n_frames)


def by_snr_args(feats_by_mod, n_classes: int, labels) -> tuple:
    """What :func:`evaluate_by_snr` and ``quantize.evaluate_by_snr_q15`` ask of their arguments: ``(feats_by_mod as one tensor,
    labels as ints, n_frames)``."""
    import torch
    if not isinstance(feats_by_mod, torch.Tensor):
        feats_by_mod = torch.stack(list(feats_by_mod))
    if feats_by_mod.dim() != 4:
        raise ValueError("feats_by_mod must be (n_mods, n_snr, n_frames, C)")
    n_mods, _, n_frames, _ = feats_by_mod.shape
    labels = [int(v) for v in labels]
    if len(labels) != n_mods or any(not 0 <= v < n_classes for v in labels):
        raise ValueError(f"labels: one class 0 ... {n_classes - 1} per modulation ({n_mods})")
    if n_frames < 1:
        raise ValueError("no frames to evaluate")
    return feats_by_mod, labels, n_frames


# ---- the `classify` command --------------------------------------------------------------------------------------------
def resolve_model_path(cfg, spec: str) -> Path:
    """``--model``: a path to a ``.pt`` / ``.npz`` file, or the id of ``ann/model-{id}.pt`` under the root."""
    p = Path(spec)
    if p.suffix in (".pt", ".npz") or p.exists():
        return p
    return cfg.paths.trained_ann / f"model-{spec}.pt"


def load_model(cfg, model_spec: str) -> tuple:
    """``--model`` -> ``(MlpModel, model id)``: :func:`resolve_model_path`, a ``.npz`` model or a ``.pt`` checkpoint."""
    path = resolve_model_path(cfg, model_spec)
    if not path.exists():
        raise FileNotFoundError(f"no model at {path}")
    model = (MlpModel.from_npz(path) if path.suffix == ".npz"
             else MlpModel.from_checkpoint(path, default_activation=cfg.training.activation))
    return model, model.model_id or (model_spec if path.name == f"model-{model_spec}.pt" else path.stem)


def fit_scaler(cfg, mode: str, dev) -> tuple:
    """The scaler of the `classify` command, which the `recording` command's ``--model`` fits the same way: the feature files
    ``calculated-features/{mod}_features.mat`` of every modulation onto ``dev``, :func:`amcpy_amd.postprocess.select_standardize`
    over the rows the reference's ``preprocess_data(cfg, mode)`` stacks (``training_snr`` or ``all_snr``).  Returns ``(feats
    (n_mods, n_snr, n_frames, 18) on dev, mean, scale)``; the columns are ``cfg.features.used``."""
    if mode not in ("training", "test"):
        raise ValueError("mode: training or test")
    import scipy.io
    import torch
    from .postprocess import select_standardize
    sig, cols = cfg.signals, [int(c) for c in cfg.features.used]
    host = []
    for mod in sig.modulations_with_noise:
        data = scipy.io.loadmat(str(cfg.paths.calculated_features / f"{mod}_features.mat"))
        host.append(np.asarray(data[sig.mat_info[mod]], dtype=np.float32))
    feats = torch.from_numpy(np.ascontiguousarray(np.stack(host))).to(dev)  # (n_mods, n_snr, n_frames, 18); loadmat's are Fortran-ordered
    snr_axis = list(cfg.training.training_snr if mode == "training" else cfg.training.all_snr)
    with torch.cuda.device(dev):
        fit_rows = feats[:, torch.tensor(snr_axis, device=dev)].reshape(-1, feats.shape[-1])
        _, mean, scale = select_standardize(fit_rows, cols)
    return feats, mean, scale


def open_command(cfg, model_spec: str, mode: str, device: Optional[int]) -> tuple:
    """How the `classify` and `quantize` commands begin, before any feature file is read: the mode, the library and a device
    present, the model, the columns ``cfg.features.used`` and the device :func:`fit_scaler` is to run on.  Returns ``(model,
    model id, cols, dev)``."""
    if mode not in ("training", "test"):
        raise ValueError("mode: training or test")
    lib = _lib.load()
    if lib.amcx_device_count() < 1:
        raise _lib.AmcxError(_lib.ENODEV, lib.amcx_strerror(_lib.ENODEV).decode())
    import torch
    model, model_id = load_model(cfg, model_spec)
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    return model, model_id, [int(c) for c in cfg.features.used], dev


def run_classification(cfg, model_spec: str, *, mode: str = "test", from_iq: bool = False, device: Optional[int] = None,
                       verbose: bool = True):
    """The `classify` command: features from ``calculated-features/{mod}_features.mat`` (``from_iq``: extracted first,
    the used features only), the scaler fitted on the device over the rows the reference's ``preprocess_data(cfg, mode)``
    stacks (``training_snr`` or ``all_snr``, every modulation), every (modulation, SNR, frame) classified; writes
    ``figures/{model_id}_figure_data.mat`` (key ``acc``, the reference's file) and ``{mod}_predictions.mat`` beside the
    feature files.  Returns ``(acc, confusion)``."""
    import scipy.io
    import torch
    model, model_id, cols, dev = open_command(cfg, model_spec, mode, device)
    if from_iq:
        from .feature_extraction import run_extraction
        run_extraction(cfg, device=device, verbose=verbose, feature_ids=sorted({c + 1 for c in cols}))
    feats, mean, scale = fit_scaler(cfg, mode, dev)
    sig, mods, n_snr = cfg.signals, list(cfg.signals.modulations_with_noise), feats.shape[1]
    with torch.cuda.device(dev):
        labels, counts = classify(feats, model, cols=cols, mean=mean, scale=scale, want=("labels", "counts"))
        labels, counts = labels.cpu().numpy(), counts.cpu().numpy()
    acc, confusion = accuracy_table(counts, [int(sig.labels[i]) for i in range(len(mods))], feats.shape[2])
    cfg.paths.ensure_dirs()
    scipy.io.savemat(str(cfg.paths.figures / f"{model_id}_figure_data.mat"), {"acc": acc})
    for i, mod in enumerate(mods):
        scipy.io.savemat(str(cfg.paths.calculated_features / f"{mod}_predictions.mat"),
                         {"Modulation": mod, "predictions": labels[i].astype(np.int32)})
    if verbose:
        print(f"model {model_id}: widths {model.widths}, {model.activation}; accuracy per modulation (rows) and SNR (columns)")
        print(" " * 8 + " ".join(f"{sig.snr_values.get(s, s):>5}" for s in range(n_snr)))
        for i, mod in enumerate(mods):
            print(f"{mod:>7} " + " ".join(f"{a:5.3f}" for a in acc[i]))
        print(f"rows without a label (non-finite probabilities): {int(confusion[:, -1].sum())}")
    return acc, confusion

