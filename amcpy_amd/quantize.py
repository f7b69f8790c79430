"""Fixed-point deployment: the reference's ``quantize`` stage (nn_quantization.py) -- a trained network as 16-bit integers for
a microcontroller -- with the two device workloads it lacks: every layer's range calibrated over ALL rows of the data set
(``amcx_mlp_range_f32``), and the integer network itself run over every one of them (``amcx_mlp_classify_q15``), so that what
the 16-bit network answers, and where it saturates, is known before it is on the board.

* The reference's table: ``Qm.n`` with ``m + n = 15``, ``m = 0 ... 6``, range ``[-2^(m-1), 2^(m-1) - 2^-n]`` -- half of what
  16 bits hold, kept because it is the reference's rule and leaves a factor 2 of headroom.  :func:`find_q_format`,
  :func:`quantize_array` (host-side numpy, bit for bit the reference's clamp, scale and round).
* :class:`QuantizedMlp`: the widths, the packed int16 block in the float block's layout and the fractional bits of the input
  and of each layer's weights, biases and outputs.  Two layouts: ``"reference"`` -- the ``Linear`` layers as stored, no
  BatchNorm fold, output formats from ``(0, max)`` of the activation-free chain, the file ``arm-data/w_and_b.mat`` as the
  reference writes it -- and ``"folded"`` (default): ``MlpModel``'s folded block, output formats from the real forward pass.
* :func:`normalize_block` (the folded layout's default): the table ends at Q6.9, and a trained network's pre-activation values
  often pass +-32.  Relu is positively homogeneous, so a layer whose range no format holds is scaled by the power of two that
  brings it inside, and every later bias by the factors so far: every float32 value of the network is the same times an exact
  power of two, the labels are the same, and nothing clips.  Where every range fits, the block is the model's, untouched.
* :func:`calibrate`, :func:`classify_q15`, :func:`evaluate_by_snr_q15` on the device; :func:`run_quantization` is the
  ``quantize`` command.

The integer arithmetic is stated in include/amcx.h (ABI 16).  Nothing here computes a range or a label on the host: without
the library or a GPU the device functions raise.  Relu only: tanh and sigmoid in fixed point need lookup tables the reference
does not define.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._mlp import OutputPlan, PackedMlp, accuracy_table, check_widths, i32s, layers as _layers, ptr, row_plan
from .classifier import (MlpModel, by_snr_args, checkpoint_state_dict, classify, fit_scaler, fold_state_dict, linear_state_dict,
                         open_command, resolve_model_path)

# the reference's table, narrowest first: (integer bits m, fractional bits n)
Q_FORMATS = tuple((m, 15 - m) for m in range(7))
FALLBACK_FRAC = 9                # Q6.9, the widest, where no format holds the range


def q_range(n_frac: int) -> tuple:
    """``(lo, hi)`` of ``Qm.n`` with ``m = 15 - n``: ``[-2^(m-1), 2^(m-1) - 2^-n]``, the reference's ``_Q_RANGE``."""
    m = 15 - int(n_frac)
    return -(2.0 ** (m - 1)), 2.0 ** (m - 1) - 2.0 ** (-int(n_frac))


def q_name(n_frac: int) -> str:
    return f"Q{15 - int(n_frac)}.{int(n_frac)}"


def find_q_format(lo: float, hi: float) -> int:
    """The fractional bits of the narrowest format of the table that holds both ends; Q6.9's where none does."""
    lo, hi = float(lo), float(hi)
    for _, n in Q_FORMATS:
        flo, fhi = q_range(n)
        if lo >= flo and hi <= fhi:
            return n
    return FALLBACK_FRAC


def quantize_array(a, n_frac: int) -> np.ndarray:
    """float -> int16 in ``Qm.n``: clamp in float32 to the format's range, multiply by ``2^n``, round half to even.  Every
    value so made lies in ``[-16384, 16383]``."""
    lo, hi = q_range(n_frac)
    a = np.asarray(a, dtype=np.float32)
    clamped = np.minimum(np.maximum(a, np.float32(lo)), np.float32(hi))
    return np.rint(clamped * np.float32(2.0 ** int(n_frac))).astype(np.int16)


def normalize_block(widths, block32, ranges) -> tuple:
    """``(block, ranges, shifts)``: the packed float32 block with layer l scaled by ``2^-k_l``, ``k_l`` the smallest for which the
    layer's range -- ``(0, max)`` of a hidden layer, ``(min, max)`` of the last, times the factors of the layers before it -- lies
    inside Q6.9, and its bias by ``2^-shifts[l]``, ``shifts[l] = k_0 + ... + k_l``; the ranges scaled the same way.  Powers of two:
    every product is exact (short of underflow), so the scaled network's pre-activation values are the original's times
    ``2^-shifts[l]`` bit for bit and its labels are the original's.  All ``k_l`` are 0 where every range fits the table."""
    widths = check_widths(widths)
    n_linear = len(widths) - 1
    ranges = _check_ranges(ranges, n_linear).astype(np.float64)
    flo, fhi = q_range(FALLBACK_FRAC)
    out, shifts, cum = [], [], 0
    for l, (w, b) in enumerate(_layers(widths, np.asarray(block32, dtype=np.float32).reshape(-1))):
        lo = ranges[l + 1][0] if l + 1 == n_linear else 0.0
        hi = ranges[l + 1][1]
        k = 0
        while lo * 2.0 ** -(cum + k) < flo or hi * 2.0 ** -(cum + k) > fhi:
            k += 1
        cum += k
        shifts.append(cum)
        out += [(w * np.float32(2.0 ** -k)).reshape(-1), b * np.float32(2.0 ** -cum)]
        ranges[l + 1] *= 2.0 ** -cum
    return np.concatenate(out).astype(np.float32), ranges.astype(np.float32), tuple(shifts)


def linear_model(sd, model_id: Optional[str] = None) -> MlpModel:
    """The ``Linear`` layers of a state_dict as stored, every BatchNorm ignored, as a model :func:`calibrate` takes (with
    ``activation="none"``: the chain the reference's ``quantize`` takes its output ranges from)."""
    return MlpModel.from_state_dict(linear_state_dict(sd), "relu", model_id)


def _check_ranges(ranges, n_linear: int) -> np.ndarray:
    ranges = np.asarray(ranges, dtype=np.float32)
    if ranges.shape != (n_linear + 1, 2):
        raise ValueError(f"ranges: (min, max) of the input and of each of the {n_linear} layers, got shape {ranges.shape}")
    if not np.all(np.isfinite(ranges)):
        raise ValueError("ranges: not finite -- no row counted in the calibration")
    return ranges


class QuantizedMlp(PackedMlp):
    """A dense network as ``amcx_mlp_classify_q15`` takes it: ``params`` the packed int16 block (per layer ``W[out][in]``
    row-major, then ``b[out]``), ``frac_input`` and per layer ``frac_weights``, ``frac_biases``, ``frac_outputs``."""

    def __init__(self, widths, params, frac_input: int, frac_weights, frac_biases, frac_outputs, *, layout: str = "folded",
                 model_id: Optional[str] = None, ranges=None, layer_shifts=None):
        super().__init__(widths, params, np.int16)
        self.frac_input = int(frac_input)
        self.frac_weights, self.frac_biases, self.frac_outputs = (tuple(int(v) for v in f) for f in (frac_weights, frac_biases, frac_outputs))
        if any(len(f) != self.n_linear for f in (self.frac_weights, self.frac_biases, self.frac_outputs)):
            raise ValueError(f"one format per layer ({self.n_linear}) for the weights, the biases and the outputs")
        if any(not 0 <= v <= 15 for v in (self.frac_input, *self.frac_weights, *self.frac_biases, *self.frac_outputs)):
            raise ValueError("every fractional-bit count is 0 ... 15")
        na = self.frac_input
        for l in range(self.n_linear):
            p = self.frac_weights[l] + na
            if p < self.frac_biases[l] or p <= self.frac_outputs[l]:
                raise ValueError(f"layer {l + 1}: the product's {p} fractional bits must hold the bias's ({self.frac_biases[l]}) "
                                 f"and exceed the output's ({self.frac_outputs[l]})")
            na = self.frac_outputs[l]
        if layout not in ("reference", "folded"):
            raise ValueError("layout: reference or folded")
        self.layout, self.model_id = layout, model_id
        self.activation = "relu"
        self.ranges = None if ranges is None else np.asarray(ranges, dtype=np.float32)
        # layer l's values stand for the float network's times 2^-layer_shifts[l] (normalize_block); zeros: as they are
        self.layer_shifts = tuple(int(v) for v in layer_shifts) if layer_shifts is not None else (0,) * self.n_linear
        if len(self.layer_shifts) != self.n_linear:
            raise ValueError(f"one shift per layer ({self.n_linear})")

    # -- construction ---------------------------------------------------------------------------------------------------------
    @classmethod
    def _from_block(cls, widths, block32, ranges, layout, model_id, normalize=False) -> "QuantizedMlp":
        widths = check_widths(widths)
        n_linear = len(widths) - 1
        ranges = _check_ranges(ranges, n_linear)
        block32 = np.asarray(block32, dtype=np.float32).reshape(-1)
        shifts = None
        if normalize:
            block32, ranges, shifts = normalize_block(widths, block32, ranges)
        fw, fb, fo, parts = [], [], [], []
        for l, (w, b) in enumerate(_layers(widths, block32)):
            fw.append(find_q_format(w.min(), w.max()))
            fb.append(find_q_format(b.min(), b.max()))
            last = l + 1 == n_linear
            # a hidden layer's relu discards what lies below 0; the reference takes (0, max) for every layer
            lo = float(ranges[l + 1][0]) if last and layout == "folded" else 0.0
            fo.append(find_q_format(lo, float(ranges[l + 1][1])))
            parts += [quantize_array(w, fw[-1]).reshape(-1), quantize_array(b, fb[-1])]
        return cls(widths, np.concatenate(parts), find_q_format(ranges[0][0], ranges[0][1]), fw, fb, fo, layout=layout,
                   model_id=model_id, ranges=ranges, layer_shifts=shifts)

    @classmethod
    def from_model(cls, model: MlpModel, ranges, normalize: bool = True) -> "QuantizedMlp":
        """The folded layout of a float model: ``ranges`` as :func:`calibrate` gives them for it with its relu.  ``normalize``:
        :func:`normalize_block` first (nothing changes where every range fits the table); ``False`` exports the block as it
        is, and what lies beyond Q6.9 clips."""
        if model.activation != "relu":
            raise ValueError(f"fixed point is defined for relu alone, the model's activation is {model.activation!r}")
        return cls._from_block(model.widths, model.params, ranges, "folded", model.model_id, normalize)

    @classmethod
    def from_state_dict(cls, sd, ranges, layout: str = "folded", activation: str = "relu", model_id: Optional[str] = None,
                        normalize: bool = True) -> "QuantizedMlp":
        """``layout="folded"``: every BatchNorm folded (``MlpModel.from_state_dict``), ``ranges`` of that model with relu.
        ``layout="reference"``: the ``Linear`` layers as stored, ``ranges`` of :func:`linear_model` with ``activation="none"``."""
        if activation != "relu":
            raise ValueError(f"fixed point is defined for relu alone, got activation {activation!r}")
        if layout == "folded":
            return cls.from_model(MlpModel.from_state_dict(sd, activation, model_id), ranges, normalize)
        if layout != "reference":
            raise ValueError("layout: reference or folded")
        widths, p64 = fold_state_dict(linear_state_dict(sd))
        return cls._from_block(widths, p64.astype(np.float32), ranges, "reference", model_id)

    # -- export ---------------------------------------------------------------------------------------------------------------
    def layers(self) -> list:
        """[(W_q (out, in) int16, b_q (out,) int16)]."""
        return _layers(self.widths, self.params)

    def info(self) -> dict:
        """The reference's ``info`` dict: its keys, its strings."""
        info = {}
        for l in range(self.n_linear):
            info[f"Layer {l + 1} weights"] = q_name(self.frac_weights[l])
            info[f"Layer {l + 1} biases"] = q_name(self.frac_biases[l])
        info["Input"] = q_name(self.frac_input)
        for l in range(self.n_linear):
            info[f"Layer {l + 1} outputs"] = q_name(self.frac_outputs[l])
        return info

    def reference_export(self) -> tuple:
        """``({"weights": concat of W_q.T.flatten(), "biases": concat of b_q}, info)`` as the reference's ``quantize`` returns."""
        ws, bs = zip(*self.layers())
        return ({"weights": np.concatenate([w.T.flatten() for w in ws]), "biases": np.concatenate([b.flatten() for b in bs])},
                self.info())

    def save_reference_mat(self, path) -> None:
        """``arm-data/w_and_b.mat`` as the reference writes it."""
        import scipy.io
        scipy.io.savemat(str(path), self.reference_export()[0])

    def save_mat(self, path, mean=None, scale=None) -> None:
        """``arm-data/{model_id}_q15.mat``: the block in this package's order (per layer ``W[out][in]`` row-major) with every
        format, ``layer_shifts`` (layer l's values are the float network's times ``2^-layer_shifts[l]``: the argmax is the same)
        and the scaler's ``mean`` and ``scale``, which the board needs."""
        import scipy.io
        ws, bs = zip(*self.layers())
        out = {"weights": np.concatenate([w.reshape(-1) for w in ws]), "biases": np.concatenate(bs),
               "widths": np.asarray(self.widths, np.int32), "frac_weights": np.asarray(self.frac_weights, np.int32),
               "frac_biases": np.asarray(self.frac_biases, np.int32), "frac_outputs": np.asarray(self.frac_outputs, np.int32),
               "frac_input": np.int32(self.frac_input), "layer_shifts": np.asarray(self.layer_shifts, np.int32)}
        if mean is not None:
            out["mean"], out["scale"] = np.asarray(mean, np.float64), np.asarray(scale, np.float64)
        scipy.io.savemat(str(path), out)


# ---- the device ------------------------------------------------------------------------------------------------------------
_RANGE_ACTS = {"relu": _lib.ACT_RELU, "none": _lib.ACT_NONE}


def calibrate(feats, model: MlpModel, *, cols: Sequence[int], mean=None, scale=None, activation: str = "relu") -> tuple:
    """Every layer's range over all rows of ``feats`` (float32 CUDA ``(..., rows, C)``), one launch: ``(ranges, skipped)``,
    ``ranges`` float32 host ``(n_linear + 1, 2)`` -- (min, max) of the standardised input, then of every layer's pre-activation
    values, the float classifier's sums bit for bit -- and the number of rows a non-finite value kept out of them.
    ``activation``: ``"relu"`` between the layers, or ``"none"`` (the chain the reference calibrates on)."""
    import torch
    if activation not in _RANGE_ACTS:
        raise ValueError(f"activation {activation!r}: relu or none (tanh and sigmoid have no fixed-point form here)")
    rows = row_plan(feats, model.n_inputs, cols, mean, scale)
    if rows.n_rows < 1:
        raise ValueError("no rows to calibrate on")
    ranges = torch.empty((model.n_linear + 1, 2), dtype=torch.float32, device=rows.device)
    skipped = torch.empty((1,), dtype=torch.int64, device=rows.device)
    from . import _stream
    _stream.launch(rows.flat, lambda lib, stream: lib.amcx_mlp_range_f32(
        *rows.entry_args(), *model.entry_args(rows.device), _RANGE_ACTS[activation], ranges.data_ptr(), skipped.data_ptr(), stream))
    return ranges.cpu().numpy(), int(skipped.item())


_OUTPUTS = ("labels", "logits", "counts", "saturated")


def classify_q15(feats, qmodel: QuantizedMlp, *, cols: Sequence[int], mean=None, scale=None, rows_per_group: Optional[int] = None,
                 want: Sequence[str] = ("labels", "logits", "counts", "saturated")):
    """The integer network over ``feats`` (float32 CUDA ``(..., rows, C)``), one C-ABI call on the current stream.  Returns
    the outputs named in ``want`` in that order (the tensor itself when one is asked for): ``"labels"`` int32 ``(..., rows)``,
    -1 for a row with a non-finite input; ``"logits"`` int16 ``(..., rows, n_classes)``; ``"counts"`` int64 as
    :func:`amcpy_amd.classifier.classify` gives them; ``"saturated"`` int64 ``(n_linear + 1,)``."""
    import torch
    from . import _stream
    if qmodel.activation != "relu":
        raise ValueError(f"fixed point is defined for relu alone, got activation {qmodel.activation!r}")
    rows = row_plan(feats, qmodel.n_inputs, cols, mean, scale)
    out = OutputPlan(want, _OUTPUTS, rows, qmodel.n_classes, rows_per_group, torch.int16)
    saturated = torch.empty((qmodel.n_linear + 1,), dtype=torch.int64, device=rows.device) if "saturated" in out.want else None
    out.out["saturated"] = saturated
    fw, fb, fo = i32s(qmodel.frac_weights), i32s(qmodel.frac_biases), i32s(qmodel.frac_outputs)
    _stream.launch(rows.flat, lambda lib, stream: lib.amcx_mlp_classify_q15(
        *rows.entry_args(), *qmodel.entry_args(rows.device), _lib.ACT_RELU, qmodel.frac_input, fw, fb, fo, *out.entry_args,
        ptr(saturated), stream))
    return out.result()


def evaluate_by_snr_q15(feats_by_mod, qmodel: QuantizedMlp, *, cols: Sequence[int], mean, scale, labels: Sequence[int]):
    """:func:`amcpy_amd.classifier.evaluate_by_snr` for the integer network: ``(acc, confusion, saturated)``."""
    feats_by_mod, labels, n_frames = by_snr_args(feats_by_mod, qmodel.n_classes, labels)
    counts, saturated = classify_q15(feats_by_mod, qmodel, cols=cols, mean=mean, scale=scale, want=("counts", "saturated"))
    return (*accuracy_table(counts.cpu().numpy(), labels, n_frames), saturated.cpu().numpy())


# ---- the `quantize` command --------------------------------------------------------------------------------------------------
def run_quantization(cfg, model_spec: str, *, mode: str = "test", layout: str = "folded", evaluate: bool = False,
                     device: Optional[int] = None, verbose: bool = True, normalize: bool = True):
    """The `quantize` command.  The scaler is :func:`amcpy_amd.classifier.fit_scaler` ``(cfg, mode, dev)``; the ranges are
    calibrated on every row of the feature files (what the reference's ``preprocess_data(cfg, "test")`` stacks: all SNRs, train
    and test rows together); the export goes to ``arm-data/`` -- ``w_and_b.mat`` (``layout="reference"``) or
    ``{model_id}_q15.mat``, its layers scaled by powers of two where a range passes the table (``normalize``,
    :func:`normalize_block`) -- and the formats are printed.  ``evaluate`` (folded layout): the integer network over every row,
    the float classifier beside it, into ``figures/{model_id}_q15_figure_data.mat`` (``acc``, ``acc_float``, ``agreement``:
    the share of rows with the same label per modulation and SNR, ``saturated``).  Returns the :class:`QuantizedMlp`, with
    the evaluation as a dict behind it when asked for."""
    if layout not in ("reference", "folded"):
        raise ValueError("layout: reference or folded")
    if evaluate and layout != "folded":
        raise ValueError("--evaluate runs the trained network: the folded layout (the reference layout ignores every BatchNorm)")
    import scipy.io
    import torch
    model, model_id, cols, dev = open_command(cfg, model_spec, mode, device)
    if model.activation != "relu":
        raise ValueError(f"fixed point is defined for relu alone, the model's activation is {model.activation!r}")
    feats, mean, scale = fit_scaler(cfg, mode, dev)
    sig = cfg.signals
    n_mods, n_snr, n_frames, _ = feats.shape
    cfg.paths.ensure_dirs()
    cfg.paths.arm_data.mkdir(parents=True, exist_ok=True)
    with torch.cuda.device(dev):
        if layout == "reference":
            path = resolve_model_path(cfg, model_spec)
            if path.suffix == ".npz":
                raise ValueError("the reference layout needs the checkpoint's state_dict (a .pt file): a .npz model is folded already")
            sd, _ = checkpoint_state_dict(path)
            ranges, skipped = calibrate(feats, linear_model(sd), cols=cols, mean=mean, scale=scale, activation="none")
            q = QuantizedMlp.from_state_dict(sd, ranges, layout="reference", model_id=model_id)
            out_path = cfg.paths.arm_data / "w_and_b.mat"
            q.save_reference_mat(out_path)
        else:
            ranges, skipped = calibrate(feats, model, cols=cols, mean=mean, scale=scale, activation="relu")
            q = QuantizedMlp.from_model(model, ranges, normalize)
            q.model_id = model_id
            out_path = cfg.paths.arm_data / f"{model_id}_q15.mat"
            q.save_mat(out_path, mean.cpu().numpy(), scale.cpu().numpy())
        if verbose:
            print(f"model {model_id}: widths {q.widths}, layout {layout}; calibrated on {n_mods * n_snr * n_frames} rows "
                  f"({skipped} skipped as non-finite) -> {out_path}")
            for key, val in q.info().items():
                print(f"  {key}: {val}")
            if any(q.layer_shifts):
                print(f"  layers scaled by 2^-k to fit the table, k per layer (cumulative): {list(q.layer_shifts)}")
        if not evaluate:
            return q
        lab_q, counts_q, saturated = classify_q15(feats, q, cols=cols, mean=mean, scale=scale, want=("labels", "counts", "saturated"))
        lab_f, counts_f = classify(feats, model, cols=cols, mean=mean, scale=scale, want=("labels", "counts"))
        agreement = (lab_q == lab_f).to(torch.float64).mean(dim=-1).cpu().numpy()
        counts_q, counts_f, saturated = counts_q.cpu().numpy(), counts_f.cpu().numpy(), saturated.cpu().numpy()
    labels = [int(sig.labels[i]) for i in range(n_mods)]
    acc, acc_float = accuracy_table(counts_q, labels, n_frames)[0], accuracy_table(counts_f, labels, n_frames)[0]
    result = {"acc": acc, "acc_float": acc_float, "agreement": agreement, "saturated": saturated}
    scipy.io.savemat(str(cfg.paths.figures / f"{model_id}_q15_figure_data.mat"), result)
    if verbose:
        print(f"Q15 against float: mean accuracy {acc.mean():.4f} / {acc_float.mean():.4f}, the same label on "
              f"{agreement.mean():.4%} of the rows; saturated (input, then each layer): {saturated.tolist()}")
    return q, result
