"""What the float classifier (classifier.py) and the fixed-point network (quantize.py) share: a network as a packed block
(:class:`PackedMlp`), and of a call of one of the three network entries -- ``amcx_mlp_classify_f32``, ``amcx_mlp_range_f32``,
``amcx_mlp_classify_q15`` -- the rows it reads (:func:`row_plan`), the outputs it fills (:class:`OutputPlan`) and the accuracy
table made of its counts (:func:`accuracy_table`)."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np

MAX_WIDTH = 32          # every layer width, input and classes included (include/amcx.h)
MAX_LINEAR = 6


def check_widths(widths) -> tuple:
    widths = tuple(int(w) for w in widths)
    if not 1 <= len(widths) - 1 <= MAX_LINEAR:
        raise ValueError(f"between 1 and {MAX_LINEAR} dense layers, got {len(widths) - 1}")
    if any(not 1 <= w <= MAX_WIDTH for w in widths):
        raise ValueError(f"every layer width must be 1 ... {MAX_WIDTH}, got {widths}")
    return widths


def params_floats(widths) -> int:
    """Length of the packed block for these widths: sum of out * in + out."""
    widths = check_widths(widths)
    return sum(widths[l + 1] * widths[l] + widths[l + 1] for l in range(len(widths) - 1))


def layers(widths, block) -> list:
    """[(W (out, in), b (out,))] views of a packed block."""
    out, at = [], 0
    for l in range(len(widths) - 1):
        n_in, n_out = widths[l], widths[l + 1]
        out.append((block[at:at + n_out * n_in].reshape(n_out, n_in), block[at + n_out * n_in:at + n_out * n_in + n_out]))
        at += n_out * n_in + n_out
    return out


def i32s(v):
    return (ctypes.c_int32 * len(v))(*v)


def ptr(t):
    return None if t is None else t.data_ptr()


class PackedMlp:
    """A dense network as the library takes it: the layer widths and ``params``, the packed block of ``dtype`` (per layer
    ``W[out][in]`` row-major, then ``b[out]``).  One device copy of the block per device, made on first use."""

    def __init__(self, widths, params, dtype):
        self.widths = check_widths(widths)
        self.params = np.ascontiguousarray(params, dtype=dtype).reshape(-1)
        if self.params.size != params_floats(self.widths):
            raise ValueError(f"the packed block of widths {self.widths} has {params_floats(self.widths)} values, got {self.params.size}")
        self._device_params = {}

    n_linear = property(lambda self: len(self.widths) - 1)
    n_inputs = property(lambda self: self.widths[0])
    n_classes = property(lambda self: self.widths[-1])

    def device_params(self, device):
        import torch
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._device_params:
            self._device_params[key] = torch.from_numpy(self.params).to(device)
        return self._device_params[key]

    def entry_args(self, device) -> tuple:
        """``params_dev, widths_host, n_linear`` of a network entry."""
        return self.device_params(device).data_ptr(), i32s(self.widths), self.n_linear


def device_doubles(v, n: int, device, name: str):
    import torch
    if isinstance(v, torch.Tensor) and v.is_cuda:
        if v.dtype != torch.float64 or v.device != device:
            raise TypeError(f"{name} must be float64 on the rows' device")
        v = v.contiguous()
    else:
        v = torch.as_tensor(np.asarray(v, dtype=np.float64)).to(device)
    if v.shape != (n,):
        raise ValueError(f"{name} must hold one value per selected column ({n}), got shape {tuple(v.shape)}")
    return v


class RowPlan(NamedTuple):
    """What a network entry takes of its rows.  ``shape``: the caller's ``(..., rows, C)``; ``flat``: its ``(n_rows, C)`` view
    (a copy where no view has unit stride) at ``stride``; ``cols``: the selection as the entry's array; ``mean``, ``scale``:
    float64 on the rows' device, or both None."""
    shape: tuple
    flat: object
    n_rows: int
    stride: int
    cols: object
    mean: object
    scale: object

    device = property(lambda self: self.flat.device)

    def entry_args(self) -> tuple:
        """``x_dev, n_rows, row_stride, n_cols, cols_host, n_sel, mean_dev, scale_dev``: how every network entry begins."""
        return (self.flat.data_ptr(), self.n_rows, self.stride, self.shape[-1], self.cols, len(self.cols), ptr(self.mean),
                ptr(self.scale))


def row_plan(feats, n_inputs: int, cols, mean, scale) -> RowPlan:
    from . import _lib
    from .postprocess import _as_rows, select_cols
    _lib.require_torch_runtime()
    feats = _as_rows(feats)
    Cc = feats.shape[-1]
    cols = select_cols(cols, Cc)
    if len(cols) != n_inputs:
        raise ValueError(f"the model takes {n_inputs} inputs, {len(cols)} columns were selected")
    if (mean is None) != (scale is None):
        raise ValueError("mean and scale go together")
    flat = feats if feats.dim() == 2 else feats.reshape(-1, Cc)
    if flat.stride(-1) != 1:
        flat = flat.contiguous()
    if mean is not None:
        mean, scale = device_doubles(mean, len(cols), feats.device, "mean"), device_doubles(scale, len(cols), feats.device, "scale")
    n_rows = int(flat.shape[0])
    stride = flat.stride(0) if n_rows > 1 else Cc           # one row has no stride of its own (_stream.rows_of)
    return RowPlan(tuple(feats.shape), flat, n_rows, stride, i32s(cols), mean, scale)


class OutputPlan:
    """The outputs of a classifying entry that the caller named in ``want``, allocated in the shapes returned: ``labels`` int32
    ``(..., rows)``, ``names[1]`` (probabilities or logits, of ``per_class_dtype``) ``(..., rows, n_classes)``, ``counts`` int64
    ``(n_groups, n_classes + 1)``.  ``out``: the outputs by name, None where not asked for; the caller puts its further ones there
    before :meth:`result`.  ``entry_args``: ``labels_dev, probs_dev | logits_dev, its stride, rows_per_group, counts_dev``."""

    def __init__(self, want, names: tuple, rows: RowPlan, n_cls: int, rows_per_group: Optional[int], per_class_dtype):
        import torch
        self.want = want = tuple(want)
        if not want or any(w not in names for w in want) or len(set(want)) != len(want):
            raise ValueError(f"want: a non-empty selection of {names}")
        lead, R, dev = rows.shape[:-2], rows.shape[-2], rows.device
        counting = "counts" in want
        rows_per_group = int((R if counting else 0) if rows_per_group is None else rows_per_group)
        if counting and (rows_per_group < 1 or rows.n_rows % rows_per_group):
            raise ValueError(f"rows_per_group {rows_per_group} does not cut {rows.n_rows} rows into whole groups")
        labels = torch.empty(lead + (R,), dtype=torch.int32, device=dev) if "labels" in want else None
        per_class = torch.empty(lead + (R, n_cls), dtype=per_class_dtype, device=dev) if names[1] in want else None
        counts = torch.empty((rows.n_rows // rows_per_group, n_cls + 1), dtype=torch.int64, device=dev) if counting else None
        self.entry_args = (ptr(labels), ptr(per_class), n_cls, rows_per_group if counting else 0, ptr(counts))
        if counting and rows_per_group == R and len(rows.shape) > 2:      # counts over the rows axis: the leading dimensions'
            counts = counts.reshape(lead + (n_cls + 1,))
        self.out = {"labels": labels, names[1]: per_class, "counts": counts}

    def result(self):
        res = tuple(self.out[w] for w in self.want)
        return res[0] if len(res) == 1 else res


def accuracy_table(counts, labels, n_frames: int) -> tuple:
    """``(acc, confusion)`` of host counts ``(n_mods, n_snr, n_classes + 1)`` over groups of ``n_frames`` rows, ``labels[i]`` the
    class of modulation i: ``acc[i][snr]`` float64, the share labelled ``labels[i]``; ``confusion[true][predicted]`` int64
    ``(n_classes, n_classes + 1)`` summed over SNR and the modulations of a class, the last column the rows without a label."""
    n_mods, n_snr, bins = counts.shape
    acc = np.zeros((n_mods, n_snr), dtype=np.float64)
    confusion = np.zeros((bins - 1, bins), dtype=np.int64)
    for i, lab in enumerate(labels):
        acc[i] = counts[i, :, lab] / float(n_frames)
        confusion[lab] += counts[i].sum(axis=0)
    return acc, confusion
