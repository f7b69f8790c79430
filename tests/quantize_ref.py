"""Host restatements of the two fixed-point entries (include/amcx.h, ABI 16), which tests/test_gpu_quantize.py compares the
device with by ``==``:

* :func:`ranges32` -- ``amcx_mlp_range_f32``: the scaler's two float32 roundings, float32 sums in the order bias, k = 0, 1, ...
  with one rounding per step (``tests/psd_ref.fma32``, exact), relu or nothing between the layers, the rows with a non-finite
  value left out and counted;
* :func:`classify_q15` -- ``amcx_mlp_classify_q15`` in int64 numpy: every sum, shift, clamp and count.
"""
import numpy as np

from tests.psd_ref import fma32


def standardize32(rows, cols, mean=None, scale=None):
    """h = float(float(x - mean) / scale), the differences and quotients taken in float64 of float32 operands."""
    x = np.asarray(rows, dtype=np.float32)[:, list(cols)]
    if mean is None:
        return x
    with np.errstate(all="ignore"):
        c = (x.astype(np.float64) - np.asarray(mean, np.float64)).astype(np.float32)
        return (c.astype(np.float64) / np.asarray(scale, np.float64)).astype(np.float32)


def layers_of(widths, block):
    out, at = [], 0
    block = np.asarray(block).reshape(-1)
    for l in range(len(widths) - 1):
        n_in, n_out = widths[l], widths[l + 1]
        out.append((block[at:at + n_out * n_in].reshape(n_out, n_in), block[at + n_out * n_in:at + n_out * n_in + n_out]))
        at += n_out * n_in + n_out
    assert at == block.size
    return out


def forward32(h, widths, params, activation):
    """The pre-activation values of every layer, float32 (rows, out) each: bias first, then one FMA per k."""
    pre = []
    h = np.asarray(h, dtype=np.float32)
    with np.errstate(all="ignore"):
        for l, (w, b) in enumerate(layers_of(widths, np.asarray(params, np.float32))):
            acc = np.broadcast_to(b.astype(np.float32), (h.shape[0], w.shape[0])).copy()
            good = np.isfinite(h).all(axis=1)          # fma32 wants finite operands: the other rows are skipped anyway
            hh = np.where(good[:, None], h, np.float32(0))
            for k in range(w.shape[1]):
                acc = fma32(w[None, :, k], hh[:, k:k + 1], acc)
            acc[~good] = np.nan
            pre.append(acc)
            h = np.where(acc < 0, np.float32(0), acc) if activation == "relu" else acc
    return pre


def ranges32(rows, cols, mean, scale, widths, params, activation):
    """``(ranges float32 (n_linear + 1, 2), skipped)``."""
    h = standardize32(rows, cols, mean, scale)
    stages = [h] + forward32(h, widths, params, activation)
    ok = np.ones(h.shape[0], dtype=bool)
    for s in stages:
        ok &= np.isfinite(s).all(axis=1)
    out = np.empty((len(stages), 2), dtype=np.float32)
    for i, s in enumerate(stages):
        out[i] = (s[ok].min(), s[ok].max()) if ok.any() else (np.inf, -np.inf)
    return out, int((~ok).sum())


def classify_q15(rows, cols, mean, scale, widths, params16, frac_input, frac_weights, frac_biases, frac_outputs, rows_per_group=None):
    """``(labels int32, logits int16, counts int64 or None, saturated int64)`` of the integer network, in int64."""
    h = standardize32(rows, cols, mean, scale)
    n_rows, n_linear, n_cls = h.shape[0], len(widths) - 1, widths[-1]
    finite = np.isfinite(h).all(axis=1)
    saturated = np.zeros(n_linear + 1, dtype=np.int64)
    with np.errstate(all="ignore"):
        t = (h * np.float32(2.0 ** frac_input)).astype(np.float32)
    below, above = t < np.float32(-16384), t > np.float32(16383)
    c = np.where(below, np.float32(-16384), np.where(above, np.float32(16383), t))
    a = np.where(finite[:, None], np.rint(np.where(np.isfinite(c), c, 0)), 0).astype(np.int64)
    saturated[0] = int(((below | above) & finite[:, None]).sum())
    na = frac_input
    for l, (w, b) in enumerate(layers_of(widths, np.asarray(params16, np.int16))):
        nw, nb, no = frac_weights[l], frac_biases[l], frac_outputs[l]
        p = nw + na
        s = p - no
        assert p >= nb and s >= 1
        acc = a @ w.astype(np.int64).T + (b.astype(np.int64) << (p - nb))[None, :]
        v = (acc + (1 << (s - 1))) >> s
        over, under = v > 32767, v < -32768
        hidden = l + 1 < n_linear
        clips = over if hidden else over | under
        saturated[l + 1] = int((clips & finite[:, None]).sum())
        a = np.clip(v, -32768, 32767)
        if hidden:
            a = np.maximum(a, 0)
        na = no
    labels = np.where(finite, np.argmax(a, axis=1), -1).astype(np.int32)
    logits = np.where(finite[:, None], a, 0).astype(np.int16)
    counts = None
    if rows_per_group:
        bins = np.where(finite, labels, n_cls).reshape(-1, rows_per_group)
        counts = np.stack([np.bincount(g, minlength=n_cls + 1) for g in bins]).astype(np.int64)
    return labels, logits, counts, saturated
