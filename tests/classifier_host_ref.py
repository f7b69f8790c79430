"""Float64 numpy forward over a packed parameter block (include/amcx.h: per layer W'[out][in] row-major, then
b'[out]) -- the CHECKER of the classifier tests and of tests/golden/make_classifier_fixtures.py.  It lives under
tests/ on purpose: the product (amcpy_amd/) computes labels on the GPU only."""
import numpy as np

ACTS = {"relu": lambda v: np.where(v < 0, 0.0, v), "tanh": np.tanh, "sigmoid": lambda v: 1.0 / (1.0 + np.exp(-v))}


def forward64(x, widths, params, activation):
    """x: (rows, widths[0]) -> probabilities (rows, widths[-1]) float64."""
    h = np.asarray(x, dtype=np.float64)
    p = np.asarray(params, dtype=np.float64).reshape(-1)
    pos, n_linear = 0, len(widths) - 1
    for l in range(n_linear):
        n_in, n_out = int(widths[l]), int(widths[l + 1])
        w = p[pos:pos + n_out * n_in].reshape(n_out, n_in)
        b = p[pos + n_out * n_in:pos + n_out * n_in + n_out]
        pos += n_out * n_in + n_out
        h = h @ w.T + b
        if l + 1 < n_linear:
            h = ACTS[activation](h)
    assert pos == p.size
    e = np.exp(h - h.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def standardize64(rows, cols, mean, scale):
    return (np.asarray(rows, dtype=np.float64)[:, list(cols)] - np.asarray(mean)) / np.asarray(scale)


def top_two_margin(p):
    s = np.sort(p, axis=1)
    return s[:, -1] - s[:, -2]


def state_dict_of(z, prefix="sd:"):
    """The state_dict arrays a fixture stores under '<prefix><key>'."""
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}
