"""Shape sweeps of the three kernels behind the feature matrix -- the classifier (amcx_mlp_kernel.h), the chunked
statistics and the scaler (amcx_post_kernels.h): case tables, seeded inputs, checkers and comparisons.  numpy only;
nothing here touches the GPU.  tests/test_post_shapes_host.py shows on the CPU that the cases have the power claimed for
them, tests/test_gpu_post_shapes.py runs them through the kernels.

Classifier.  Width tuples run ``inputs, hidden..., classes``.  One position at a time takes every width around a block
of 8 (``EDGE``), a chain changes its number of blocks from layer to layer at depth 1 to 6, and the corners hold the extremes.
Every case has its own parameters (``make_params``: scaled so that no unit saturates or dies and no class wins alone;
``sensitivity`` measures that every single element of the packed block matters) and its own 1100 rows (``make_feed``:
two tiles of 512 and a ragged third whose last wave holds 12 rows), fed through a 32-column matrix by a column
selection that leaves no column in its own place, NaN in every column that is not selected.

Statistics.  ``stat_row_counts(n_cols)`` are the row counts that hit every cut of the kernel for that column count: a
partial tile, a tile, a tile and a row, a ragged third tile, and a count at which a 3-group call gives every workgroup
two tiles and the last one a ragged single one.

Scaler.  ``two_roundings`` is the contract, float(float(x - mean) / scale) in IEEE double, checked bit for bit.
"""
import numpy as np

from tests import classifier_host_ref as href

ACTS = ("relu", "tanh", "sigmoid")

# ---------------------------------------------------------------------------------------------------------------------
# classifier: cases
# ---------------------------------------------------------------------------------------------------------------------
EDGE = (1, 7, 8, 9, 16, 17, 24, 25, 31, 32)
CHAIN = (9, 32, 7, 17, 8, 25)
CORNERS = ((32,) * 7, (1,) * 7, (32, 32), (32, 1, 32), (2, 32, 2))
WIDTHS = tuple([(w, 12, 5) for w in EDGE] + [(6, w, 5) for w in EDGE] + [(6, 12, w) for w in EDGE] +
               [CHAIN[:d] + (6,) for d in range(1, 7)] + list(CORNERS))
FEW = ((9, 32, 7, 6), (6, 12, 32), (6, 12, 1))          # the shapes of the separate tests: 6, 32 and 1 classes
ROWS = 1100
N_COLS = 32
SEAM_ROWS = (0, 511, 512, 1099)                         # first row, both sides of a tile seam, the last row
GROUP_SIZES = (1, 2, 11, 50, 100, 275, 550, 1100)       # all divide 1100; most divide neither 64 nor 512
TIE_CASES = (((9, 32, 7, 6), (1, 4)), ((6, 12, 32), (2, 5)), ((6, 12, 32), (3, 11)))   # inside a block of 8, across blocks
BOUND_FACTOR = 4          # tests/test_gpu_classifier.py::test_probabilities_and_labels_match_the_reference
MARGIN_FACTOR = 8
_TARGET = {"relu": 1.0, "tanh": 1.0, "sigmoid": 3.0, "last": 2.0}
_PARAM_SEED, _ROW_SEED = 20, 21
_SALT = {((32, 1, 32), "relu"): 2, ((6, 1, 5), "sigmoid"): 5}


def case_id(widths):
    return "x".join(str(w) for w in widths)


def layer_slices(widths):
    """[(weights start, bias start, n_out, n_in)] of the packed block, per layer."""
    out, pos = [], 0
    for l in range(len(widths) - 1):
        n_in, n_out = int(widths[l]), int(widths[l + 1])
        out.append((pos, pos + n_out * n_in, n_out, n_in))
        pos += n_out * n_in + n_out
    return out


def make_params(widths, act, salt=None):
    """The packed float32 block of a case, calibrated on the case's own rows layer by layer (in float64, on the checker's
    standardised rows): weights U(-1, 1), every output unit scaled so that its pre-activation has standard deviation t
    over the 1100 rows (hidden layers: 1 for relu and tanh, 3 for sigmoid; the last layer: 2; times U(0.6, 1.4) per unit), its bias set so that the
    pre-activation has mean t U(-0.5, 0.5), for relu hidden units 0.3 t more (every unit alive on most rows, dead on
    some).  Plain random initialisation does not do: deep sigmoid networks collapse to one class, deep relu networks
    hold units dead on every row, and a third of a 32-wide network's elements move no probability at all.  A few shapes
    (one hidden unit, two classes) still miss a condition of tests/test_post_shapes_host.py with the first draw and
    take a later one (``_SALT``): the conditions are on the checker alone, no kernel output enters."""
    salt = _SALT.get((tuple(widths), act), 0) if salt is None else salt
    rng = np.random.default_rng([_PARAM_SEED, salt, ACTS.index(act), *widths])
    h, fn = make_feed(widths).x64, href.ACTS[act]
    n_linear, blocks = len(widths) - 1, []
    for l in range(n_linear):
        n_in, n_out, hidden = widths[l], widths[l + 1], l + 1 < n_linear
        t = (_TARGET[act] if hidden else _TARGET["last"]) * rng.uniform(0.6, 1.4, n_out)
        w = rng.uniform(-1.0, 1.0, (n_out, n_in))
        s = (h @ w.T).std(axis=0)
        w = w * (t / np.where(s > 1e-9, s, 1.0))[:, None]
        b = t * (rng.uniform(-0.5, 0.5, n_out) + (0.3 if hidden and act == "relu" else 0.0)) - (h @ w.T).mean(axis=0)
        w, b = w.astype(np.float32), b.astype(np.float32)
        blocks += [w.reshape(-1), b]
        h = h @ w.astype(np.float64).T + b
        if hidden:
            h = fn(h)
    return np.concatenate(blocks)


def two_roundings(x, mean, scale):
    """The scaler's contract: float(float(x - mean) / scale), subtraction and division in IEEE double."""
    c = (np.asarray(x).astype(np.float64) - np.asarray(mean, np.float64)).astype(np.float32)
    return (c.astype(np.float64) / np.asarray(scale, np.float64)).astype(np.float32)


def deranged_columns(rng, n_cols, n_sel):
    """n_sel different columns of n_cols, none in its own place (cols[j] != j); n_cols == 1 has only column 0."""
    if n_cols == 1:
        return np.zeros(n_sel, np.int64)
    while True:
        cols = rng.permutation(n_cols)[:n_sel]
        if (cols != np.arange(n_sel)).all():
            return cols


class Feed:
    """The rows of one case: ``wide`` (1100 x n_cols float32, NaN in the unused columns), ``cols``, float64 ``mean`` /
    ``scale`` of the selected columns, ``scaled32`` (the two roundings: what the second pass is fed) and ``x64`` (the
    float64 standardisation: what the checker is fed)."""

    def __init__(self, widths):
        n_in = int(widths[0])
        rng = np.random.default_rng([_ROW_SEED, *widths])
        self.n_cols = N_COLS
        self.cols = deranged_columns(rng, self.n_cols, n_in)
        x = rng.standard_normal((ROWS, self.n_cols))
        x = (x * rng.uniform(0.2, 4.0, self.n_cols) + rng.uniform(-3.0, 5.0, self.n_cols)).astype(np.float32)
        sel = x[:, self.cols].astype(np.float64)
        self.mean, self.scale = sel.mean(axis=0), sel.std(axis=0)
        unused = np.setdiff1d(np.arange(self.n_cols), self.cols)
        x[:, unused] = np.nan
        self.wide = x
        self.scaled32 = two_roundings(x[:, self.cols], self.mean, self.scale)
        self.x64 = href.standardize64(x, self.cols, self.mean, self.scale)


_feeds = {}


def make_feed(widths):
    """One Feed per width tuple (the activations of a shape share their rows), built once and left unchanged."""
    widths = tuple(widths)
    if widths not in _feeds:
        _feeds[widths] = Feed(widths)
    return _feeds[widths]


# ---------------------------------------------------------------------------------------------------------------------
# classifier: references and comparisons
# ---------------------------------------------------------------------------------------------------------------------
def forward32_torch(x32, widths, params, act, dtype=None):
    """The same layers run by torch on the CPU as the reference's module runs them: linear, activation, softmax.
    float32 by default (the yardstick of the bound); dtype=torch.float64 checks the checker."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float32
    fn = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[act]
    h = torch.from_numpy(np.ascontiguousarray(x32)).to(dtype)
    p = torch.from_numpy(np.asarray(params, np.float32)).to(dtype)
    sl = layer_slices(widths)
    with torch.no_grad():
        for l, (w0, b0, n_out, n_in) in enumerate(sl):
            h = F.linear(h, p[w0:b0].reshape(n_out, n_in), p[b0:b0 + n_out])
            if l + 1 < len(sl):
                h = fn(h)
        return torch.softmax(h, dim=1).numpy()


def forward64(x, widths, params, act):
    with np.errstate(over="ignore"):                    # a saturated sigmoid: exp -> inf -> 0, as the device's
        return href.forward64(x, widths, params, act)


def err32_of(x32, x64, widths, params, act):
    """(p64, err32): the checker's probabilities and the float32 reference's own distance from them."""
    p64 = forward64(x64, widths, params, act)
    p32 = forward32_torch(x32, widths, params, act)
    return p64, float(np.abs(p32.astype(np.float64) - p64).max())


_table = {}


def case_table(act):
    """{widths: (params, p64, err32)} over WIDTHS for one activation, and E(act), the median err32: computed once."""
    if act not in _table:
        rows = {}
        for widths in WIDTHS:
            feed, params = make_feed(widths), make_params(widths, act)
            p64, err = err32_of(feed.scaled32, feed.x64, widths, params, act)
            rows[widths] = (params, p64, err)
        _table[act] = (rows, float(np.median([r[2] for r in rows.values()])))
    return _table[act]


def bound_of(err32, floor):
    """4 x max(err32(case), E(act)): the float32 reference's own error, floored by the activation's median because a few
    cases have a float32 reference that is exact by luck while the device's expf and division still round."""
    return BOUND_FACTOR * max(err32, floor)


def clear_rows(p64, err32, floor, skip=None):
    """(clear, want): rows whose p64 top-two margin exceeds 8 x max(err32, E), and the first argmax of p64.  ``skip``:
    a class left out of both (the second of two tied classes: it never wins, and its twin is no rival)."""
    p = np.array(p64, dtype=np.float64)
    if skip is not None:
        p[:, skip] = -1.0
    if p.shape[1] == 1:
        return np.ones(len(p), bool), np.zeros(len(p), np.int64)
    return href.top_two_margin(p) > MARGIN_FACTOR * max(err32, floor), p.argmax(axis=1)


def compare_probs(p, labels, p64, err32, floor, what, skip=None):
    """THE comparison of the classifier sweeps; returns (worst / bound, rows under the margin rule)."""
    p, labels = np.asarray(p), np.asarray(labels)
    bound = bound_of(err32, floor)
    assert p.dtype == np.float32 and p.shape == p64.shape and labels.shape == (len(p64),), what
    worst = float(np.abs(p.astype(np.float64) - p64).max())
    assert np.isfinite(p).all() and worst <= bound, (
        f"{what}: max|p - p64| = {worst:.3e} beyond {bound:.3e} = 4 x max(err32 {err32:.3e}, E {floor:.3e}); rows "
        f"{np.flatnonzero(~(np.abs(p.astype(np.float64) - p64).max(axis=1) <= bound))[:16].tolist()}")
    assert np.array_equal(labels, p.argmax(axis=1)), f"{what}: a label is not the first maximum of its own probabilities"
    clear, want = clear_rows(p64, err32, floor, skip)
    bad = np.flatnonzero(clear & (labels != want))
    assert bad.size == 0, f"{what}: labels differ from argmax(p64) on clear rows {bad[:16].tolist()}"
    return worst / bound, int((~clear).sum())


def sensitivity(x64, widths, params, act, delta=0.5, first=128):
    """For every element of the packed block: max over rows and classes of |p(element + delta) - p| in float64, by the
    checker's own arithmetic.  Only what lies downstream of the element is recomputed: the element's own output unit,
    a rank-one update of the next layer, whole layers behind that.  The first ``first`` rows are tried alone; an output
    unit with an element that stays under 1e-3 there is redone on all rows."""
    sl = layer_slices(widths)
    p = np.asarray(params, np.float64)
    n_linear, fn = len(sl), href.ACTS[act]
    Ws = [p[w0:b0].reshape(n_out, n_in) for w0, b0, n_out, n_in in sl]
    bs = [p[b0:b0 + n_out] for w0, b0, n_out, n_in in sl]

    def softmax(z):
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)

    def run(rows):
        hs, zs, h = [np.asarray(x64, np.float64)[rows]], [], None
        for l in range(n_linear):
            zs.append(hs[-1] @ Ws[l].T + bs[l])
            hs.append(fn(zs[-1]) if l + 1 < n_linear else zs[-1])
        return hs, zs, softmax(zs[-1])

    def moves(l, o, hs, zs, base):
        """(n_in + 1,): element (o, k) of layer l for every k, then bias o"""
        dz = delta * np.concatenate([hs[l].T, np.ones((1, len(base)))])           # (V, R)
        zc = zs[l][:, o][None, :] + dz
        if l == n_linear - 1:
            z = np.repeat(zs[l][None], len(dz), axis=0)
            z[:, :, o] = zc
        else:
            dh = fn(zc) - hs[l + 1][:, o][None, :]
            z = zs[l + 1][None] + dh[:, :, None] * Ws[l + 1][:, o][None, None, :]
            for m in range(l + 2, n_linear):
                z = fn(z) @ Ws[m].T + bs[m]
        return np.abs(softmax(z) - base[None]).max(axis=(1, 2))

    out = np.zeros(p.size)
    some, full = run(slice(0, first)), None
    for l, (w0, b0, n_out, n_in) in enumerate(sl):
        for o in range(n_out):
            mv = moves(l, o, *some)
            if mv.min() < 1e-3:
                full = full or run(slice(None))
                mv = np.maximum(mv, moves(l, o, *full))
            out[w0 + o * n_in:w0 + (o + 1) * n_in] = mv[:-1]
            out[b0 + o] = mv[-1]
    return out


def last_layer(widths, params):
    """(W, b): writable views of the last layer inside ``params``."""
    w0, b0, n_out, n_in = layer_slices(widths)[-1]
    return params[w0:b0].reshape(n_out, n_in), params[b0:b0 + n_out]


def tie_share(p64, pair):
    """share of the rows on which the tied pair holds the maximum"""
    return float((p64[:, pair[0]] >= p64.max(axis=1)).mean())


def tie_params(widths, act, pair):
    """The case's parameters with class pair[1] a copy of class pair[0] in the last layer (weights and bias), the
    pair's bias raised in steps of 0.25 until it wins on three rows in ten."""
    o, o2 = pair
    params = make_params(widths, act).copy()
    W, b = last_layer(widths, params)
    feed = make_feed(widths)
    W[o2], b[o2] = W[o], b[o]
    for _ in range(400):
        if tie_share(forward64(feed.x64, widths, params, act), pair) >= 0.3:
            return params
        b[o] += np.float32(0.25)
        b[o2] = b[o]
    raise AssertionError(f"tie {widths} {act} {pair}: the pair never wins")


def scaled_last_layer(widths, act, factor):
    params = make_params(widths, act).copy()
    W, b = last_layer(widths, params)
    W *= np.float32(factor)
    b *= np.float32(factor)
    return params


def nan_seam_rows(feed):
    """(wide, bad): the case's matrix with a NaN in a USED column of each of SEAM_ROWS (another column each time)."""
    wide = feed.wide.copy()
    for i, r in enumerate(SEAM_ROWS):
        wide[r, feed.cols[i % len(feed.cols)]] = np.nan
    return wide, np.array(SEAM_ROWS)


def group_counts(labels, rows_per_group, n_classes):
    """np.bincount of the labels per group, label -1 in the extra last bin."""
    lab = np.asarray(labels).reshape(-1, rows_per_group)
    return np.stack([np.bincount(np.where(g < 0, n_classes, g), minlength=n_classes + 1) for g in lab]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
STAT_COLS = tuple(range(1, 33))
STAT_GROUPS = (1, 3)
STAT_PAD = 5                                   # row_stride = n_cols + 5 in the strided pass, NaN in the padding
MANY_GROUPS, MANY_ROWS, MANY_COLS = 131_073, 5, 3        # two pooling slices of 65 535 groups and three groups more
MANY_SEAMS = (65_534, 65_535, 131_069, 131_070)
MEAN_TOL = dict(rtol=1e-12, atol=1e-13)        # tests/test_gpu_postprocess.py::test_statistics_shapes_outliers_and_infinities
STD_TOL = dict(rtol=1e-11, atol=0)


def stat_row_lanes(n_cols):
    return min(256 // n_cols, 32)


def stat_tile_rows(n_cols):
    return 16 * stat_row_lanes(n_cols)


def stat_row_counts(n_cols):
    """Rows per group: 1, L - 1, L, L + 1 (L row lanes: the threads of a column), T - 1, T, T + 1 (T = 16 L, a tile),
    2 T + 3, and 344 T + 7: 345 tiles, which a 3-group call (342 workgroups wanted per group) cuts into 172 chunks of
    two tiles and a last one of a single tile of 7 rows.  A chunk of more than one tile needs more than 1024 tiles in
    the whole call, so this one count is 345 T n_cols floats per group (at most 5.7 MB) and cannot be smaller."""
    L, T = stat_row_lanes(n_cols), stat_tile_rows(n_cols)
    return tuple(sorted({r for r in (1, L - 1, L, L + 1, T - 1, T, T + 1, 2 * T + 3, 344 * T + 7) if r > 0}))


def stat_values(n_groups, rows, n_cols, stride=None, seed=0):
    """(n_groups, rows, stride) float32: normal x 3 plus a per-column offset of order 50 in the first n_cols columns,
    NaN in the padding behind them."""
    rng = np.random.default_rng([30, seed, n_groups, rows, n_cols])
    stride = stride or n_cols
    x = np.full((n_groups, rows, stride), np.nan, np.float32)
    x[:, :, :n_cols] = rng.standard_normal((n_groups, rows, n_cols), np.float32) * np.float32(3) + \
        (rng.standard_normal(n_cols) * 50).astype(np.float32)
    return x


def stat_reference(x, n_cols):
    """numpy's two-pass float64 mean / std of the float64 cast, over the rows of every group."""
    x64 = x[:, :, :n_cols].astype(np.float64)
    return x64.mean(axis=1), x64.std(axis=1)


def compare_stats(mean, std, x, n_cols, what):
    want_m, want_s = stat_reference(x, n_cols)
    assert mean.shape == want_m.shape and std.shape == want_s.shape, what
    assert np.allclose(mean, want_m, **MEAN_TOL), (what, "mean", float(np.nanmax(np.abs(mean - want_m))))
    assert np.allclose(std, want_s, **STD_TOL), (what, "std", float(np.nanmax(np.abs(std / want_s - 1))))
    if x.shape[1] == 1:
        assert (std == 0).all(), (what, "one row: std is exactly 0")


def many_groups_values():
    return stat_values(MANY_GROUPS, MANY_ROWS, MANY_COLS, seed=1)


# ---------------------------------------------------------------------------------------------------------------------
# scaler
# ---------------------------------------------------------------------------------------------------------------------
SCALE_COLS = (1, 18, 32)
SCALE_SELECTIONS = (1, 2, 7, 18, 31, 32)
SCALE_ROWS = (1, 255, 256, 257, 1023, 1024, 1025, 2049)
SCALE_PAD = 3                                  # out_stride = n_sel + 3, row_stride = n_cols + 3
SENTINEL = np.float32(-12345.5)


def scale_selections(n_cols):
    """[(n_sel, cols)] for a column count: a seeded permutation's first n_sel columns, for every n_sel that fits; at
    n_sel of 2, 7 and 32 the last selected column is replaced by a repeat of the first."""
    out = []
    for n_sel in SCALE_SELECTIONS:
        if n_sel > n_cols:
            continue
        rng = np.random.default_rng([40, n_cols, n_sel])
        cols = deranged_columns(rng, n_cols, n_sel) if n_sel > 1 else rng.integers(0, n_cols, 1)
        if n_sel in (7, 32) or (n_sel == 2 and n_cols > 1):
            cols[-1] = cols[0]
        out.append((n_sel, cols.astype(np.int32)))
    return out


def scale_values(rows, n_cols):
    """(rows, n_cols) float32, every column with its own spread (0.01 ... 1000) and offset"""
    rng = np.random.default_rng([41, rows, n_cols])
    x = rng.standard_normal((rows, n_cols)) * 10.0 ** rng.uniform(-2, 3, n_cols) + rng.standard_normal(n_cols) * 50
    return x.astype(np.float32)


def fit_reference(x, cols):
    """(mean, scale) as sklearn's StandardScaler fits them: float64 mean and population std, scale 1 where the variance
    is within its bound for a constant column (sklearn/preprocessing/_data.py _is_constant_feature)."""
    sel = x[:, cols].astype(np.float64)
    n, mean, var = len(sel), sel.mean(axis=0), sel.var(axis=0)
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    return mean, np.where(constant, 1.0, np.sqrt(var))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def explain_scaler_difference(got, x_sel, mean, scale):
    """Which of the two operations differs, and by how much (for the message of a failed bit comparison)."""
    c = (x_sel.astype(np.float64) - mean).astype(np.float32)
    want = (c.astype(np.float64) / scale).astype(np.float32)
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    one = ((x_sel.astype(np.float64) - mean) / scale).astype(np.float32)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    return (f"{len(bad)} of {got.size} elements differ, first at {bad[:4].tolist()}, worst {int(ulps.max())} ulp; "
            f"{int((got.view(np.int32) == one.view(np.int32))[tuple(bad.T)].sum())} of them equal the ONE-rounding quotient "
            f"(the subtraction was not rounded to float32)")
