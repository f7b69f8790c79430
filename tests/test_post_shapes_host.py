"""The cases of the shape sweeps (tests/post_shapes.py), checked without a GPU: a sweep is only as good as its inputs.

Classifier, for the reference alone: (a) every element of every packed block, moved by 0.5, moves some probability of
some row by at least 1e-3 -- so an element that a kernel stages to the wrong place, drops or reads twice shows far above
the bound; (b) at most 2 of the 1100 rows of a case fall under the margin rule; (c) at least min(n_classes, 3) classes
win rows; (d) the float64 checker agrees with torch's float64 run of the same layers to 1e-12.  The tied pairs win their
share, the saturated and large-logit variants stay finite in the checker.

Statistics: the row counts of every column count contain every cut of the kernel, the chunk count taken from the
library (amcx_group_stats_workspace_bytes loads without a GPU); the seams of the pooling slices have different means.

Scaler: the two roundings differ from one rounding somewhere in every case (the contract is observable), the selections
hold what they promise."""
import time

import numpy as np
import pytest

from tests import classifier_host_ref as href
from tests import post_shapes as ps


# ---------------------------------------------------------------------------------------------------------------------
# classifier
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table_holds_what_the_sweep_promises():
    W = ps.WIDTHS
    assert len(W) == len(set(W)) == 41 and all(1 <= len(w) - 1 <= 6 and 1 <= min(w) and max(w) <= 32 for w in W)
    for pos in range(3):
        assert {w[pos] for w in W if len(w) == 3} >= set(ps.EDGE)
    assert {len(w) - 1 for w in W} == {1, 2, 3, 4, 5, 6}
    chain = [w for w in W if w[0] == 9 and w[-1] == 6]
    assert len(chain) == 6 and [-(-w // 8) for w in chain[-1]] == [2, 4, 1, 3, 1, 4, 1]       # blocks of 8 per layer
    assert all(w in W for w in ps.FEW)
    assert ps.ROWS == 2 * 512 + 64 + 12 and all(ps.ROWS % g == 0 for g in ps.GROUP_SIZES)
    assert sum(1 for g in ps.GROUP_SIZES if 64 % g and g % 64) >= 5
    for widths, (o, o2) in ps.TIE_CASES:
        assert o < o2 < widths[-1]
    assert [(o // 8 == o2 // 8) for _, (o, o2) in ps.TIE_CASES] == [True, True, False]


@pytest.mark.parametrize("widths", ps.WIDTHS, ids=ps.case_id)
def test_feed_is_wide_deranged_and_nan_padded(widths):
    f = ps.make_feed(widths)
    n_in = widths[0]
    assert f.wide.shape == (ps.ROWS, 32) and f.wide.dtype == np.float32 and len(set(f.cols.tolist())) == n_in
    assert (f.cols != np.arange(n_in)).all()
    unused = np.setdiff1d(np.arange(32), f.cols)
    assert np.isnan(f.wide[:, unused]).all() and np.isfinite(f.wide[:, f.cols]).all()
    assert len(unused) == 32 - n_in
    # the two roundings do real work: they differ from the single rounding of the float64 quotient on some element
    one = f.x64.astype(np.float32)
    assert not ps.same_bits(one, f.scaled32) or n_in * ps.ROWS < 2000
    assert np.abs(f.x64.mean(axis=0)).max() < 1e-12 and np.abs(f.x64.std(axis=0) - 1).max() < 1e-12
    assert ps.make_feed(widths) is f


@pytest.mark.parametrize("act", ps.ACTS)
def test_every_parameter_element_matters(act):
    """(a).  One-class cases are left out: the softmax of one class is 1 whatever the logit, no element can move it, and
    the GPU test of those cases asks for exactly 1.0 and label 0."""
    t0, worst = time.perf_counter(), {}
    for widths in ps.WIDTHS:
        if widths[-1] == 1:
            continue
        moves = ps.sensitivity(ps.make_feed(widths).x64, widths, ps.make_params(widths, act), act)
        worst[widths] = float(moves.min())
        assert moves.shape == (ps.make_params(widths, act).size,)
        assert moves.min() >= 1e-3, (widths, act, int(moves.argmin()), float(moves.min()), int((moves < 1e-3).sum()))
    low = min(worst, key=worst.get)
    print(f"\n[sensitivity {act}] least move {worst[low]:.2e} in {ps.case_id(low)}; {time.perf_counter() - t0:.1f} s")


def test_sensitivity_recomputes_what_forward64_computes():
    """The downstream-only recomputation against the plain one: element by element on a small case."""
    widths, act = (9, 32, 7, 6), "tanh"
    feed, params = ps.make_feed(widths), ps.make_params(widths, act)
    moves = ps.sensitivity(feed.x64, widths, params, act, first=ps.ROWS)
    base = href.forward64(feed.x64, widths, params, act)
    rng = np.random.default_rng(5)
    for i in list(rng.choice(params.size, 24, replace=False)) + [0, params.size - 1]:
        p = params.astype(np.float64)
        p[i] += 0.5
        plain = np.abs(href.forward64(feed.x64, widths, p, act) - base).max()
        assert abs(plain - moves[i]) <= 1e-12, (i, plain, moves[i])


@pytest.mark.parametrize("act", ps.ACTS)
def test_margin_cap_class_spread_and_checker(act):
    """(b), (c), (d), and the float32 reference inside its own bound."""
    import torch
    rows, floor = ps.case_table(act)
    print(f"\n[{act}] E = median err32 = {floor:.3e}, max err32 = {max(r[2] for r in rows.values()):.3e}")
    assert 1e-8 < floor < 1e-6
    for widths, (params, p64, err) in rows.items():
        feed = ps.make_feed(widths)
        clear, want = ps.clear_rows(p64, err, floor)
        assert (~clear).sum() <= 2, (widths, act, int((~clear).sum()))
        n_cls = widths[-1]
        if n_cls > 1:
            assert len(np.unique(want)) >= min(n_cls, 3), (widths, act, np.bincount(want, minlength=n_cls))
        t64 = ps.forward32_torch(feed.x64, widths, params, act, dtype=torch.float64)
        assert np.abs(t64 - p64).max() <= 1e-12, (widths, act)
        assert np.abs(p64.sum(axis=1) - 1).max() < 1e-12
        p32 = ps.forward32_torch(feed.scaled32, widths, params, act)
        ratio, _ = ps.compare_probs(p32, p32.argmax(axis=1), p64, err, floor, (widths, act))
        assert ratio <= 1 / ps.BOUND_FACTOR + 1e-9


def test_comparison_fails_for_a_wrong_element():
    """compare_probs is not vacuous: one weight of the middle layer set to zero is caught on every activation."""
    widths = (9, 32, 7, 6)
    for act in ps.ACTS:
        rows, floor = ps.case_table(act)
        params, p64, err = rows[widths]
        feed = ps.make_feed(widths)
        broken = params.copy()
        w0 = ps.layer_slices(widths)[1][0]
        broken[w0 + 3 * 32 + 17] = 0
        p = ps.forward32_torch(feed.scaled32, widths, broken, act)
        with pytest.raises(AssertionError):
            ps.compare_probs(p, p.argmax(axis=1), p64, err, floor, "broken")


@pytest.mark.parametrize("act", ps.ACTS)
def test_tied_pairs_win_their_share(act):
    for widths, pair in ps.TIE_CASES:
        params = ps.tie_params(widths, act, pair)
        W, b = ps.last_layer(widths, params)
        assert np.array_equal(W[pair[0]], W[pair[1]]) and b[pair[0]] == b[pair[1]]
        p64 = ps.forward64(ps.make_feed(widths).x64, widths, params, act)
        share = ps.tie_share(p64, pair)
        print(f"\n[tie {ps.case_id(widths)} {act} {pair}] the pair wins {share:.3f} of the rows")
        assert 0.25 <= share < 0.9
        clear, want = ps.clear_rows(p64, 1e-7, 1e-7, skip=pair[1])
        assert (want != pair[1]).all() and clear[want == pair[0]].mean() > 0.9


@pytest.mark.parametrize("act", ps.ACTS)
def test_saturated_and_large_logit_variants_stay_finite_in_the_checker(act):
    for widths in ps.FEW:
        feed = ps.make_feed(widths)
        params = ps.scaled_last_layer(widths, act, 50.0)
        p64 = ps.forward64(feed.x64, widths, params, act)
        assert np.isfinite(p64).all()
        if widths[-1] > 1:                                    # float32 underflows where the checker stays positive
            assert (ps.forward32_torch(feed.scaled32, widths, params, act) == 0).any() and (act == "relu" or (p64 > 0).all())
        if act == "relu":
            continue
        for factor in (1e4, 1e30):
            x = feed.scaled32 * np.float32(factor)
            assert np.isfinite(x).all()
            p64 = ps.forward64(x, widths, ps.make_params(widths, act), act)
            assert np.isfinite(p64).all() and np.abs(p64.sum(axis=1) - 1).max() < 1e-12


def test_nan_seams_and_group_counts():
    feed = ps.make_feed((6, 12, 32))
    wide, bad = ps.nan_seam_rows(feed)
    assert bad.tolist() == [0, 511, 512, 1099]
    assert np.isnan(wide[bad][:, feed.cols]).sum(axis=1).tolist() == [1, 1, 1, 1]
    keep = np.setdiff1d(np.arange(ps.ROWS), bad)
    assert np.array_equal(wide[keep][:, feed.cols], feed.wide[keep][:, feed.cols])
    lab = np.array([0, 2, -1, 2, 1, -1])
    assert ps.group_counts(lab, 3, 3).tolist() == [[1, 0, 1, 1], [0, 1, 1, 1]]


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
def _chunks(n_groups, rows, n_cols):
    from amcpy_amd import _lib
    need = _lib.load().amcx_group_stats_workspace_bytes(n_groups, rows, n_cols)
    assert need > 0 and need % (n_groups * n_cols * 24) == 0
    return need // (n_groups * n_cols * 24)


@pytest.mark.parametrize("n_cols", ps.STAT_COLS)
def test_row_counts_contain_every_cut(n_cols):
    """The chunk count is the library's (its workspace size: three doubles per group, column and chunk).  A cut into c
    chunks of whole tiles with c equal to the number of tiles is one tile per chunk; with fewer chunks than tiles some
    chunk walks more than one tile; a row count that is no multiple of the tile leaves the last chunk ragged."""
    L, T = ps.stat_row_lanes(n_cols), ps.stat_tile_rows(n_cols)
    assert L == min(256 // n_cols, 32) and L * n_cols <= 256 and T == 16 * L
    counts = ps.stat_row_counts(n_cols)
    assert {1, L, L + 1, T - 1, T, T + 1, 2 * T + 3} <= set(counts) and (L - 1 in counts or L == 1)
    tiles = lambda r: -(-r // T)                                                  # noqa: E731
    cuts = {(g, r): _chunks(g, r, n_cols) for g in ps.STAT_GROUPS for r in counts}
    assert all(1 <= c <= tiles(r) for (g, r), c in cuts.items())
    for g in ps.STAT_GROUPS:
        assert any(r < T and cuts[g, r] == 1 for r in counts)                     # a single partial tile
        assert cuts[g, T] == 1                                                    # an exact tile
        assert any(r > T and r % T and cuts[g, r] >= 2 for r in counts)           # a ragged last tile, in a later chunk
        assert any(cuts[g, r] == tiles(r) > 2 and r % T for r in counts)          # several chunks, the last ragged
    big = max(counts)
    assert 1 < cuts[3, big] < tiles(big) and big % T                              # chunks of more than one tile, last ragged
    assert 3 * big * (n_cols + ps.STAT_PAD) * 4 <= 28 << 20


def test_statistics_inputs_and_reference():
    x = ps.stat_values(3, 40, 7, stride=12)
    assert x.shape == (3, 40, 12) and np.isnan(x[:, :, 7:]).all() and np.isfinite(x[:, :, :7]).all()
    m, s = ps.stat_reference(x, 7)
    assert m.shape == s.shape == (3, 7) and np.abs(m).max() > 10 and (np.abs(s - 3) < 1.5).all()
    ps.compare_stats(m, s, x, 7, "self")
    with pytest.raises(AssertionError):                       # one float of padding read as data
        ps.compare_stats(*ps.stat_reference(x, 8), x, 7, "padding")
    shifted = m.copy()
    shifted[1] = m[2]
    with pytest.raises(AssertionError):
        ps.compare_stats(shifted, s, x, 7, "group off by one")
    one = ps.stat_values(1, 1, 5)
    assert (ps.stat_reference(one, 5)[1] == 0).all()


def test_many_groups_seams_have_different_means():
    assert ps.MANY_GROUPS == 2 * 65_535 + 3 and ps.MANY_GROUPS * ps.MANY_ROWS * ps.MANY_COLS * 4 < 8 << 20
    x = ps.many_groups_values()
    m, s = ps.stat_reference(x, ps.MANY_COLS)
    seams = sorted(set(ps.MANY_SEAMS) | {g + d for g in (65_535, 131_070) for d in (-1, 0, 1)})
    for i, a in enumerate(seams):
        for b in seams[i + 1:]:
            assert not np.allclose(m[a], m[b], rtol=1e-3, atol=1e-3), (a, b)
            assert not np.allclose(s[a], s[b], rtol=1e-3, atol=1e-3), (a, b)


# ---------------------------------------------------------------------------------------------------------------------
# scaler
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", ps.SCALE_COLS)
def test_scaler_cases(n_cols):
    sels = ps.scale_selections(n_cols)
    assert [n for n, _ in sels] == [n for n in ps.SCALE_SELECTIONS if n <= n_cols]
    assert all(len(c) == n and c.min() >= 0 and c.max() < n_cols for n, c in sels)
    if n_cols > 1:
        assert any(len(set(c.tolist())) < len(c) for _, c in sels)
        assert any(len(set(c.tolist())) == len(c) == n_cols for _, c in sels) or n_cols == 32
    assert {1023, 1024, 1025, 255, 256, 257, 1, 2049} == set(ps.SCALE_ROWS)
    for rows in ps.SCALE_ROWS:
        x = ps.scale_values(rows, n_cols)
        for n_sel, cols in sels:
            mean, scale = ps.fit_reference(x, cols)
            assert (scale > 0).all() and (rows > 1 or (scale == 1).all())
            two = ps.two_roundings(x[:, cols], mean, scale)
            one = ((x[:, cols].astype(np.float64) - mean) / scale).astype(np.float32)
            assert np.isfinite(two).all()
            if rows * n_sel >= 2049:                          # the contract is observable: the roundings differ somewhere
                assert not ps.same_bits(one, two), (rows, n_sel)
            if rows > 1:
                from sklearn.preprocessing import StandardScaler
                sc = StandardScaler().fit(x[:, cols])
                assert np.allclose(mean, sc.mean_, rtol=1e-12, atol=1e-12) and np.allclose(scale, sc.scale_, rtol=1e-10)
