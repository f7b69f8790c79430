"""Shape sweeps of the kernels behind the feature matrix (needs an MI355X: -m gpu): amcx_mlp_classify_kernel at every
width around a block of 8 in every position, at depth 1 to 6 and at the corners, with exact ties, saturated units, huge
logits, one class, NaN rows at the tile seams, groups that straddle waves and tiles, and a padded probability matrix;
amcx_stats_part_kernel / amcx_stats_combine_kernel at every column count from 1 to 32 and every cut of a group into
tiles and chunks, over padded rows, and over more groups than one pooling launch takes; the two scaler kernels bit for
bit against numpy at every selection width.  Cases, inputs and comparisons are tests/post_shapes.py (checked on the CPU
by tests/test_post_shapes_host.py).

Classifier bound: max|p - p64| <= 4 x max(err32(case), E(act)), p64 the float64 checker on the float64-standardised
rows, err32 the distance from p64 of the same network run by torch on the CPU in float32 on the rows as the scaler
rounds them (computed at run time), E(act) the median of err32 over the activation's 41 cases (measured: 3.7e-7 / 2.7e-7 /
3.7e-7 for relu / tanh / sigmoid).  Labels equal argmax(p64) wherever its top-two margin exceeds 8 x max(err32, E)."""
import ctypes

import numpy as np
import pytest

from tests import post_shapes as ps

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _model(widths, act, params):
    from amcpy_amd.classifier import MlpModel
    return MlpModel(widths, act, params)


def _both_passes(feed, widths, act, params, wide=None):
    """(labels, probs) of the case fed through the wide matrix with mean / scale, after checking that the pass over
    the pre-scaled rows (numpy's two roundings, no mean / scale) gives the same bits."""
    from amcpy_amd.classifier import classify
    model, want = _model(widths, act, params), ("labels", "probs")
    x = _dev(feed.wide if wide is None else wide)
    lab, pr = classify(x, model, cols=feed.cols.tolist(), mean=feed.mean, scale=feed.scale, want=want)
    lab, pr = _host(lab), _host(pr)
    if wide is None:
        lab2, pr2 = classify(_dev(feed.scaled32), model, cols=range(widths[0]), want=want)
        assert np.array_equal(lab, _host(lab2)) and ps.same_bits(pr, _host(pr2)), (widths, act, "pre-scaled pass")
    return lab, pr


def _unscaled(x32, widths, act, params):
    from amcpy_amd.classifier import classify
    lab, pr = classify(_dev(x32), _model(widths, act, params), cols=range(widths[0]), want=("labels", "probs"))
    return _host(lab), _host(pr)


# ---------------------------------------------------------------------------------------------------------------------
# classifier
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ps.ACTS)
def test_classifier_widths_and_depths(act):
    """Every case of tests/post_shapes.py: WIDTHS -- (w, 12, 5), (6, w, 5) and (6, 12, w) for w in 1, 7, 8, 9, 16, 17,
    24, 25, 31, 32, the chain (9, 32, 7, 17, 8, 25) cut at depth 1 to 6 with 6 classes behind it, (32,) * 7, (1,) * 7,
    (32, 32), (32, 1, 32), (2, 32, 2) -- on 1100 rows through a 32-column matrix with deranged columns and NaN in the
    unused ones; the pre-scaled pass bit-identical.  Prints worst / bound per case."""
    rows, floor = ps.case_table(act)
    print(f"\n[classifier {act}] E = median err32 = {floor:.3e}")
    for widths, (params, p64, err) in rows.items():
        lab, pr = _both_passes(ps.make_feed(widths), widths, act, params)
        ratio, under = ps.compare_probs(pr, lab, p64, err, floor, f"classifier {ps.case_id(widths)} {act}")
        print(f"[classifier {act}] {ps.case_id(widths):>20}: err32 {err:.2e}, worst / bound {ratio:.3f}, rows under the margin rule {under}")
        if widths[-1] == 1:
            assert (pr == 1.0).all() and (lab == 0).all()
        else:
            assert np.abs(pr.astype(np.float64).sum(axis=1) - 1).max() < 1e-5 and lab.min() >= 0


@pytest.mark.parametrize("act", ps.ACTS)
def test_exact_ties_keep_the_first_maximum(act):
    """Two classes with identical weights and bias in the last layer, inside one block of 8 and across blocks, winning
    about a third of the rows: their probabilities are bit-identical and the label is never the second of them."""
    _, floor = ps.case_table(act)
    for widths, (o, o2) in ps.TIE_CASES:
        feed, params = ps.make_feed(widths), ps.tie_params(widths, act, (o, o2))
        p64, err = ps.err32_of(feed.scaled32, feed.x64, widths, params, act)
        lab, pr = _both_passes(feed, widths, act, params)
        assert ps.same_bits(pr[:, o], pr[:, o2]), (widths, act, (o, o2))
        assert (lab != o2).all() and (lab == o).mean() >= 0.25, (widths, act, (o, o2), float((lab == o).mean()))
        ratio, _ = ps.compare_probs(pr, lab, p64, err, floor, f"tie {ps.case_id(widths)} {act} {(o, o2)}", skip=o2)
        print(f"\n[tie {act}] {ps.case_id(widths)} {(o, o2)}: the pair wins {(lab == o).mean():.3f}, worst / bound {ratio:.3f}")


@pytest.mark.parametrize("act", ("tanh", "sigmoid"))
def test_saturated_units(act):
    """Inputs times 1e4 and 1e30 (no sum overflows): every probability finite, every label set, the bound as ever.
    Not for relu, whose logits grow with the input until the float64 answer is no float32 target."""
    _, floor = ps.case_table(act)
    for widths in ps.FEW:
        feed, params = ps.make_feed(widths), ps.make_params(widths, act)
        for factor in (1e4, 1e30):
            x = feed.scaled32 * np.float32(factor)
            p64, err = ps.err32_of(x, x.astype(np.float64), widths, params, act)
            lab, pr = _unscaled(x, widths, act, params)
            assert np.isfinite(pr).all() and lab.min() >= 0
            ratio, _ = ps.compare_probs(pr, lab, p64, err, floor, f"saturation x{factor:g} {ps.case_id(widths)} {act}")
            print(f"\n[saturation {act}] {ps.case_id(widths)} x{factor:g}: err32 {err:.2e}, worst / bound {ratio:.3f}")


@pytest.mark.parametrize("act", ps.ACTS)
def test_large_logits(act):
    """The last layer times 50: exponentials underflow to 0 in float32 where p64 stays tiny and positive."""
    _, floor = ps.case_table(act)
    for widths in ps.FEW:
        feed, params = ps.make_feed(widths), ps.scaled_last_layer(widths, act, 50.0)
        p64, err = ps.err32_of(feed.scaled32, feed.x64, widths, params, act)
        lab, pr = _both_passes(feed, widths, act, params)
        ratio, _ = ps.compare_probs(pr, lab, p64, err, floor, f"large logits {ps.case_id(widths)} {act}")
        print(f"\n[large logits {act}] {ps.case_id(widths)}: err32 {err:.2e}, worst / bound {ratio:.3f}, zeros {(pr == 0).mean():.3f}")


@pytest.mark.parametrize("widths", ps.FEW + ((1,) * 7,), ids=ps.case_id)
def test_nan_rule_at_the_seams_and_counts(widths):
    """A NaN in a used column of rows 0, 511, 512 and 1099: label -1, all-NaN probabilities, the extra bin (bin 32 with 32
    classes), every other row's bits as without it; with one class every other row has probability exactly 1.0 and
    label 0.  Counts equal np.bincount of the returned labels per group for rows_per_group of 1, 2, 11, 50, 100, 275,
    550 and 1100."""
    from amcpy_amd.classifier import classify
    n_cls, feed = widths[-1], ps.make_feed(widths)
    wide, bad = ps.nan_seam_rows(feed)
    keep = np.setdiff1d(np.arange(ps.ROWS), bad)
    for act in ps.ACTS:
        params = ps.make_params(widths, act)
        clean_lab, clean_pr = _both_passes(feed, widths, act, params)
        lab, pr = _both_passes(feed, widths, act, params, wide=wide)
        assert (lab[bad] == -1).all() and np.isnan(pr[bad]).all(), (widths, act)
        assert np.array_equal(lab[keep], clean_lab[keep]) and ps.same_bits(pr[keep], clean_pr[keep]), (widths, act)
        if n_cls == 1:
            assert (pr[keep] == 1.0).all() and (lab[keep] == 0).all()
        x, model = _dev(wide), _model(widths, act, params)
        for g in ps.GROUP_SIZES:
            counts = _host(classify(x, model, cols=feed.cols.tolist(), mean=feed.mean, scale=feed.scale, rows_per_group=g,
                                    want=("counts",)))
            want = ps.group_counts(lab, g, n_cls)
            assert counts.shape == want.shape == (ps.ROWS // g, n_cls + 1) and np.array_equal(counts, want), (widths, act, g)
            assert counts[:, n_cls].sum() == len(bad) and counts.sum() == ps.ROWS


@pytest.mark.parametrize("widths", ps.FEW, ids=ps.case_id)
def test_probability_padding_and_output_subsets_through_the_abi(widths):
    """probs_stride = n_classes + 3 with a sentinel in the padding that survives; labels only, probabilities only and
    counts only each equal the call that asks for all three."""
    import torch
    from amcpy_amd import _lib
    lib = _lib.load()
    n_cls, n_in, feed, act, g = widths[-1], widths[0], ps.make_feed(widths), "tanh", 275
    wide, _ = ps.nan_seam_rows(feed)
    x, params = _dev(wide), _dev(ps.make_params(widths, act))
    mean, scale = _dev(feed.mean), _dev(feed.scale)
    cols = (ctypes.c_int32 * n_in)(*feed.cols.tolist())
    w = (ctypes.c_int32 * len(widths))(*widths)
    stride = n_cls + 3

    def call(want):
        lab = torch.full((ps.ROWS,), -7, dtype=torch.int32, device="cuda") if "labels" in want else None
        pr = torch.full((ps.ROWS, stride), float(ps.SENTINEL), dtype=torch.float32, device="cuda") if "probs" in want else None
        cn = torch.full((ps.ROWS // g, n_cls + 1), -7, dtype=torch.int64, device="cuda") if "counts" in want else None
        ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
        _lib.check(lib.amcx_mlp_classify_f32(x.data_ptr(), ps.ROWS, ps.N_COLS, ps.N_COLS, cols, n_in, mean.data_ptr(),
                                             scale.data_ptr(), params.data_ptr(), w, len(widths) - 1, _lib.ACTIVATIONS[act],
                                             ptr(lab), ptr(pr), stride, g if cn is not None else 0, ptr(cn),
                                             torch.cuda.current_stream().cuda_stream))
        return tuple(None if t is None else _host(t) for t in (lab, pr, cn))

    lab, pr, cn = call(("labels", "probs", "counts"))
    assert (pr[:, n_cls:] == ps.SENTINEL).all() and not (pr[:, :n_cls] == ps.SENTINEL).any()
    ref_lab, ref_pr = _both_passes(feed, widths, act, ps.make_params(widths, act), wide=wide)
    assert np.array_equal(lab, ref_lab) and ps.same_bits(pr[:, :n_cls], ref_pr)
    assert np.array_equal(cn, ps.group_counts(lab, g, n_cls))
    only = call(("labels",))
    assert np.array_equal(only[0], lab) and only[1] is None and only[2] is None
    only = call(("probs",))
    assert ps.same_bits(only[1], pr)
    only = call(("counts",))
    assert np.array_equal(only[2], cn)


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
def _stats(x, n_cols):
    from amcpy_amd.postprocess import snr_statistics
    xd = _dev(x)
    view = xd[:, :, :n_cols]
    assert view.stride(1) == x.shape[2]
    mean, std = snr_statistics(view)
    return _host(mean), _host(std)


@pytest.mark.parametrize("n_cols", ps.STAT_COLS)
def test_statistics_every_cut(n_cols):
    """One column count: 1, L - 1, L, L + 1, T - 1, T, T + 1, 2 T + 3 and 344 T + 7 rows per group (L row lanes, T rows
    a tile), 1 group and 3 groups, contiguous rows and rows of n_cols + 5 floats with NaN behind the columns, against
    numpy's two-pass float64 mean / std at the tolerances of test_statistics_shapes_outliers_and_infinities."""
    for rows in ps.stat_row_counts(n_cols):
        for groups in ps.STAT_GROUPS:
            for stride in (n_cols, n_cols + ps.STAT_PAD):
                x = ps.stat_values(groups, rows, n_cols, stride)
                mean, std = _stats(x, n_cols)
                ps.compare_stats(mean, std, x, n_cols, f"statistics {groups} x {rows} x {n_cols}, row stride {stride}")


def test_statistics_wide_row_stride():
    for groups, rows in ((3, ps.stat_row_lanes(18) + 1), (1, 2 * ps.stat_tile_rows(18) + 3)):
        x = ps.stat_values(groups, rows, 18, 4099)
        mean, std = _stats(x, 18)
        ps.compare_stats(mean, std, x, 18, f"statistics {groups} x {rows} x 18, row stride 4099")


def test_statistics_more_groups_than_one_pooling_launch():
    """131 073 groups of 5 rows x 3 columns: the pooling launch goes in two slices of 65 535 groups and one of 3; every
    group is compared (the groups on both sides of each seam have different means: tests/test_post_shapes_host.py)."""
    x = ps.many_groups_values()
    mean, std = _stats(x, ps.MANY_COLS)
    ps.compare_stats(mean, std, x, ps.MANY_COLS, "statistics of 131 073 groups")


# ---------------------------------------------------------------------------------------------------------------------
# scaler
# ---------------------------------------------------------------------------------------------------------------------
def _assert_transform(got, x_sel, mean, scale, what):
    want = ps.two_roundings(x_sel, mean, scale)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert ps.same_bits(got, want), (what, ps.explain_scaler_difference(np.ascontiguousarray(got), x_sel, mean, scale))


@pytest.mark.parametrize("n_cols", ps.SCALE_COLS)
def test_scaler_is_exact(n_cols):
    """select_standardize (fit + transform) and amcx_select_scale_f32 (columns on the device), selections of 1, 2, 7, 18,
    31 and 32 columns as far as they fit (repeats among them), 1, 255, 256, 257, 1023, 1024, 1025 and 2049 rows: the
    transform equals ((x.astype(f8) - mean).astype(f4).astype(f8) / scale).astype(f4) bit for bit, given the mean and
    scale the call returned or was given; the fitted mean / scale are numpy's to rtol 1e-12 / 1e-10.  Through the ABI
    also with rows of n_cols + 3 floats (NaN padding) in and n_sel + 3 floats out (a sentinel that survives)."""
    import torch
    from amcpy_amd import _lib
    from amcpy_amd.postprocess import select_standardize
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    for rows in ps.SCALE_ROWS:
        x = ps.scale_values(rows, n_cols)
        padded = np.full((rows, n_cols + ps.SCALE_PAD), np.nan, np.float32)
        padded[:, :n_cols] = x
        xd, pd = _dev(x), _dev(padded)
        for n_sel, cols in ps.scale_selections(n_cols):
            what = f"scaler {rows} x {n_cols}, columns {cols.tolist()}"
            want_mean, want_scale = ps.fit_reference(x, cols)
            x_sel = x[:, cols]
            # fit + transform through the wrapper, contiguous
            out, mean, scale = select_standardize(xd, cols.tolist())
            out, mean, scale = _host(out), _host(mean), _host(scale)
            assert np.allclose(mean, want_mean, rtol=1e-12, atol=1e-12) and np.allclose(scale, want_scale, rtol=1e-10, atol=0), what
            _assert_transform(out, x_sel, mean, scale, what + " (fit + transform)")
            # fit + transform through the ABI, padded rows in and out
            o_stride = n_sel + ps.SCALE_PAD
            buf = torch.full((rows, o_stride), float(ps.SENTINEL), dtype=torch.float32, device="cuda")
            m2 = torch.empty((n_sel,), dtype=torch.float64, device="cuda")
            s2 = torch.empty_like(m2)
            need = lib.amcx_standardize_workspace_bytes(rows, n_cols)
            ws = torch.empty((int(need),), dtype=torch.uint8, device="cuda")
            cols_c = (ctypes.c_int32 * n_sel)(*cols.tolist())
            _lib.check(lib.amcx_standardize_fit_transform_f32(pd.data_ptr(), rows, n_cols + ps.SCALE_PAD, n_cols, cols_c, n_sel,
                                                              buf.data_ptr(), o_stride, m2.data_ptr(), s2.data_ptr(),
                                                              ws.data_ptr(), ws.numel(), stream))
            got, m2, s2 = _host(buf), _host(m2), _host(s2)
            assert np.array_equal(m2, mean) and np.array_equal(s2, scale), what + " (padded rows: another mean / scale)"
            assert (got[:, n_sel:] == ps.SENTINEL).all(), what + " (fit + transform wrote into the output padding)"
            _assert_transform(got[:, :n_sel], x_sel, m2, s2, what + " (fit + transform, padded)")
            # the plain transform, columns on the device, mean / scale given
            buf = torch.full((rows, o_stride), float(ps.SENTINEL), dtype=torch.float32, device="cuda")
            cd, md, sd = _dev(cols.astype(np.int32)), _dev(want_mean), _dev(want_scale)
            _lib.check(lib.amcx_select_scale_f32(pd.data_ptr(), rows, n_cols + ps.SCALE_PAD, cd.data_ptr(), n_sel,
                                                 md.data_ptr(), sd.data_ptr(), buf.data_ptr(), o_stride, stream))
            got = _host(buf)
            assert (got[:, n_sel:] == ps.SENTINEL).all(), what + " (transform wrote into the output padding)"
            _assert_transform(got[:, :n_sel], x_sel, want_mean, want_scale, what + " (transform)")
