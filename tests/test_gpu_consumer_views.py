"""The consumer entries' alignment gate (include/amcx.h: a pointer aligned to its ELEMENT, 4 bytes for float32 and 8 for
float64) refuses nothing legitimate: views whose data begin 4 bytes behind a 16-byte boundary at a row stride of 19, and a
mean / scale that begin 8 bytes behind one, give the bits of contiguous copies of the same values."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS = [0, 3, 4, 9, 13, 17]


@pytest.fixture(scope="module")
def views():
    """(the (3, 70, 18) view of a (3, 70, 19) tensor, its contiguous copy, mean / scale as [1:7] of 7 doubles, their copies)"""
    import torch
    rng = np.random.default_rng(24)
    base = torch.from_numpy(rng.standard_normal((3, 70, 19)).astype(np.float32)).cuda()
    view = base[..., 1:]
    assert view.data_ptr() % 16 == 4 and view.stride() == (70 * 19, 19, 1)
    mean7 = torch.from_numpy(rng.standard_normal(7)).cuda()
    scale7 = torch.from_numpy(rng.uniform(0.5, 2.0, 7)).cuda()
    mean, scale = mean7[1:7], scale7[1:7]
    assert mean.data_ptr() % 16 == 8 and scale.data_ptr() % 16 == 8 and mean.dtype == torch.float64
    return view, view.contiguous().clone(), mean, scale, mean.clone(), scale.clone()


def _bits(*tensors):
    return [t.cpu().numpy().tobytes() for t in tensors]


def test_snr_statistics_on_a_view_gives_the_bits_of_its_copy(views):
    from amcpy_amd.postprocess import snr_statistics
    view, copy = views[:2]
    got, want = snr_statistics(view), snr_statistics(copy)
    assert got[0].shape == (3, 18) and _bits(*got) == _bits(*want)


def test_select_standardize_on_a_view_gives_the_bits_of_its_copy(views):
    from amcpy_amd.postprocess import select_standardize
    view, copy = views[:2]
    rows = view.reshape(-1, 18)                                               # still the view: 210 rows at stride 19
    assert rows.data_ptr() == view.data_ptr() and rows.stride() == (19, 1)
    got, want = select_standardize(rows, COLS), select_standardize(copy.reshape(-1, 18), COLS)
    assert got[0].shape == (210, 6) and _bits(*got) == _bits(*want)


def test_classify_on_views_gives_the_bits_of_their_copies(views):
    from amcpy_amd.classifier import MlpModel, classify, params_floats
    view, copy, mean, scale, mean_c, scale_c = views
    widths = (6, 5, 3)
    model = MlpModel(widths, "relu", np.random.default_rng(6).standard_normal(params_floats(widths)).astype(np.float32))
    want_all = ("labels", "probs", "counts")
    got = classify(view, model, cols=COLS, mean=mean, scale=scale, want=want_all)
    want = classify(copy, model, cols=COLS, mean=mean_c, scale=scale_c, want=want_all)
    assert got[0].shape == (3, 70) and got[1].shape == (3, 70, 3) and got[2].shape == (3, 4)
    assert int(got[2].sum()) == 210 and _bits(*got) == _bits(*want)
