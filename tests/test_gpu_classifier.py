"""GPU tests of the classifier (amcx_mlp_classify_f32 behind amcpy_amd.classifier): parity with the reference's own
probabilities, the two-rounding and batching contracts bit for bit, the per-group counts and the NaN rule, graph
capture, IQ -> label end to end, and the `classify` command.  Fixtures: tests/golden/classifier_*.npz, written by
tests/golden/make_classifier_fixtures.py from the reference's model class on the CPU."""
import ctypes
import importlib.util
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
USED = (2, 4, 6, 8, 12, 14)
BIG = 638_976


def _href():
    spec = importlib.util.spec_from_file_location("classifier_host_ref", REPO / "tests" / "classifier_host_ref.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fixture_model(name):
    from amcpy_amd.classifier import MlpModel
    z = np.load(GOLDEN / f"classifier_{name}.npz", allow_pickle=False)
    return z, MlpModel.from_state_dict(_href().state_dict_of(z), str(z["activation"]))


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


def _big_rows(n=BIG, seed=11):
    """A feature-like matrix on the device: 18 columns of different offsets and spreads."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, 18), generator=g, device="cuda", dtype=torch.float32)
    off = torch.linspace(-3.0, 5.0, 18, device="cuda")
    spread = torch.linspace(0.2, 4.0, 18, device="cuda")
    return x * spread + off


@pytest.mark.parametrize("name", ["ref_relu", "ref_tanh", "ref_sigmoid", "ref_odd"])
def test_probabilities_and_labels_match_the_reference(name):
    """max|p_gpu - p64| <= 4 x ref32_err over all 8192 rows (ref32_err: the reference's own float32 deviation from its
    float64 self, stored in the fixture; the factor covers the folded BatchNorm, the summation order and the device's
    exp / tanh, each a rounding source of the reference's own size).  Labels equal argmax(p64) on every row whose p64
    top-two margin exceeds 8 x ref32_err; at most 0.1 % of the rows (8) may be left out."""
    import torch
    from amcpy_amd.classifier import classify
    href = _href()
    z, model = _fixture_model(name)
    x = torch.from_numpy(z["x"]).cuda()
    labels, probs = classify(x, model, cols=range(model.n_inputs), want=("labels", "probs"))
    torch.cuda.synchronize()
    p, lab, p64, err = probs.cpu().numpy().astype(np.float64), labels.cpu().numpy(), z["p64"], float(z["ref32_err"])
    worst = np.abs(p - p64).max()
    print(f"\n{name}: max|p_gpu - p64| = {worst:.3e} = {worst / err:.2f} x ref32_err ({err:.3e})")
    assert probs.dtype == torch.float32 and labels.dtype == torch.int32 and p.shape == p64.shape
    assert np.abs(p.sum(axis=1) - 1).max() < 1e-5 and lab.min() >= 0
    assert worst <= 4 * err
    clear = href.top_two_margin(p64) > 8 * err
    left_out = 1.0 - clear.mean()
    print(f"{name}: rows left out by the margin rule: {int((~clear).sum())} of {len(clear)}")
    assert left_out <= 0.001
    assert np.array_equal(lab[clear], p64.argmax(1)[clear])
    assert np.array_equal(lab, p.argmax(1))                       # the label is the first maximum of its own probabilities


def test_two_roundings_and_batching_are_bit_exact():
    """classify(x, cols, mean, scale) == classify(amcx_select_scale_f32's output, no mean) bit for bit (the scaler's
    two float32 roundings), and a row's bits do not depend on batching or alignment: the whole matrix, two halves, a
    row-strided view, rows offset by one, and n_rows of 1 / 63 / 64 / 65 / 638 976."""
    import torch
    from amcpy_amd import _lib
    from amcpy_amd.classifier import classify
    from amcpy_amd.postprocess import select_standardize
    _, model = _fixture_model("ref_relu")
    x = _big_rows()
    scaled, mean, scale = select_standardize(x, USED)
    both = ("labels", "probs")
    lab, pr = classify(x, model, cols=USED, mean=mean, scale=scale, want=both)
    lab2, pr2 = classify(scaled, model, cols=range(6), want=both)
    assert _same(lab, lab2) and _same(pr, pr2)
    # the same through the plain transform entry point (columns on the device)
    out = torch.empty_like(scaled)
    cols_dev = torch.tensor(USED, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().amcx_select_scale_f32(x.data_ptr(), BIG, 18, cols_dev.data_ptr(), 6, mean.data_ptr(),
                                                 scale.data_ptr(), out.data_ptr(), 6,
                                                 torch.cuda.current_stream().cuda_stream))
    lab3, pr3 = classify(out, model, cols=range(6), want=both)
    assert _same(lab, lab3) and _same(pr, pr3)
    # host copies of mean / scale give the same bits as the device ones
    lab4 = classify(x, model, cols=USED, mean=mean.cpu().numpy(), scale=scale.cpu().numpy())
    assert _same(lab, lab4)
    assert int((lab >= 0).sum()) == BIG and len(torch.unique(lab)) == 6
    half = BIG // 2 + 37
    for lo, hi in ((0, half), (half, BIG), (1, BIG), (0, 1), (5, 68), (0, 63), (0, 64), (0, 65), (BIG - 65, BIG)):
        l, p = classify(x[lo:hi], model, cols=USED, mean=mean, scale=scale, want=both)
        assert _same(l, lab[lo:hi]) and _same(p, pr[lo:hi]), (lo, hi)
    wide = torch.full((100_000, 24), float("nan"), device="cuda")
    wide[:, :18] = x[:100_000]
    l, p = classify(wide[:, :18], model, cols=USED, mean=mean, scale=scale, want=both)
    assert wide[:, :18].stride(0) == 24 and _same(l, lab[:100_000]) and _same(p, pr[:100_000])
    l, p = classify(x[:100_000:2], model, cols=USED, mean=mean, scale=scale, want=both)
    assert _same(l, lab[:100_000:2]) and _same(p, pr[:100_000:2])
    # leading dimensions are only a shape
    l = classify(x[:96_000].reshape(6, 16, 1000, 18), model, cols=USED, mean=mean, scale=scale)
    assert l.shape == (6, 16, 1000) and _same(l.reshape(-1), lab[:96_000])
    empty = classify(x[:0], model, cols=USED, mean=mean, scale=scale)
    assert empty.shape == (0,)


def test_counts_and_the_nan_rule():
    """counts == np.bincount of the returned labels per group, for 6 x 16 groups of 1000 and for one group of 638 976.
    A row with a NaN / inf in a USED column gets label -1, NaN probabilities and lands in the extra bin; a NaN in an
    unused column changes nothing."""
    import torch
    from amcpy_amd.classifier import classify
    _, model = _fixture_model("ref_relu")
    x = _big_rows(seed=12)
    mean = x[:, list(USED)].double().mean(0)
    scale = x[:, list(USED)].double().std(0)
    kw = dict(cols=USED, mean=mean, scale=scale)
    clean_lab, clean_pr = classify(x, model, want=("labels", "probs"), **kw)
    bad_nan, bad_inf, bad_ninf, harmless = 5, 1999, 95_999, 77
    x[bad_nan, 4] = float("nan")
    x[bad_inf, 2] = float("inf")
    x[bad_ninf, 14] = float("-inf")
    x[harmless, 3] = float("nan")                                   # column 3 is not used
    x[BIG - 1, 12] = float("nan")
    lab, pr, counts = classify(x[:96_000].reshape(6, 16, 1000, 18), model, want=("labels", "probs", "counts"), **kw)
    assert counts.shape == (6, 16, 7) and counts.dtype == torch.int64
    lab_h, counts_h = lab.cpu().numpy().reshape(96, 1000), counts.cpu().numpy().reshape(96, 7)
    for g in range(96):
        want = np.bincount(np.where(lab_h[g] < 0, 6, lab_h[g]), minlength=7)
        assert np.array_equal(counts_h[g], want), g
    assert counts_h.sum() == 96_000 and counts_h[:, 6].sum() == 3
    flat_lab, flat_pr = lab.reshape(-1), pr.reshape(-1, 6)
    for r in (bad_nan, bad_inf, bad_ninf):
        assert int(flat_lab[r]) == -1 and bool(torch.isnan(flat_pr[r]).all()), r
    keep = torch.ones(96_000, dtype=torch.bool, device="cuda")
    keep[[bad_nan, bad_inf, bad_ninf]] = False
    assert _same(flat_lab[keep], clean_lab[:96_000][keep]) and _same(flat_pr[keep], clean_pr[:96_000][keep])
    assert int(flat_lab[harmless]) == int(clean_lab[harmless]) >= 0
    # groups that do not line up with waves or tiles, and a grouping given explicitly on a 2-D matrix
    c2 = classify(x[:96_000], model, rows_per_group=750, want=("counts",), **kw).cpu().numpy()
    l2 = flat_lab.cpu().numpy().reshape(128, 750)
    assert c2.shape == (128, 7)
    assert all(np.array_equal(c2[g], np.bincount(np.where(l2[g] < 0, 6, l2[g]), minlength=7)) for g in range(128))
    with pytest.raises(ValueError):
        classify(x[:96_000], model, rows_per_group=999, want=("counts",), **kw)
    # one group of everything
    lab_all, c_all = classify(x, model, want=("labels", "counts"), **kw)
    la = lab_all.cpu().numpy()
    assert c_all.shape == (1, 7)
    assert np.array_equal(c_all.cpu().numpy()[0], np.bincount(np.where(la < 0, 6, la), minlength=7))
    assert int(c_all[0, 6]) == 4 and int(c_all.sum()) == BIG
    # counts alone, and counts are zeroed by the call itself
    again = classify(x, model, want=("counts",), **kw)
    assert torch.equal(again, c_all)


def test_graph_capture_replays_to_the_same_bits():
    """The call allocates nothing and synchronises nothing: captured on a single stream (no parallel branches) it
    replays to the bits of the eager call, on inputs changed after the capture too."""
    import torch
    from amcpy_amd import _lib
    _, model = _fixture_model("ref_tanh")
    n = 96_000
    x = _big_rows(n, seed=13)
    mean = x[:, list(USED)].double().mean(0)
    scale = x[:, list(USED)].double().std(0)
    params = model.device_params(x.device)
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    probs = torch.empty((n, 6), dtype=torch.float32, device="cuda")
    counts = torch.empty((96, 7), dtype=torch.int64, device="cuda")
    cols = (ctypes.c_int32 * 6)(*USED)
    widths = (ctypes.c_int32 * 5)(*model.widths)
    lib = _lib.load()

    def call():
        _lib.check(lib.amcx_mlp_classify_f32(x.data_ptr(), n, 18, 18, cols, 6, mean.data_ptr(), scale.data_ptr(),
                                             params.data_ptr(), widths, 4, _lib.ACT_TANH, labels.data_ptr(), probs.data_ptr(),
                                             6, 1000, counts.data_ptr(), torch.cuda.current_stream().cuda_stream))

    call()
    torch.cuda.synchronize()
    eager = (labels.clone(), probs.clone(), counts.clone())
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    for t in (labels, probs, counts):
        t.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(labels, eager[0]) and _same(probs, eager[1]) and torch.equal(counts, eager[2])
    x.copy_(_big_rows(n, seed=14))                                 # new inputs in the captured buffers
    graph.replay()
    torch.cuda.synchronize()
    replayed = (labels.clone(), probs.clone(), counts.clone())
    call()
    torch.cuda.synchronize()
    assert _same(labels, replayed[0]) and _same(probs, replayed[1]) and torch.equal(counts, replayed[2])
    assert not _same(labels, eager[0])


def test_iq_to_label_end_to_end():
    """classify_frames on the fixture's held-out frames (regenerated on the host exactly as the generator did,
    N = 1024): labels agree with the CPU chain's (CPU checker features -> float64 scaler -> the reference's model in
    float64) on every row whose p64 top-two margin exceeds 8 x ref32_err, at most 0.1 % of the rows left out, and the
    accuracy differs from the recorded one by no more than the left-out share.  The features come from the no-FFT
    plan kernel."""
    import torch
    from amcpy_amd import _lib, synth
    from amcpy_amd.classifier import classify_frames
    href = _href()
    z, model = _fixture_model("synth6")
    n, N = int(z["heldout_frames"]), int(z["frame_size"])
    iq = np.concatenate([synth.host_block(synth.MODS6[int(mi)], float(snr), n, N, seed=int(seed))
                         for mi, snr, seed in z["heldout_seeds"]]).astype(np.complex64)
    cols = [int(c) for c in z["cols"]]
    assert cols == list(USED)
    mask = _lib.feature_mask([c + 1 for c in cols])
    assert _lib.kernel_name_subset(N, _lib.VARIANT_AUTO, mask) == f"amcx_features_subset_wave_kernel<{N}, 1>"
    labels, counts = classify_frames(torch.from_numpy(iq).cuda(), model, cols=cols, mean=z["mean"], scale=z["scale"],
                                     rows_per_group=n, want=("labels", "counts"))
    torch.cuda.synchronize()
    lab, true, want = labels.cpu().numpy(), z["true"], z["labels"]
    assert lab.shape == want.shape == (iq.shape[0],) and lab.min() >= 0
    clear = href.top_two_margin(z["p64"]) > 8 * float(z["ref32_err"])
    left_out = 1.0 - clear.mean()
    differ = int((lab != want).sum())
    acc = float((lab == true).mean())
    print(f"\nend to end: {differ} of {len(lab)} labels differ from the CPU chain, {int((~clear).sum())} rows left out, "
          f"accuracy {acc:.4f} (CPU chain {float(z['accuracy']):.4f})")
    assert left_out <= 0.001
    assert np.array_equal(lab[clear], want[clear])
    assert abs(acc - float(z["accuracy"])) <= left_out + 1e-12
    c = counts.cpu().numpy()
    assert c.shape == (36, 7) and c.sum() == len(lab) and c[:, 6].sum() == 0
    assert np.array_equal(c[:, :6], np.stack([np.bincount(g, minlength=6) for g in lab.reshape(36, n)]))


def test_classify_command_from_iq(tmp_path):
    """`python -m amcpy_amd classify --from-iq` in a fresh child process on a synthetic root of the default SNR grid
    (6 modulations x 16 SNRs x 64 frames x 1024 samples): writes figures/{model_id}_figure_data.mat with `acc` of
    shape (6, 16) float64 -- the reference's evaluate_by_snr file -- equal to evaluate_by_snr called in process on the
    files the command extracted, and {mod}_predictions.mat (int32 (n_snr, n_frames)) beside them."""
    import scipy.io
    import torch
    from amcpy_amd import synth
    from amcpy_amd.classifier import classify, evaluate_by_snr
    from amcpy_amd.config import Config, Paths, SignalConfig
    from amcpy_amd.postprocess import select_standardize
    n_snr, n_frames, fs = 16, 64, 1024
    cfg = Config(paths=Paths(root=tmp_path), signals=SignalConfig(num_frames=n_frames, frame_size=fs))
    cfg.paths.ensure_dirs()
    blocks = synth.host_frames(synth.MODS6, n_snr, n_frames, fs)
    scipy.io.savemat(str(cfg.paths.mat_data / cfg.paths.mat_filename), {cfg.signals.mat_info[m]: blocks[m] for m in synth.MODS6})
    _, model = _fixture_model("synth6")
    model.save_npz(tmp_path / "synth6.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["PYTHONPATH"] = str(REPO) + os.pathsep + os.environ.get("PYTHONPATH", "")
    cmd = [sys.executable, "-m", "amcpy_amd", "classify", "--root", str(tmp_path), "--model", str(tmp_path / "synth6.npz"),
           "--from-iq", "--mode", "training", "--num-frames", str(n_frames), "--frame-size", str(fs)]
    r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "accuracy per modulation" in r.stdout
    got = scipy.io.loadmat(str(cfg.paths.figures / "synth6_figure_data.mat"))["acc"]
    assert got.shape == (6, 16) and got.dtype == np.float64
    feats = np.ascontiguousarray(np.stack([
        scipy.io.loadmat(str(cfg.paths.calculated_features / f"{m}_features.mat"))[cfg.signals.mat_info[m]] for m in synth.MODS6]))
    assert feats.shape == (6, n_snr, n_frames, 18) and feats.dtype == np.float32
    dev = torch.from_numpy(feats).cuda()
    fit = dev[:, list(cfg.training.training_snr)].reshape(-1, 18)
    _, mean, scale = select_standardize(fit, USED)
    acc, confusion = evaluate_by_snr(dev, model, cols=USED, mean=mean, scale=scale, labels=cfg.signals.labels)
    assert acc.shape == (6, 16) and acc.dtype == np.float64
    assert np.array_equal(acc, got)
    assert confusion.shape == (6, 7) and confusion.sum() == 6 * n_snr * n_frames and confusion[:, 6].sum() == 0
    labels = classify(dev, model, cols=USED, mean=mean, scale=scale).cpu().numpy()
    for i, m in enumerate(synth.MODS6):
        pred = scipy.io.loadmat(str(cfg.paths.calculated_features / f"{m}_predictions.mat"))["predictions"]
        assert pred.dtype == np.int32 and pred.shape == (n_snr, n_frames) and np.array_equal(pred, labels[i])
        assert np.array_equal(acc[i], (labels[i] == i).mean(axis=1))
