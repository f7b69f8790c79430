"""Fixed-point deployment on the device (include/amcx.h ABI 16; amcpy_amd/quantize.py): amcx_mlp_range_f32 and
amcx_mlp_classify_q15 against tests/quantize_ref.py.  Integer arithmetic, and min / max of float32 sums taken in a fixed
order, leave nothing to a tolerance: every comparison below is ``==``."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import quantize_ref as qr
from tests.classifier_host_ref import state_dict_of

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
USED = (2, 4, 6, 8, 12, 14)
# widths 1, 7, 8, 9, 31, 32 on either side of a layer, depths 1 ... 6
SHAPES = ((1, 1), (7, 8, 9), (32, 31, 1), (9, 32, 32, 7), (8, 1, 31, 9, 32), (31, 7, 32, 8, 9, 2), (6, 8, 7, 9, 32, 31, 5))
ROWS = (1, 63, 64, 65, 513)


def _rng(*key):
    return np.random.default_rng([20240611, *key])


def _float_case(widths, n_rows, seed, n_cols=None, bad_rows=()):
    """(rows float32 (n_rows, n_cols), cols, mean, scale, packed float32 block)."""
    g = _rng(seed, n_rows, *widths)
    n_cols = n_cols or min(32, widths[0] + 3)
    cols = [int(c) for c in g.permutation(n_cols)[:widths[0]]]
    rows = (g.standard_normal((n_rows, n_cols)) * 3 + 0.5).astype(np.float32)
    for r, c, v in bad_rows:
        rows[r % n_rows, cols[c % len(cols)]] = v
    mean, scale = g.standard_normal(widths[0]), 0.5 + g.random(widths[0]) * 2
    block = np.concatenate([np.concatenate([(g.standard_normal(widths[l + 1] * widths[l]) * 1.3 / np.sqrt(widths[l])),
                                            g.standard_normal(widths[l + 1]) * 0.4]) for l in range(len(widths) - 1)]).astype(np.float32)
    return rows, cols, mean, scale, block


def _model(widths, block):
    from amcpy_amd.classifier import MlpModel
    return MlpModel(widths, "relu", block)


def _view(rows, pad_rows=3, pad_left=2, pad_right=5):
    """The rows as an offset, strided view of a larger CUDA tensor."""
    import torch
    big = torch.full((rows.shape[0] + pad_rows, rows.shape[1] + pad_left + pad_right), float("nan"), dtype=torch.float32, device="cuda")
    view = big[pad_rows:, pad_left:pad_left + rows.shape[1]]
    view.copy_(torch.from_numpy(rows))
    assert view.storage_offset() > 0 and (rows.shape[0] == 1 or view.stride(0) > rows.shape[1])
    return view


# ---- calibration -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["relu", "none"])
def test_ranges_equal_the_float32_restatement(activation):
    import torch
    from amcpy_amd import quantize as qz
    bad = ((0, 0, np.nan), (5, 1, np.inf), (70, 2, -np.inf), (200, 0, np.nan), (64, 0, 3.0e38))
    for i, widths in enumerate(SHAPES):
        for n_rows in ROWS:
            rows, cols, mean, scale, block = _float_case(widths, n_rows, i, bad_rows=bad if n_rows >= 63 and i % 2 else ())
            want, want_skipped = qr.ranges32(rows, cols, mean, scale, widths, block, activation)
            model = _model(widths, block)
            for feats in (torch.from_numpy(rows).cuda(), _view(rows)):
                got, skipped = qz.calibrate(feats, model, cols=cols, mean=mean, scale=scale, activation=activation)
                assert got.dtype == np.float32 and got.shape == (len(widths), 2)
                assert np.array_equal(got, want) and skipped == want_skipped, (widths, n_rows, got, want, skipped, want_skipped)
    # rows standardised already (no scaler), and rows all of which are skipped: the ranges stay (+inf, -inf)
    rows, cols, _, _, block = _float_case((7, 8, 9), 65, 99)
    got, skipped = qz.calibrate(torch.from_numpy(rows).cuda(), _model((7, 8, 9), block), cols=cols, activation=activation)
    want, _ = qr.ranges32(rows, cols, None, None, (7, 8, 9), block, activation)
    assert np.array_equal(got, want) and skipped == 0
    rows[:, cols[0]] = np.nan
    got, skipped = qz.calibrate(torch.from_numpy(rows).cuda(), _model((7, 8, 9), block), cols=cols, activation=activation)
    assert skipped == 65 and np.all(got[:, 0] == np.inf) and np.all(got[:, 1] == -np.inf)


def test_ranges_over_many_tiles_and_every_workgroup():
    """100 003 rows: more tiles than one round of workgroups, the last one partial; NaN and inf rows scattered."""
    import torch
    from amcpy_amd import quantize as qz
    widths, n_rows = (6, 9, 4), 100_003
    bad = tuple((r, r % 6, v) for r, v in ((0, np.nan), (511, np.inf), (512, -np.inf), (51_234, np.nan), (100_002, np.inf)))
    rows, cols, mean, scale, block = _float_case(widths, n_rows, 7, n_cols=18, bad_rows=bad)
    for activation in ("relu", "none"):
        want, want_skipped = qr.ranges32(rows, cols, mean, scale, widths, block, activation)
        got, skipped = qz.calibrate(torch.from_numpy(rows).cuda(), _model(widths, block), cols=cols, mean=mean, scale=scale,
                                    activation=activation)
        assert np.array_equal(got, want) and skipped == want_skipped == 5


@pytest.mark.parametrize("name", ["default", "spread", "ties"])
def test_fixture_networks_give_the_references_info_strings(name):
    """The device's ranges of the Linear-only, activation-free chain choose the formats the reference's torch calls chose."""
    import torch
    from amcpy_amd import quantize as qz
    z = np.load(GOLDEN / f"quantize_ref_{name}.npz", allow_pickle=False)
    sd = state_dict_of(z)
    lin = qz.linear_model(sd)
    ranges, skipped = qz.calibrate(torch.from_numpy(z["x"]).cuda(), lin, cols=range(lin.n_inputs), activation="none")
    assert skipped == 0 and np.array_equal(ranges[0], z["ranges"][0])
    assert np.allclose(ranges, z["ranges"], rtol=1e-5, atol=1e-6)                 # torch's GEMM sums in another order
    q = qz.QuantizedMlp.from_state_dict(sd, ranges, layout="reference")
    save, info = q.reference_export()
    assert info == dict(zip((str(k) for k in z["info_keys"]), (str(v) for v in z["info_values"])))
    assert np.array_equal(save["weights"], z["weights"]) and np.array_equal(save["biases"], z["biases"])


# ---- the integer network -----------------------------------------------------------------------------------------------------------
def _q15_case(widths, n_rows, seed, full):
    """Random int16 parameters -- the whole int16 range (`full`) or moderate ones -- and formats the ABI admits."""
    g = _rng(seed, n_rows, int(full), *widths)
    n_linear = len(widths) - 1
    n_cols = min(32, widths[0] + 2)
    cols = [int(c) for c in g.permutation(n_cols)[:widths[0]]]
    rows = (g.standard_normal((n_rows, n_cols)) * 2).astype(np.float32)
    mean, scale = g.standard_normal(widths[0]) * 0.3, 0.5 + g.random(widths[0])
    hi = 32768 if full else 1 << 10
    block = np.concatenate([g.integers(-hi, hi, widths[l + 1] * widths[l] + widths[l + 1]) for l in range(n_linear)]).astype(np.int16)
    fi, fw, fb, fo = int(g.integers(9, 16)), g.integers(9, 16, n_linear), g.integers(9, 16, n_linear), g.integers(9, 16, n_linear)
    return rows, cols, mean, scale, block, fi, [int(v) for v in fw], [int(v) for v in fb], [int(v) for v in fo]


def _qmodel(widths, block, fi, fw, fb, fo):
    from amcpy_amd.quantize import QuantizedMlp
    return QuantizedMlp(widths, block, fi, fw, fb, fo)


def _check_q15(feats, rows, cols, mean, scale, q, rows_per_group, tag):
    from amcpy_amd import quantize as qz
    want = qr.classify_q15(rows, cols, mean, scale, q.widths, q.params, q.frac_input, q.frac_weights, q.frac_biases, q.frac_outputs,
                           rows_per_group)
    labels, logits, counts, saturated = qz.classify_q15(feats, q, cols=cols, mean=mean, scale=scale, rows_per_group=rows_per_group)
    labels, logits, counts, saturated = (t.cpu().numpy() for t in (labels, logits, counts, saturated))
    assert labels.dtype == np.int32 and logits.dtype == np.int16 and counts.dtype == np.int64 and saturated.dtype == np.int64
    assert np.array_equal(logits, want[1]), tag
    assert np.array_equal(labels, want[0]), tag
    assert np.array_equal(counts, want[2]) and counts.sum() == rows.shape[0], tag
    assert np.array_equal(saturated, want[3]), (tag, saturated, want[3])
    return want


GROUPS = {1: (1,), 63: (1, 9, 63), 64: (1, 8, 64), 65: (5, 13, 65), 513: (19, 27, 513)}


@pytest.mark.parametrize("full", [False, True], ids=["moderate", "full_range"])
def test_q15_equals_the_int64_restatement(full):
    import torch
    bad = ((2, 0, np.nan), (40, 1, np.inf), (64, 0, -np.inf), (300, 2, np.nan))
    for i, widths in enumerate(SHAPES):
        for n_rows in ROWS:
            rows, cols, mean, scale, block, fi, fw, fb, fo = _q15_case(widths, n_rows, i, full)
            if i % 2:
                for r, c, v in bad:
                    rows[r % n_rows, cols[c % len(cols)]] = v
            q = _qmodel(widths, block, fi, fw, fb, fo)
            rpg = GROUPS[n_rows][i % len(GROUPS[n_rows])]
            feats = _view(rows) if (i + n_rows) % 2 else torch.from_numpy(rows).cuda()
            _check_q15(feats, rows, cols, mean, scale, q, rpg, (widths, n_rows, full))


def test_q15_over_many_tiles_and_every_workgroup():
    import torch
    widths, n_rows = (6, 26, 29, 30, 6), 100_003
    rows, cols, mean, scale, block, *_ = _q15_case(widths, n_rows, 3, False)
    fi, fw, fb, fo = 11, [12] * 4, [12] * 4, [10] * 4          # (formats under which this block's labels are spread over four classes)
    for r, v in ((0, np.nan), (511, np.inf), (512, -np.inf), (51_234, np.nan), (100_002, np.inf)):
        rows[r, cols[r % 6]] = v
    want = _check_q15(torch.from_numpy(rows).cuda(), rows, cols, mean, scale, _qmodel(widths, block, fi, fw, fb, fo), n_rows, "big")  # (100 003 is prime: one group)
    assert (want[0] == -1).sum() == 5 and want[2][:, -1].sum() == 5 and len(set(want[0].tolist())) >= 4


def test_every_format_in_every_role_and_the_extreme_shifts():
    import torch
    widths, n_rows = (6, 8, 4), 65
    rows, cols, mean, scale, block, *_ = _q15_case(widths, n_rows, 5, False)
    feats = torch.from_numpy(rows).cuda()
    for role in range(4):
        for n in range(9, 16):
            f = [[12], [12, 12], [12, 12], [12, 12]]
            f[role] = [n] * len(f[role])
            _check_q15(feats, rows, cols, mean, scale, _qmodel(widths, block, f[0][0], f[1], f[2], f[3]), 13, (role, n))
    # the smallest shifts the ABI admits (P = Nb: the bias as it is; P - No = 1) and the largest (P = 30 with Nb = No = 0)
    _check_q15(feats, rows, cols, mean, scale, _qmodel(widths, block, 0, [1, 1], [1, 1], [0, 0]), 5, "smallest")
    _check_q15(feats, rows, cols, mean, scale, _qmodel(widths, block, 15, [15, 15], [0, 0], [0, 14]), 5, "largest")
    full = _q15_case(widths, n_rows, 6, True)[4]
    _check_q15(feats, rows, cols, mean, scale, _qmodel(widths, full, 15, [15, 15], [0, 0], [0, 14]), 5, "largest, full range")


def _direct(a, widths, block, fi, fw, fb, fo, rows_per_group=None):
    """Rows that ARE the quantised input: with frac_input = fi, h = a / 2^fi exactly (|a| <= 16383 unless a clamp is meant)."""
    import torch
    rows = (np.asarray(a, dtype=np.float64) / 2.0 ** fi).astype(np.float32)
    q = _qmodel(widths, np.asarray(block, dtype=np.int16), fi, fw, fb, fo)
    want = _check_q15(torch.from_numpy(rows).cuda(), rows, range(widths[0]), None, None, q, rows_per_group or rows.shape[0], "direct")
    return want


def test_halves_round_up_in_both_signs():
    """s = 1: an odd accumulator lies exactly on a half.  W = [[1, 0], [0, 1]], b = 0, Nw = 1, Na = 0, No = 0."""
    a = [[3, -3], [1, -1], [5, -5], [2, -2], [-7, 7]]
    want = _direct(a, (2, 2), [1, 0, 0, 1, 0, 0], 0, [1], [0], [0])
    assert want[1].tolist() == [[2, -1], [1, 0], [3, -2], [1, -1], [-3, 4]]      # 1.5 -> 2, -1.5 -> -1, 0.5 -> 1, -0.5 -> 0
    # the same on a wider shift: s = 4, acc = 8 (0.5 -> 1), -8 (-0.5 -> 0), 24 (1.5 -> 2), -24 (-1.5 -> -1)
    want = _direct([[8, -8], [24, -24]], (2, 2), [1, 0, 0, 1, 0, 0], 0, [4], [0], [0])
    assert want[1].tolist() == [[1, 0], [2, -1]]


def test_saturation_planted_at_each_layer_in_both_signs():
    """Identity layers (W = 2 I with s = 1) but for one of gain +-32767 / 2: its outputs pass +-32767 for |a| >= 3."""
    eye2 = [2, 0, 0, 2, 0, 0]
    a = [[5, 9], [1, 0], [100, 3], [0, 0]]
    for layer in range(3):
        for sign in (1, -1):
            g = 32767 * sign if sign > 0 else -32768
            block = []
            for l in range(3):
                block += [g, 0, 0, g, 0, 0] if l == layer else eye2
            want = _direct(a, (2, 2, 2, 2), block, 0, [1, 1, 1], [0, 0, 0], [0, 0, 0])
            sat = want[3].tolist()
            # a clip above always counts; one below counts in the last layer only (relu makes it 0 in a hidden one either way)
            expect = 4 if sign > 0 or layer == 2 else 0              # 5, 9, 100 and 3: |a| >= 3
            assert sat == [0] + [expect if l == layer else 0 for l in range(3)], (layer, sign, sat)
            top = 32767 if sign > 0 else (-32768 if layer == 2 else 0)
            assert want[1][0].tolist() == [top, top]


def test_input_clamps_at_both_ends_nonfinite_rows_and_argmax_ties():
    import torch
    from amcpy_amd import quantize as qz
    widths, fi = (2, 4), 9
    block = [1, 0, 0, 1, 1, 1, 0, 0, 5, 7, 7, 3]            # logits: round((a0, a1, a0 + a1, 0) / 1024) + (5, 7, 7, 3): P = 10, s = 10
    rows = np.array([[0.0, 0.0], [40.0, -40.0], [1e30, -1e30], [3.0e38, 3.0e38], [np.nan, 0.0], [0.0, np.inf], [-np.inf, 1.0],
                     [16383 / 512, -16384 / 512], [16383.5 / 512, -16384.5 / 512]], dtype=np.float32)
    q = _qmodel(widths, np.asarray(block, np.int16), fi, [1], [0], [0])
    want = _check_q15(torch.from_numpy(rows).cuda(), rows, (0, 1), None, None, q, 3, "clamps")
    assert want[0].tolist()[:2] == [1, 0] and want[0].tolist()[4:7] == [-1, -1, -1]           # a tie (7, 7): the first maximum
    assert want[1][0].tolist() == [5, 7, 7, 3] and want[1][1].tolist() == [21, -9, 7, 3]
    # rows 1, 2, 3 clamp both values (3.0e38 * 2^9 is +inf: it clamps); rows 4 ... 6 have no label and count nowhere; row 7 sits
    # on the two ends; row 8 lies half a step beyond them, where the clamp changes what rint would give
    assert want[3][0] == 2 + 2 + 2 + 0 + 2 and want[2][:, -1].tolist() == [0, 2, 1]
    assert not want[1][4:7].any()
    labels = qz.classify_q15(torch.from_numpy(rows).cuda(), q, cols=(0, 1), want=("labels",)).cpu().numpy()
    assert np.array_equal(labels, want[0])


def test_extreme_values_need_more_than_32_bits():
    """Width 32, every weight -32768 and every input at the clamp's end -16384 -- the most negative value the entry's input
    admits; the hidden layer's 32767s meet -32768s next -- and the mixed-sign extremes.  |acc| reaches 2^35, a bias shifted by 30 reaches 2^45."""
    widths = (32, 32, 32)
    lo = np.full(32 * 32 + 32, -32768, dtype=np.int64)
    hi = np.full(32 * 32 + 32, 32767, dtype=np.int64)
    mixed = np.where(np.arange(32 * 32 + 32) % 2 == 0, -32768, 32767)
    a = np.stack([np.full(32, -16384), np.full(32, 16383), np.where(np.arange(32) % 2 == 0, -16384, 16383),
                  np.where(np.arange(32) % 2 == 0, 16383, -16384), np.zeros(32, dtype=np.int64)])
    for first in (lo, hi, mixed):
        for second in (lo, hi, mixed):
            for fw, fb, fo in (([15, 15], [0, 0], [0, 0]), ([15, 0], [15, 0], [14, 13]), ([0, 15], [0, 15], [0, 0])):
                _direct(a, widths, np.concatenate([first, second]), 15, fw, fb, fo)
    # no weight at all: the bias alone, shifted by 30
    zero_w = np.concatenate([np.zeros(32 * 32, dtype=np.int64), np.full(32, -32768)])
    want = _direct(a, widths, np.concatenate([zero_w, zero_w]), 15, [15, 15], [0, 0], [0, 0])
    assert (want[1] == -32768).all() and want[3].tolist() == [0, 0, 0]          # exactly the end: no clip


def test_graph_capture_replayed_twice_gives_the_same_bits():
    import torch
    from amcpy_amd import _lib
    widths, n = (6, 26, 29, 30, 6), 4_099
    rows, cols, mean, scale, block, fi, fw, fb, fo = _q15_case(widths, n, 8, False)
    rows = np.ascontiguousarray(rows[:, :8])
    _, _, _, _, fblock = _float_case(widths, 1, 8)
    x = torch.from_numpy(rows).cuda()
    mean_d, scale_d = torch.from_numpy(mean).cuda(), torch.from_numpy(scale).cuda()
    p16, p32 = torch.from_numpy(block).cuda(), torch.from_numpy(fblock).cuda()
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    logits = torch.empty((n, 6), dtype=torch.int16, device="cuda")
    counts = torch.empty((1, 7), dtype=torch.int64, device="cuda")
    saturated = torch.empty(5, dtype=torch.int64, device="cuda")
    ranges = torch.empty((5, 2), dtype=torch.float32, device="cuda")
    skipped = torch.empty(1, dtype=torch.int64, device="cuda")
    outs = (labels, logits, counts, saturated, ranges, skipped)
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)     # noqa: E731
    cols_c, widths_c, fw_c, fb_c, fo_c = i32(cols), i32(widths), i32(fw), i32(fb), i32(fo)
    lib = _lib.load()

    def call():
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.amcx_mlp_classify_q15(x.data_ptr(), n, 8, 8, cols_c, 6, mean_d.data_ptr(), scale_d.data_ptr(), p16.data_ptr(),
                                             widths_c, 4, _lib.ACT_RELU, fi, fw_c, fb_c, fo_c, labels.data_ptr(), logits.data_ptr(), 6,
                                             n, counts.data_ptr(), saturated.data_ptr(), st))
        _lib.check(lib.amcx_mlp_range_f32(x.data_ptr(), n, 8, 8, cols_c, 6, mean_d.data_ptr(), scale_d.data_ptr(), p32.data_ptr(),
                                          widths_c, 4, _lib.ACT_RELU, ranges.data_ptr(), skipped.data_ptr(), st))

    call()
    torch.cuda.synchronize()
    eager = [t.clone() for t in outs]
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    for _ in range(2):
        for t in outs:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for t, e in zip(outs, eager):
            assert torch.equal(t, e)
    want = qr.classify_q15(rows, cols, mean, scale, widths, block, fi, fw, fb, fo, n)
    assert np.array_equal(eager[0].cpu().numpy(), want[0]) and np.array_equal(eager[3].cpu().numpy(), want[3])
    assert np.array_equal(eager[4].cpu().numpy(), qr.ranges32(rows, cols, mean, scale, widths, fblock, "relu")[0])


# ---- end to end --------------------------------------------------------------------------------------------------------------------
N_SNR, N_FRAMES, FRAME = 16, 64, 1024


@pytest.fixture(scope="module")
def quantize_run(tmp_path_factory):
    """`python -m amcpy_amd quantize --evaluate` in a fresh child process on a synthetic root of the default SNR grid (as
    test_classify_command_from_iq builds one), behind the `classify --from-iq` command, which extracts the features and writes
    the float table.  Both in the command's default mode, test: the scaler fitted on the rows the ranges are calibrated on, as
    the reference does.  Run once for the tests below: ``(cfg, quantize's stdout)``."""
    import scipy.io
    from amcpy_amd import synth
    from amcpy_amd.classifier import MlpModel
    from amcpy_amd.config import Config, Paths, SignalConfig
    root = tmp_path_factory.mktemp("quantize_root")
    cfg = Config(paths=Paths(root=root), signals=SignalConfig(num_frames=N_FRAMES, frame_size=FRAME))
    cfg.paths.ensure_dirs()
    blocks = synth.host_frames(synth.MODS6, N_SNR, N_FRAMES, FRAME)
    scipy.io.savemat(str(cfg.paths.mat_data / cfg.paths.mat_filename), {cfg.signals.mat_info[m]: blocks[m] for m in synth.MODS6})
    z = np.load(GOLDEN / "classifier_synth6.npz", allow_pickle=False)
    MlpModel.from_state_dict(state_dict_of(z), str(z["activation"])).save_npz(root / "synth6.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["PYTHONPATH"] = str(REPO) + os.pathsep + os.environ.get("PYTHONPATH", "")
    common = ["--root", str(root), "--model", str(root / "synth6.npz"), "--num-frames", str(N_FRAMES), "--frame-size", str(FRAME)]
    for cmd in ([sys.executable, "-m", "amcpy_amd", "classify", "--from-iq", *common],
                [sys.executable, "-m", "amcpy_amd", "quantize", "--evaluate", *common]):
        r = subprocess.run(cmd, env=env, cwd=str(root), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print("\n" + r.stdout)
    return cfg, r.stdout


def test_quantize_command_evaluates_beside_the_float_classifier(quantize_run):
    """arm-data/{id}_q15.mat and figures/{id}_q15_figure_data.mat: `acc_float` is the `classify` command's table; `acc`,
    `agreement` and `saturated` are what the int64 restatement gives for the exported integers, formats and scaler on the
    feature files.  The agreement between the float and the Q15 labels is printed: a reported figure, not a gate."""
    import scipy.io
    from amcpy_amd import synth
    cfg, stdout = quantize_run
    assert "Layer 4 outputs: Q" in stdout and "Input: Q" in stdout
    table = scipy.io.loadmat(str(cfg.paths.figures / "synth6_figure_data.mat"))["acc"]
    got = scipy.io.loadmat(str(cfg.paths.figures / "synth6_q15_figure_data.mat"))
    assert np.array_equal(got["acc_float"], table)
    assert got["acc"].shape == got["agreement"].shape == (6, N_SNR) and got["saturated"].reshape(-1).shape == (5,)
    ex = scipy.io.loadmat(str(cfg.paths.arm_data / "synth6_q15.mat"))
    widths = ex["widths"].reshape(-1).tolist()
    assert ex["weights"].dtype == ex["biases"].dtype == np.int16 and ex["weights"].size + ex["biases"].size == 2051
    assert ex["mean"].size == ex["scale"].size == 6 and widths == [6, 26, 29, 30, 6]
    # the exported integers, run by the int64 restatement over the feature files
    w, b, at_w, at_b, block = ex["weights"].reshape(-1), ex["biases"].reshape(-1), 0, 0, []
    for l in range(4):
        block += [w[at_w:at_w + widths[l] * widths[l + 1]], b[at_b:at_b + widths[l + 1]]]
        at_w, at_b = at_w + widths[l] * widths[l + 1], at_b + widths[l + 1]
    feats = np.stack([scipy.io.loadmat(str(cfg.paths.calculated_features / f"{m}_features.mat"))[cfg.signals.mat_info[m]]
                      for m in synth.MODS6]).astype(np.float32)
    fracs = [ex[k].reshape(-1).tolist() for k in ("frac_weights", "frac_biases", "frac_outputs")]
    labels, _, _, saturated = qr.classify_q15(feats.reshape(-1, 18), cfg.features.used, ex["mean"].reshape(-1), ex["scale"].reshape(-1),
                                              widths, np.concatenate(block), int(ex["frac_input"].reshape(-1)[0]), *fracs)
    assert np.array_equal(saturated, got["saturated"].reshape(-1))
    truth = np.repeat(np.asarray(cfg.signals.labels)[:6], N_SNR * N_FRAMES)
    assert np.array_equal((labels == truth).reshape(6, N_SNR, N_FRAMES).mean(axis=2), got["acc"])
    print(f"\nsynth6 on {6 * N_SNR * N_FRAMES} rows: Q15 and float labels agree on {got['agreement'].mean():.4%}; accuracy "
          f"{got['acc'].mean():.4f} (Q15) / {got['acc_float'].mean():.4f} (float); saturated {got['saturated'].reshape(-1).tolist()}")


def test_quantize_command_saturates_nowhere_on_the_calibration_rows(quantize_run):
    """`saturated` is all zero on the rows the formats were calibrated on.  The trained synth6 network's pre-activation values
    reach 106 in layer 3 and 362 in layer 4 on this root, past the table's last format: exported as it is (`--no-normalize`) 66
    and 1061 of those outputs clip.  The command's default scales such layers by exact powers of two instead
    (`amcpy_amd.quantize.normalize_block`; `layer_shifts` in the exported file says by how much), and nothing clips."""
    import scipy.io
    cfg, stdout = quantize_run
    got = scipy.io.loadmat(str(cfg.paths.figures / "synth6_q15_figure_data.mat"))
    shifts = scipy.io.loadmat(str(cfg.paths.arm_data / "synth6_q15.mat"))["layer_shifts"].reshape(-1).tolist()
    print(f"\nsaturated on the calibration rows: {got['saturated'].reshape(-1).tolist()}; layer shifts {shifts}")
    assert len(shifts) == 4 and shifts == sorted(shifts) and shifts[-1] > 0 and "layers scaled by 2^-k" in stdout
    assert not got["saturated"].any()


def test_reference_layout_from_a_checkpoint_writes_the_references_file(quantize_run):
    """`run_quantization(layout="reference")` on the same root, from a checkpoint file as the reference's training writes one:
    arm-data/w_and_b.mat holds the `Linear` layers as stored (no fold), quantised in the formats their own ranges choose, in
    the reference's transposed order; the output formats come from the device's ranges of the activation-free chain."""
    import scipy.io
    import torch
    from amcpy_amd import quantize as qz
    cfg, _ = quantize_run
    z = np.load(GOLDEN / "classifier_synth6.npz", allow_pickle=False)
    sd = state_dict_of(z)
    path = cfg.paths.root / "model-synth6ref.pt"
    torch.save({"model_state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, "model_id": "synth6ref"}, str(path))
    q = qz.run_quantization(cfg, str(path), layout="reference", verbose=False)
    assert q.layout == "reference" and q.widths == (6, 26, 29, 30, 6)
    mat = scipy.io.loadmat(str(cfg.paths.arm_data / "w_and_b.mat"))
    save, info = q.reference_export()
    assert mat["weights"].dtype == np.int16 and mat["weights"].shape == (1, save["weights"].size)
    assert np.array_equal(mat["weights"].reshape(-1), save["weights"]) and np.array_equal(mat["biases"].reshape(-1), save["biases"])
    w0 = np.asarray(sd["layers.0.weight"], dtype=np.float32)
    assert q.frac_weights[0] == qz.find_q_format(w0.min(), w0.max())
    assert np.array_equal(save["weights"][:w0.size], qz.quantize_array(w0, q.frac_weights[0]).T.reshape(-1))
    assert all(info[f"Layer {l} outputs"] == qz.q_name(qz.find_q_format(0.0, q.ranges[l][1])) for l in range(1, 5))
    with pytest.raises(ValueError, match="folded"):
        qz.run_quantization(cfg, str(path), layout="reference", evaluate=True, verbose=False)


def test_agreement_with_the_float_labels_on_the_reference_fixture():
    """classifier_ref_relu.npz: calibrate, fold, quantise and run both networks over its 8192 rows.  Nothing saturates on the
    rows the model was calibrated on; the agreement is printed (a reported figure)."""
    import torch
    from amcpy_amd import quantize as qz
    from amcpy_amd.classifier import MlpModel, classify
    z = np.load(GOLDEN / "classifier_ref_relu.npz", allow_pickle=False)
    model = MlpModel.from_state_dict(state_dict_of(z), "relu")
    x = torch.from_numpy(z["x"]).cuda()
    ranges, skipped = qz.calibrate(x, model, cols=range(6))
    q = qz.QuantizedMlp.from_model(model, ranges)
    labels, saturated = qz.classify_q15(x, q, cols=range(6), want=("labels", "saturated"))
    float_labels = classify(x, model, cols=range(6))
    assert skipped == 0 and not saturated.cpu().numpy().any()
    want = qr.classify_q15(z["x"], range(6), None, None, q.widths, q.params, q.frac_input, q.frac_weights, q.frac_biases, q.frac_outputs)
    assert np.array_equal(labels.cpu().numpy(), want[0])
    # the table of evaluate_by_snr_q15 is those labels counted: 2 "modulations" x 4 "SNRs" x 1024 rows
    acc, confusion, sat = qz.evaluate_by_snr_q15(x.reshape(2, 4, 1024, 6), q, cols=range(6), mean=None, scale=None, labels=(3, 0))
    lab = want[0].reshape(2, 4, 1024)
    assert np.array_equal(acc, np.stack([(lab[0] == 3).mean(axis=1), (lab[1] == 0).mean(axis=1)])) and not sat.any()
    assert confusion.sum() == 8192 and np.array_equal(confusion[3][:6], np.bincount(lab[0].reshape(-1), minlength=6))
    print(f"\nclassifier_ref_relu on 8192 rows: Q15 and float labels agree on {(labels == float_labels).double().mean().item():.4%}")


def test_leading_dimensions_and_groups_shape_both_classifiers_alike():
    """classify and classify_q15 on a (2, 3, 5, C) view with padding -- one that flattens to a strided view and one that has to be
    copied -- with want=("labels", "counts"): labels (2, 3, 5), counts over the rows axis (2, 3, n_classes + 1), and with
    rows_per_group=15 (2, n_classes + 1).  Thirty rows of a fixture network each, one of them with a NaN (label -1, the last bin):
    the float labels are argmax(p64) (every row's top-two margin is far beyond 8 x ref32_err, asserted), the integer ones the
    int64 restatement's (the fixture whose first thirty rows get four different labels), compared with ==."""
    import torch
    from amcpy_amd import quantize as qz
    from amcpy_amd.classifier import MlpModel, classify
    zf = np.load(GOLDEN / "classifier_ref_odd.npz", allow_pickle=False)
    model = MlpModel.from_state_dict(state_dict_of(zf), str(zf["activation"]))
    s = np.sort(zf["p64"][:30], axis=1)
    assert (s[:, -1] - s[:, -2]).min() > 8 * float(zf["ref32_err"])
    xf, want_f = zf["x"][:30].copy(), zf["p64"][:30].argmax(1)
    xf[7, 0], want_f[7] = np.nan, -1
    zq = np.load(GOLDEN / "quantize_ref_default.npz", allow_pickle=False)
    q = qz.QuantizedMlp.from_state_dict(state_dict_of(zq), zq["ranges"], layout="reference")
    xq = zq["x"][:30].copy()
    xq[7, 0] = np.nan
    want_q = {g: qr.classify_q15(xq, range(q.n_inputs), None, None, q.widths, q.params, q.frac_input, q.frac_weights,
                                 q.frac_biases, q.frac_outputs, g) for g in (5, 15)}
    assert len(set(want_q[5][0].tolist())) >= 4 and want_q[5][0][7] == -1

    def counts_of(labels, n_cls, g):
        return np.stack([np.bincount(np.where(r < 0, n_cls, r), minlength=n_cls + 1) for r in labels.reshape(-1, g)])

    def views(x):
        n = x.shape[1]
        strided = torch.full((2, 3, 5, n + 7), float("nan"), dtype=torch.float32, device="cuda")[..., 2:2 + n]
        copied = torch.full((2, 3, 6, n + 7), float("nan"), dtype=torch.float32, device="cuda")[:, :, 1:, 2:2 + n]
        for v in (strided, copied):
            v.copy_(torch.from_numpy(x.reshape(2, 3, 5, n)))
        assert strided.reshape(-1, n).data_ptr() == strided.data_ptr() and copied.reshape(-1, n).data_ptr() != copied.data_ptr()
        return strided, copied

    for run, x, n_cls, want_labels, want_counts in (
            (lambda f, **kw: classify(f, model, cols=range(model.n_inputs), want=("labels", "counts"), **kw), xf, model.n_classes,
             want_f, {g: counts_of(want_f, model.n_classes, g) for g in (5, 15)}),
            (lambda f, **kw: qz.classify_q15(f, q, cols=range(q.n_inputs), want=("labels", "counts"), **kw), xq, q.n_classes,
             want_q[5][0], {g: want_q[g][2] for g in (5, 15)})):
        for feats in views(x):
            labels, counts = run(feats)
            assert labels.shape == (2, 3, 5) and labels.dtype == torch.int32
            assert counts.shape == (2, 3, n_cls + 1) and counts.dtype == torch.int64
            assert np.array_equal(labels.cpu().numpy().reshape(-1), want_labels)
            assert np.array_equal(counts.cpu().numpy().reshape(6, n_cls + 1), want_counts[5])
            labels15, counts15 = run(feats, rows_per_group=15)
            assert labels15.shape == (2, 3, 5) and counts15.shape == (2, n_cls + 1)
            assert torch.equal(labels15, labels) and np.array_equal(counts15.cpu().numpy(), want_counts[15])


def test_votes_of_many_groups_in_a_wave_and_a_lone_last_row():
    """mlp_vote, the histogram both classifiers call: 513 rows in groups of 19 are 27 groups, three or four of them inside every
    wave slot's 64 rows, group boundaries at no multiple of 64, and row 512 alone in the second tile.  Six rows carry a NaN (the
    first, the two either side of a group boundary, the two either side of the slot boundary at 256, one more), so the extra bin
    is used.  For classify and for classify_q15, counts[g] == numpy.bincount of that classifier's OWN returned labels over rows
    19 g ... 19 g + 18, label -1 in bin n_classes: integers, compared with ==."""
    import torch
    from amcpy_amd import quantize as qz
    from amcpy_amd.classifier import MlpModel, classify
    n_rows, per_group, bad = 513, 19, (0, 18, 19, 255, 256, 300)
    z = np.load(GOLDEN / "classifier_ref_relu.npz", allow_pickle=False)
    model = MlpModel.from_state_dict(state_dict_of(z), "relu")
    x = torch.from_numpy(z["x"][:n_rows].copy()).cuda()
    ranges, _ = qz.calibrate(x, model, cols=range(6))
    q = qz.QuantizedMlp.from_model(model, ranges)
    for k, r in enumerate(bad):
        x[r, k % 6] = float("nan")
    n_cls = model.n_classes
    for name, run in (("classify", lambda: classify(x, model, cols=range(6), rows_per_group=per_group, want=("labels", "counts"))),
                      ("classify_q15", lambda: qz.classify_q15(x, q, cols=range(6), rows_per_group=per_group, want=("labels", "counts")))):
        labels, counts = run()
        lab, got = labels.cpu().numpy(), counts.cpu().numpy()
        assert lab.shape == (n_rows,) and got.shape == (n_rows // per_group, n_cls + 1), name
        assert sorted(np.flatnonzero(lab < 0).tolist()) == list(bad) and len(set(lab[lab >= 0].tolist())) >= 3, name
        want = np.stack([np.bincount(np.where(g < 0, n_cls, g), minlength=n_cls + 1) for g in lab.reshape(-1, per_group)])
        assert np.array_equal(got, want), name
        assert got.sum() == n_rows and got[:, n_cls].sum() == len(bad), name
