"""Fixed-point deployment on the host (amcpy_amd/quantize.py, include/amcx.h ABI 16): the Q-format table and the export
against the reference's own ``quantize`` (tests/golden/quantize_ref_*.npz, written by tests/golden/make_quantize_fixtures.py),
the ABI, the kernels' resources, the two entries' refusals in the order the header states, and the int64 restatement's
saturation counts on calibrated rows.  Needs no GPU."""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib
from amcpy_amd import quantize as qz
from amcpy_amd.classifier import MlpModel
from tests import quantize_ref as qr
from tests.classifier_host_ref import state_dict_of
from tests.stream_inputs import aligned as _aligned

REPO = Path(__file__).resolve().parents[1]
GOLD = REPO / "tests" / "golden"
E, OK = _lib.EINVAL, _lib.OK
NAMES = ("default", "spread", "ties")
PAST_2_58 = ((1 << 40, 1 << 40), (1 << 2, (1 << 56) + 1))


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def _fixture(name):
    return np.load(GOLD / f"quantize_ref_{name}.npz", allow_pickle=False)


def _info(z):
    return dict(zip((str(k) for k in z["info_keys"]), (str(v) for v in z["info_values"])))


# ---- the table ---------------------------------------------------------------------------------------------------------------
def test_the_table_is_the_references():
    assert [qz.q_name(n) for _, n in qz.Q_FORMATS] == ["Q0.15", "Q1.14", "Q2.13", "Q3.12", "Q4.11", "Q5.10", "Q6.9"]
    assert qz.q_range(15) == (-0.5, 0.5 - 2.0 ** -15) and qz.q_range(9) == (-32.0, 32.0 - 2.0 ** -9)
    for m, n in qz.Q_FORMATS:
        lo, hi = qz.q_range(n)
        assert lo == -(2.0 ** (m - 1)) and hi == 2.0 ** (m - 1) - 2.0 ** -n
        # both ends are held by the format itself, a step beyond either end by the next one (or the fallback)
        assert qz.find_q_format(lo, hi) == n
        wider = n - 1 if n > 9 else 9
        assert qz.find_q_format(lo - 2.0 ** -n, hi) == wider and qz.find_q_format(lo, hi + 2.0 ** -n) == wider
    assert qz.find_q_format(0.0, 0.0) == 15 and qz.find_q_format(-100.0, 5.0) == 9 and qz.find_q_format(0.0, 1e9) == 9


def test_quantize_array_rounds_half_to_even_and_clamps_at_both_ends():
    for _, n in qz.Q_FORMATS:
        lo, hi = qz.q_range(n)
        step = 2.0 ** -n
        a = np.array([lo, hi, lo - 1.0, hi + 1.0, 0.5 * step, 1.5 * step, 2.5 * step, -0.5 * step, -1.5 * step, -2.5 * step,
                      0.49 * step, 0.51 * step, -1e9, 1e9], dtype=np.float32)
        got = qz.quantize_array(a, n)
        assert got.dtype == np.int16
        assert got.tolist() == [-16384, 16383, -16384, 16383, 0, 2, 2, 0, -2, -2, 0, 1, -16384, 16383], n
    every = qz.quantize_array(np.linspace(-40, 40, 100001), 9)
    assert every.min() == -16384 and every.max() == 16383


# ---- against the reference's own stage -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_export_equals_the_references_bit_for_bit(name, tmp_path):
    import scipy.io
    z = _fixture(name)
    sd = state_dict_of(z)
    q = qz.QuantizedMlp.from_state_dict(sd, z["ranges"], layout="reference")
    save, info = q.reference_export()
    assert set(save) == {"weights", "biases"}
    for key in save:
        assert save[key].dtype == np.int16 and save[key].ndim == 1
        assert np.array_equal(save[key], z[key]), key
    assert info == _info(z)
    # the transposed order: the first in * out values are W_q.T of the first Linear
    w0 = q.layers()[0][0]
    assert np.array_equal(save["weights"][:w0.size], w0.T.reshape(-1))
    assert int(np.abs(save["weights"].astype(np.int32)).max()) <= 16384 and int(save["weights"].max()) <= 16383
    # the file, as loadmat sees it
    q.save_reference_mat(tmp_path / "w_and_b.mat")
    mat = {k: v for k, v in scipy.io.loadmat(str(tmp_path / "w_and_b.mat")).items() if not k.startswith("__")}
    assert sorted(mat) == [str(k) for k in z["mat_names"]]
    for k, shape, dtype in zip(z["mat_names"], z["mat_shapes"], z["mat_dtypes"]):
        assert mat[str(k)].shape == tuple(shape) == (1, z[str(k)].size) and str(mat[str(k)].dtype) == str(dtype) == "int16"
        assert np.array_equal(mat[str(k)].reshape(-1), z[str(k)])


def test_the_fixtures_cover_every_format_the_fallback_and_the_ties():
    seen = set()
    for name in NAMES:
        seen |= set(_info(_fixture(name)).values())
    assert seen == {"Q0.15", "Q1.14", "Q2.13", "Q3.12", "Q4.11", "Q5.10", "Q6.9"}
    z = _fixture("spread")
    sd = state_dict_of(z)
    assert np.abs(sd["2.bias"]).max() > 32 and np.abs(sd["4.weight"]).max() > 32                 # the fallback's clamp is hit
    assert z["biases"].min() == -16384 and z["biases"].max() == 16383 and z["weights"].min() == -16384 and z["weights"].max() == 16383
    t = state_dict_of(_fixture("ties"))
    halves = t["0.weight"].astype(np.float64) * 2.0 ** 15
    assert np.sum(halves - np.floor(halves) == 0.5) >= 28 and t["0.weight"].min() == -0.5 and t["0.weight"].max() == np.float32(0.5 - 2.0 ** -15)


def test_folded_layout_takes_the_models_block_and_the_real_ranges(tmp_path):
    import scipy.io
    z = _fixture("default")
    model = MlpModel.from_state_dict(state_dict_of(z), "relu", "m1")
    ranges, skipped = qr.ranges32(z["x"], range(6), None, None, model.widths, model.params, "relu")
    assert skipped == 0
    q = qz.QuantizedMlp.from_model(model, ranges)
    assert q.layout == "folded" and q.widths == model.widths and q.params.dtype == np.int16 and q.params.size == model.params.size
    at = 0
    for l, (w, b) in enumerate(qr.layers_of(model.widths, model.params)):
        assert q.frac_weights[l] == qz.find_q_format(w.min(), w.max()) and q.frac_biases[l] == qz.find_q_format(b.min(), b.max())
        last = l + 1 == model.n_linear
        assert q.frac_outputs[l] == qz.find_q_format(ranges[l + 1][0] if last else 0.0, ranges[l + 1][1])
        assert np.array_equal(q.params[at:at + w.size], qz.quantize_array(w, q.frac_weights[l]).reshape(-1))
        at += w.size + b.size
    q.save_mat(tmp_path / "m1_q15.mat", np.arange(6.0), np.arange(6.0) + 1)
    mat = scipy.io.loadmat(str(tmp_path / "m1_q15.mat"))
    assert {"weights", "biases", "widths", "frac_weights", "frac_biases", "frac_outputs", "frac_input", "mean", "scale"} <= set(mat)
    assert mat["weights"].dtype == np.int16 and mat["widths"].reshape(-1).tolist() == list(model.widths)
    with pytest.raises(ValueError, match="tanh"):
        qz.QuantizedMlp.from_model(MlpModel.from_state_dict(state_dict_of(z), "tanh"), ranges)
    with pytest.raises(ValueError, match="sigmoid"):
        qz.QuantizedMlp.from_state_dict(state_dict_of(z), ranges, activation="sigmoid")


@pytest.mark.parametrize("name", ("default", "ties"))
def test_a_model_calibrated_on_some_rows_does_not_saturate_on_them(name):
    """The int64 restatement, for the networks every one of whose ranges a format of the table holds: the table's factor 2 of
    headroom covers what the rounding of weights and activations adds.  (`spread` goes beyond +-32 on purpose: below.)"""
    z = _fixture(name)
    model = MlpModel.from_state_dict(state_dict_of(z), "relu")
    cols = range(model.n_inputs)
    ranges, _ = qr.ranges32(z["x"], cols, None, None, model.widths, model.params, "relu")
    q = qz.QuantizedMlp.from_model(model, ranges)
    labels, logits, _, saturated = qr.classify_q15(z["x"], cols, None, None, q.widths, q.params, q.frac_input, q.frac_weights,
                                                   q.frac_biases, q.frac_outputs)
    assert saturated.tolist() == [0] * (model.n_linear + 1)
    assert labels.min() >= 0 and logits.shape == (z["x"].shape[0], model.n_classes)


def test_where_the_fallback_clamps_the_restatement_reports_the_saturation():
    """`spread`, exported as it is (normalize=False): weights, biases and outputs beyond Q6.9's +-32 are clamped by the export,
    and the counts say where."""
    z = _fixture("spread")
    model = MlpModel.from_state_dict(state_dict_of(z), "relu")
    ranges, _ = qr.ranges32(z["x"], range(5), None, None, model.widths, model.params, "relu")
    assert ranges[2:, 1].min() > 32
    q = qz.QuantizedMlp.from_model(model, ranges, normalize=False)
    assert q.layer_shifts == (0, 0, 0)
    saturated = qr.classify_q15(z["x"], range(5), None, None, q.widths, q.params, q.frac_input, q.frac_weights, q.frac_biases,
                                q.frac_outputs)[3]
    assert saturated[0] == 0 and saturated[2:].sum() > 0


def test_normalisation_scales_by_exact_powers_of_two_and_only_where_the_table_ends():
    """A network whose layers pass +-32 (the `default` fixture's, layers 2 ... 4 made 8, 4 and 16 times larger): every layer's
    range lands inside Q6.9, the scaled float32 network's pre-activation values are the original's times 2^-shifts[l] bit for
    bit (so its labels are the original's), and the integer network calibrated that way saturates nowhere on those rows --
    while the same network exported as it is clips.  Where every range fits (`default`) nothing is touched."""
    for name in ("default",):
        z = _fixture(name)
        model = MlpModel.from_state_dict(state_dict_of(z), "relu")
        ranges, _ = qr.ranges32(z["x"], range(model.n_inputs), None, None, model.widths, model.params, "relu")
        block, scaled, shifts = qz.normalize_block(model.widths, model.params, ranges)
        assert shifts == (0,) * model.n_linear and np.array_equal(block, model.params) and np.array_equal(scaled, ranges)
        assert np.array_equal(qz.QuantizedMlp.from_model(model, ranges).params, qz.QuantizedMlp.from_model(model, ranges, False).params)
    z = _fixture("default")
    base = MlpModel.from_state_dict(state_dict_of(z), "relu")
    parts = []
    for (w, b), gain in zip(qr.layers_of(base.widths, base.params), (1.0, 8.0, 4.0, 16.0)):
        parts += [(w * np.float32(gain)).reshape(-1), b * np.float32(gain)]
    model = MlpModel(base.widths, "relu", np.concatenate(parts))
    cols = range(6)
    ranges, _ = qr.ranges32(z["x"], cols, None, None, model.widths, model.params, "relu")
    assert ranges[2:, 1].min() > 64                                  # beyond even the int16 headroom of Q6.9
    block, scaled, shifts = qz.normalize_block(model.widths, model.params, ranges)
    assert shifts[0] == 0 and list(shifts) == sorted(shifts) and shifts[-1] >= 6
    lo, hi = qz.q_range(9)
    assert (scaled[1:-1, 1] <= hi).all() and lo <= scaled[-1, 0] and scaled[-1, 1] <= hi
    again, _ = qr.ranges32(z["x"], cols, None, None, model.widths, block, "relu")
    assert np.array_equal(again, scaled)                              # powers of two: the same sums, scaled exactly
    pre, pre_scaled = (qr.forward32(z["x"], model.widths, blk, "relu") for blk in (model.params, block))
    for l in range(4):
        assert np.array_equal(pre_scaled[l], pre[l] * np.float32(2.0 ** -shifts[l]))
    q = qz.QuantizedMlp.from_model(model, ranges)
    assert q.layer_shifts == shifts and np.array_equal(q.ranges, scaled)
    run = lambda m: qr.classify_q15(z["x"], cols, None, None, m.widths, m.params, m.frac_input, m.frac_weights, m.frac_biases,      # noqa: E731
                                    m.frac_outputs)
    labels, _, _, saturated = run(q)
    assert saturated.tolist() == [0, 0, 0, 0, 0]
    assert (labels == pre[-1].argmax(axis=1)).mean() > 0.99
    assert run(qz.QuantizedMlp.from_model(model, ranges, normalize=False))[3][2:].sum() > 0


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("amcx_mlp_range_f32", "amcx_mlp_classify_q15", "amcx_mlp_q15_params_shorts", "amcx_kernel_name_mlp_q15")


def test_abi_16_in_header_binding_and_library():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 16 and lib.amcx_abi_version() == 16
    header = (REPO / "include" / "amcx.h").read_text()
    assert "#define AMCX_ABI_VERSION 16" in header and "#define AMCX_ACT_NONE 3" in header and _lib.ACT_NONE == 3
    lines = [header.index(f"#define AMCX_ABI_VERSION {v}") for v in (16, 15, 14, 13, 12, 11, 10)]
    assert lines == sorted(lines)                                               # the newest first
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header) and re.search(rf" T {name}$", exported, re.M), name
    w = _i32(6, 26, 29, 30, 6)
    assert lib.amcx_mlp_q15_params_shorts(w, 4) == lib.amcx_mlp_params_floats(w, 4) == 2051
    assert lib.amcx_mlp_q15_params_shorts(_i32(6, 33, 6), 2) == -1
    assert [_lib.kernel_name_mlp_q15(i) for i in range(3)] == ["amcx_mlp_q15_kernel", "amcx_mlp_range_kernel", "amcx_mlp_range_init_kernel"]
    with pytest.raises(ValueError):
        _lib.kernel_name_mlp_q15(3)


def test_both_kernels_are_in_the_resource_table_without_spills_and_every_older_kernel_kept_its_bytes():
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    for name in ("amcx_mlp_q15_kernel", "amcx_mlp_range_kernel", "amcx_mlp_range_init_kernel"):
        assert table[name]["spill"] == 0 and table[name]["scratch"] == 0, name
    listing = (REPO / "profiles" / "r25_q15_codeobj_kernels.txt").read_text()
    assert "DIFFERENT" not in listing and "ONLY IN A" not in listing and "90 kernels / device functions identical" in listing
    assert sorted(re.findall(r"ONLY IN B\s+amcx::(\w+)", listing)) == ["amcx_mlp_q15_kernel", "amcx_mlp_range_init_kernel", "amcx_mlp_range_kernel"]


def test_sharing_the_network_routines_moved_the_three_inference_kernels_alone():
    """amcx_mlp_shape.h (parameter staging, row load, the float32 sums, the votes and the scaler's two roundings, which the float
    classifier, the range calibration and the integer network now all call): the parent commit's library against the tree's, per
    kernel -- nothing on one side only, nothing different but those three, which keep their registers and spill nothing; and the
    copies are gone from the two kernel headers."""
    three = ["amcx_mlp_classify_kernel", "amcx_mlp_q15_kernel", "amcx_mlp_range_kernel"]
    listing = (REPO / "profiles" / "r31_mlp_shared_codeobj_kernels.txt").read_text()
    assert "ONLY IN A" not in listing and "ONLY IN B" not in listing
    assert "98 kernels / device functions identical" in listing
    assert sorted(re.findall(r"^DIFFERENT\s+amcx::(\S+)\s*$", listing, re.M)) == three and listing.count("DIFFERENT") == 3
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    for name, vgpr in zip(three, (182, 197, 195)):                              # the parent's counts
        assert table[name] == {"vgpr": vgpr, "spill": 0, "scratch": 0}, name
    csrc = REPO / "amcpy_amd" / "csrc"
    shared = (csrc / "amcx_mlp_shape.h").read_text()
    assert "__global__" not in shared
    assert re.findall(r'#include\s+(\S+)', shared) == ["<hip/hip_runtime.h>"]
    chain = re.compile(r"__builtin_fmaf\(w8\[k\]")
    assert chain.search(shared) and "__ballot(mine" in shared
    for routine in ("mlp_stage_params(", "mlp_standardise(", "mlp_load_rows(", "mlp_finite(", "mlp_dense_f32(", "mlp_vote("):
        assert len(re.findall(rf"__device__ inline \w+ {re.escape(routine)}", shared)) == 1, routine
    for header in ("amcx_mlp_kernel.h", "amcx_mlp_q15_kernel.h"):
        text = (csrc / header).read_text()
        for call in ("mlp_stage_params(", "mlp_load_rows(", "mlp_dense_f32(", "mlp_vote("):
            assert call in text, (header, call)
        assert "__ballot(mine" not in text and not chain.search(text), header
        assert "/ scale[" not in text and "__syncthreads" not in text, header       # the scaler and the staging barriers
    assert (csrc / "amcx_post_kernels.h").read_text().count("mlp_standardise(") == 2
    for p in csrc.rglob("*"):
        if p.is_file() and p.suffix in (".h", ".hip", ".py", ".json"):
            text = p.read_text(errors="replace")
            for old in ("q15_load_rows", "q15_dense_f32", "q15_stage_params", "q15_finite"):
                assert old not in text, (p, old)


# ---- the refusals, in the header's order ---------------------------------------------------------------------------------------
SHARED_LIMITS = (dict(n_rows=-1), dict(n_cols=0), dict(n_cols=33, stride=33), dict(stride=17), dict(stride=0), dict(stride=-18),
                 dict(cols=None), dict(widths=None), dict(widths=_i32(6, 0, 29, 30, 6)), dict(widths=_i32(6, 33, 29, 30, 6)),
                 dict(n_linear=0), dict(widths=_i32(*[6] * 8), n_linear=7), dict(n_sel=5, cols=_i32(2, 4, 6, 8, 12)),
                 dict(cols=_i32(2, 4, 6, 8, 12, 18)), dict(cols=_i32(-1, 4, 6, 8, 12, 14)))


def test_range_refusals_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_mlp_range_f32
    keep, p = _aligned()
    nul = dict(x=None, mean=None, scale=None, params=None, ranges=None, skipped=None)

    def call(**kw):
        a = {**dict(x=p, n_rows=1000, stride=18, n_cols=18, cols=_i32(2, 4, 6, 8, 12, 14), n_sel=6, mean=p, scale=p, params=p,
                    widths=_i32(6, 26, 29, 30, 6), n_linear=4, act=_lib.ACT_RELU, ranges=p, skipped=p), **kw}
        return f(a["x"], a["n_rows"], a["stride"], a["n_cols"], a["cols"], a["n_sel"], a["mean"], a["scale"], a["params"], a["widths"],
                 a["n_linear"], a["act"], a["ranges"], a["skipped"], None)
    # 1. the limits, also where the call would otherwise be the no-op; tanh and sigmoid are no choice here
    for kw in SHARED_LIMITS + (dict(mean=None, scale=p), dict(mean=p, scale=None), dict(act=_lib.ACT_TANH), dict(act=_lib.ACT_SIGMOID),
                               dict(act=4), dict(act=-1)):
        assert call(**kw) == E and call(**{"n_rows": 0, **nul, **kw}) == E, kw
    for R, s in PAST_2_58:
        assert call(n_rows=R, stride=s) == E, (R, s)
    # 2. nothing to do: no pointer is looked at
    assert call(n_rows=0, **nul) == OK and call(n_rows=0, act=_lib.ACT_NONE, stride=1 << 60, **nul) == OK
    # 3. null pointers and alignment, every pointer of the entry
    for kw in (dict(x=None), dict(params=None), dict(ranges=None), dict(skipped=None), dict(x=p + 2), dict(mean=p + 4), dict(scale=p + 4),
               dict(params=p + 2), dict(ranges=p + 2), dict(skipped=p + 4)):
        assert call(**kw) == E and call(act=_lib.ACT_NONE, **kw) == E, kw
    del keep


def test_q15_refusals_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_mlp_classify_q15
    keep, p = _aligned()
    nul = dict(x=None, mean=None, scale=None, params=None, labels=None, logits=None, counts=None, saturated=None)

    def call(**kw):
        a = {**dict(x=p, n_rows=1000, stride=18, n_cols=18, cols=_i32(2, 4, 6, 8, 12, 14), n_sel=6, mean=p, scale=p, params=p,
                    widths=_i32(6, 26, 29, 30, 6), n_linear=4, act=_lib.ACT_RELU, fi=12, fw=_i32(13, 14, 14, 14), fb=_i32(14, 14, 14, 15),
                    fo=_i32(10, 10, 10, 11), labels=p, logits=p, lstride=6, rpg=100, counts=p, saturated=p), **kw}
        return f(a["x"], a["n_rows"], a["stride"], a["n_cols"], a["cols"], a["n_sel"], a["mean"], a["scale"], a["params"], a["widths"],
                 a["n_linear"], a["act"], a["fi"], a["fw"], a["fb"], a["fo"], a["labels"], a["logits"], a["lstride"], a["rpg"],
                 a["counts"], a["saturated"], None)
    assert call(n_rows=0, **nul) == OK
    # 1. the limits, also where the call would otherwise be the no-op (a stride or a group is judged where its pointer is given):
    #    relu only; every format 0 ... 15; P >= Nb and P > No
    formats = (dict(fi=-1), dict(fi=16), dict(fw=None), dict(fb=None), dict(fo=None), dict(fw=_i32(16, 14, 14, 14)),
               dict(fw=_i32(13, 14, 14, -1)), dict(fb=_i32(14, 16, 14, 15)), dict(fo=_i32(10, 10, 10, 16)), dict(fo=_i32(10, 10, -1, 11)),
               dict(fi=0, fw=_i32(0, 14, 14, 14), fb=_i32(1, 14, 14, 15), fo=_i32(0, 10, 10, 11)),       # P = 0 < Nb = 1
               dict(fi=0, fw=_i32(5, 14, 14, 14), fb=_i32(5, 14, 14, 15), fo=_i32(5, 10, 10, 11)),       # P = 5 = No: no shift
               dict(fi=3, fw=_i32(2, 14, 14, 14), fb=_i32(5, 14, 14, 15), fo=_i32(6, 10, 10, 11)))       # P = 5 < No = 6
    for kw in SHARED_LIMITS + (dict(mean=None, scale=p), dict(mean=p, scale=None), dict(act=_lib.ACT_TANH), dict(act=_lib.ACT_SIGMOID),
                               dict(act=_lib.ACT_NONE), dict(act=-1)) + formats + (
            dict(logits=p, lstride=5), dict(logits=p, lstride=0), dict(logits=p, lstride=-6), dict(rpg=-1), dict(rpg=0, counts=p)):
        assert call(**kw) == E and call(**{"n_rows": 0, **nul, **kw}) == E, kw
    # ... the smallest and the largest shifts the ABI admits pass the limits: P = Nb, P - No = 1; P = 30, Nb = No = 0
    assert call(n_rows=0, fi=0, fw=_i32(1, 15, 15, 15), fb=_i32(1, 0, 0, 0), fo=_i32(0, 14, 15, 15), **nul) == OK
    assert call(n_rows=0, fi=15, fw=_i32(15, 15, 15, 15), fb=_i32(0, 0, 0, 0), fo=_i32(0, 0, 0, 0), **nul) == OK
    assert call(rpg=999) == E and call(n_rows=0, rpg=999, **nul) == OK
    for R, s in PAST_2_58:
        assert call(n_rows=R, stride=s, rpg=0, counts=None) == E and call(n_rows=R, lstride=s, rpg=0, counts=None) == E, (R, s)
    # 2. nothing to do: no pointer is looked at
    assert call(n_rows=0, rpg=0, **nul) == OK
    # 3. null pointers (x and the parameters: every output is optional) and alignment, every pointer
    for kw in (dict(x=None), dict(params=None), dict(x=p + 2), dict(mean=p + 4), dict(scale=p + 4), dict(params=p + 1), dict(labels=p + 2),
               dict(logits=p + 1), dict(counts=p + 4), dict(saturated=p + 4)):
        assert call(**kw) == E, kw
    # 4. no output asked for: AMCX_OK behind the pointer checks, nothing launched
    none = dict(labels=None, logits=None, counts=None, saturated=None, rpg=0)
    assert call(**none) == OK and call(**none, mean=None, scale=None) == OK
    assert call(**none, x=None) == E and call(**none, params=None) == E and call(**none, params=p + 1) == E
    del keep


def test_python_names_the_activation_it_refuses():
    with pytest.raises(ValueError, match="tanh"):
        qz.calibrate(None, None, cols=(0,), activation="tanh")
    z = _fixture("ties")
    q = qz.QuantizedMlp.from_state_dict(state_dict_of(z), z["ranges"], layout="reference")
    q.activation = "sigmoid"
    with pytest.raises(ValueError, match="sigmoid"):
        qz.classify_q15(None, q, cols=(0, 1, 2, 3))
    with pytest.raises(ValueError, match="shape"):
        qz.QuantizedMlp.from_state_dict(state_dict_of(z), z["ranges"][:2], layout="reference")
    with pytest.raises(ValueError, match="fractional bits"):
        qz.QuantizedMlp((4, 3), np.zeros(15, np.int16), 3, (2,), (5,), (6,))
