"""CPU-only tests of the classifier's host side (amcpy_amd/classifier.py, the amcx_mlp_* entry points' argument
checks, the `classify` command's parser): the BatchNorm fold against the reference's own float64 probabilities, the
checkpoint loader that runs nothing the file names, validation before any HIP call.  No GPU compute is called here;
the float64 forward that checks the fold lives in tests/classifier_host_ref.py, not in the product."""
import ctypes as C
import importlib.util
import sys
import types
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"


def _href():
    spec = importlib.util.spec_from_file_location("classifier_host_ref", REPO / "tests" / "classifier_host_ref.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["relu", "tanh", "sigmoid", "odd"])
def test_fold_reproduces_the_reference_probabilities(name):
    """MlpModel.from_state_dict folds every BatchNorm into its Linear in float64 and rounds once to float32.  A float64
    forward over the packed block must reproduce the fixture's p64 (the reference's module in double()) within
    4 x ref32_err, ref32_err being the reference's own float32 deviation from its float64 self -- the yardstick and
    margin of the GPU parity test -- and, over the un-rounded float64 fold, to 1e-12 (float64 reassociation of the
    BatchNorm affine only).  When the fixtures were generated the rounded fold alone moved the probabilities by
    3.4e-7 / 2.8e-7 / 2.2e-7 / 9.3e-8 (relu / tanh / sigmoid / odd) = 0.36 / 0.35 / 0.50 / 0.34 x ref32_err, and the
    un-rounded fold by at most 1.7e-15."""
    from amcpy_amd.classifier import MlpModel, params_floats
    href = _href()
    z = np.load(GOLDEN / f"classifier_ref_{name}.npz", allow_pickle=False)
    act, err = str(z["activation"]), float(z["ref32_err"])
    m = MlpModel.from_state_dict(href.state_dict_of(z), act)
    assert m.widths == ((6, 26, 29, 30, 6) if name != "odd" else (4, 32, 7, 3))
    assert m.params.dtype == np.float32 and m.params.size == params_floats(m.widths) == m.params64.size
    assert np.array_equal(m.params, m.params64.astype(np.float32))            # one rounding
    d32 = np.abs(href.forward64(z["x"], m.widths, m.params, act) - z["p64"]).max()
    d64 = np.abs(href.forward64(z["x"], m.widths, m.params64, act) - z["p64"]).max()
    print(f"{name}: rounded fold {d32:.3e} = {d32 / err:.2f} x ref32_err ({err:.3e}); float64 fold {d64:.2e}")
    assert d32 <= 4 * err
    assert d64 <= 1e-12


def test_fixtures_keep_what_the_gpu_tests_rely_on():
    href = _href()
    for name in ("relu", "tanh", "sigmoid", "odd"):
        z = np.load(GOLDEN / f"classifier_ref_{name}.npz", allow_pickle=False)
        assert z["x"].shape[0] == 8192 and z["x"].dtype == np.float32
        err = float(z["ref32_err"])
        assert err == np.abs(z["p32"].astype(np.float64) - z["p64"]).max() > 0
        assert (href.top_two_margin(z["p64"]) < 8 * err).mean() <= 0.0005
        assert (np.bincount(z["p64"].argmax(1), minlength=z["p64"].shape[1]) / 8192).min() >= 0.05
    z = np.load(GOLDEN / "classifier_synth6.npz", allow_pickle=False)
    assert float(z["accuracy"]) > 0.5 and float(z["accuracy"]) == (z["labels"] == z["true"]).mean()


def test_npz_round_trip_and_shape_discovery(tmp_path):
    from amcpy_amd.classifier import MlpModel, fold_state_dict
    rng = np.random.default_rng(3)
    sd = {"net.0.weight": rng.standard_normal((5, 3)), "net.0.bias": rng.standard_normal(5),
          "net.2.weight": rng.standard_normal((2, 5)), "net.2.bias": rng.standard_normal(2)}
    widths, p64 = fold_state_dict(sd)
    assert widths == (3, 5, 2)
    assert np.array_equal(p64, np.concatenate([sd["net.0.weight"].ravel(), sd["net.0.bias"],
                                               sd["net.2.weight"].ravel(), sd["net.2.bias"]]))
    m = MlpModel.from_state_dict(sd, "sigmoid", model_id="abc")
    m.save_npz(tmp_path / "m.npz")
    back = MlpModel.from_npz(tmp_path / "m.npz")
    assert back.widths == m.widths and back.activation == "sigmoid" and back.model_id == "abc"
    assert np.array_equal(back.params, m.params) and np.array_equal(back.params64, m.params64)
    with pytest.raises(ValueError):
        MlpModel.from_state_dict({"l.0.weight": np.zeros((33, 3)), "l.0.bias": np.zeros(33)})
    with pytest.raises(ValueError):
        MlpModel.from_state_dict({f"l.{i}.weight": np.zeros((3, 3)) for i in range(7)})
    with pytest.raises(ValueError):
        MlpModel((3, 5, 2), "gelu", np.zeros(32))
    with pytest.raises(ValueError):
        MlpModel((3, 5, 2), "relu", np.zeros(31))


def test_checkpoint_loads_without_the_reference_and_runs_nothing(tmp_path):
    """The reference's train_model saves {"model_state_dict", "model_id", "config"} with `config` an instance of its own
    dataclasses.  from_checkpoint must return the weights with `amcpy` NOT importable, read the activation from the
    stubbed config, and must not import or call anything the file names: a second, booby-trapped entry whose
    __reduce__ would write a marker file leaves no marker."""
    import torch
    from amcpy_amd.classifier import MlpModel, load_checkpoint
    href = _href()
    z = np.load(GOLDEN / "classifier_ref_tanh.npz", allow_pickle=False)
    sd = {k: torch.from_numpy(v.copy()) for k, v in href.state_dict_of(z).items()}
    marker = tmp_path / "marker"

    @dataclass(frozen=True)
    class TrainingConfig:
        activation: str = "tanh"
        layer_size_hl1: int = 26

    @dataclass(frozen=True)
    class Config:
        training: TrainingConfig = field(default_factory=TrainingConfig)
        root: Path = Path("/somewhere")

    class Trap:
        def __reduce__(self):
            return (_touch, (str(marker),))

    pkg, mod = types.ModuleType("amcpy"), types.ModuleType("amcpy.config")
    for cls in (TrainingConfig, Config, Trap):
        cls.__module__, cls.__qualname__ = "amcpy.config", cls.__name__
        setattr(mod, cls.__name__, cls)
    mod._touch = _touch
    _touch.__module__ = "amcpy.config"
    sys.modules["amcpy"], sys.modules["amcpy.config"] = pkg, mod
    try:
        torch.save({"model_state_dict": sd, "model_id": "1a2b3c4d", "config": Config(), "extra": Trap()},
                   tmp_path / "model-1a2b3c4d.pt")
    finally:
        del sys.modules["amcpy"], sys.modules["amcpy.config"]
        _touch.__module__ = __name__
    with pytest.raises(ImportError):
        import amcpy  # noqa: F401
    assert not marker.exists()
    with pytest.raises(Exception):                         # torch's safe loader refuses the config object
        torch.load(tmp_path / "model-1a2b3c4d.pt", weights_only=True)
    m = MlpModel.from_checkpoint(tmp_path / "model-1a2b3c4d.pt")
    assert not marker.exists(), "the loader ran a global the checkpoint names"
    assert "amcpy" not in sys.modules
    want = MlpModel.from_state_dict(href.state_dict_of(z), "tanh")
    assert m.activation == "tanh" and m.model_id == "1a2b3c4d" and m.widths == want.widths
    assert np.array_equal(m.params, want.params)
    assert MlpModel.from_checkpoint(tmp_path / "model-1a2b3c4d.pt", activation="relu").activation == "relu"
    ck = load_checkpoint(tmp_path / "model-1a2b3c4d.pt")
    assert ck["config"].training.layer_size_hl1 == 26
    assert not marker.exists()
    (tmp_path / "junk.pt").write_bytes(b"not a zip")
    with pytest.raises(ValueError):
        load_checkpoint(tmp_path / "junk.pt")


def _touch(path):
    Path(path).write_text("ran")
    return 0


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def test_mlp_argument_validation_needs_no_gpu():
    """Every limit is checked before any HIP call: widths 1 ... 32, 1 ... 6 layers, widths[0] == n_sel, columns in
    range, mean and scale together, whole groups, non-null parameters; an empty batch is a no-op."""
    from amcpy_amd import _lib
    lib = _lib.load()
    w = _i32(6, 26, 29, 30, 6)
    cols = _i32(2, 4, 6, 8, 12, 14)
    assert lib.amcx_mlp_params_floats(w, 4) == 26 * 6 + 26 + 29 * 26 + 29 + 30 * 29 + 30 + 6 * 30 + 6 == 2051
    assert lib.amcx_mlp_params_floats(_i32(4, 32, 7, 3), 3) == 32 * 4 + 32 + 7 * 32 + 7 + 3 * 7 + 3
    assert lib.amcx_mlp_params_floats(_i32(6, 0, 6), 2) == -1 and lib.amcx_mlp_params_floats(_i32(6, 33, 6), 2) == -1
    assert lib.amcx_mlp_params_floats(_i32(6), 0) == -1 and lib.amcx_mlp_params_floats(_i32(*[6] * 8), 7) == -1
    assert lib.amcx_mlp_params_floats(None, 4) == -1
    assert lib.amcx_mlp_params_floats(_i32(*[32] * 7), 6) == 6 * (32 * 32 + 32)

    fake = 4096                                             # a non-null pointer that is never dereferenced: every call below is refused first

    def call(n_rows=1000, stride=18, n_cols=18, cols=cols, n_sel=6, mean=None, scale=None, params=fake, widths=w,
             n_linear=4, act=_lib.ACT_RELU, labels=fake, probs=None, pstride=6, rpg=0, counts=None):
        return lib.amcx_mlp_classify_f32(fake, n_rows, stride, n_cols, cols, n_sel, mean, scale, params, widths, n_linear,
                                         act, labels, probs, pstride, rpg, counts, None)

    E = _lib.EINVAL
    assert call(widths=_i32(6, 0, 29, 30, 6)) == E and call(widths=_i32(6, 33, 29, 30, 6)) == E
    assert call(n_linear=0) == E and call(widths=_i32(*[6] * 8), n_linear=7) == E
    assert call(n_sel=5, cols=_i32(2, 4, 6, 8, 12)) == E                     # widths[0] != n_sel
    assert call(cols=_i32(2, 4, 6, 8, 12, 18)) == E and call(cols=_i32(-1, 4, 6, 8, 12, 14)) == E
    assert call(mean=fake) == E and call(scale=fake) == E                     # both or neither
    assert call(rpg=999, counts=fake) == E                                    # 1000 rows are not whole groups of 999
    assert call(rpg=0, counts=fake) == E
    assert call(params=None) == E
    assert call(act=3) == E and call(stride=17) == E and call(n_cols=33, stride=33) == E
    assert call(probs=fake, pstride=5) == E
    assert call(n_rows=-1) == E
    assert call(n_rows=0) == _lib.OK
    assert call(n_rows=0, rpg=10, counts=fake) == _lib.OK
    assert call(n_rows=0, widths=_i32(6, 33, 29, 30, 6)) == E                 # an invalid shape stays invalid for an empty batch
    buf = C.create_string_buffer(64)
    assert lib.amcx_mlp_kernel_name(w, 4, buf, len(buf)) == _lib.OK and buf.value == b"amcx_mlp_classify_kernel"
    assert lib.amcx_mlp_kernel_name(_i32(6, 40, 6), 2, buf, len(buf)) == E


def test_python_argument_checks_and_no_host_path():
    """classify() takes CUDA tensors only (the error types of postprocess.py) and nothing under amcpy_amd/ computes a
    label on the host: without a GPU the command fails with ENODEV."""
    import torch
    from amcpy_amd import _lib
    from amcpy_amd.classifier import MlpModel, classify, run_classification
    from amcpy_amd.config import Config, Paths
    m = MlpModel((2, 3, 2), "relu", np.zeros(9 + 8, np.float32))
    with pytest.raises(TypeError):
        classify(torch.zeros(4, 18), m, cols=[0, 1])                         # a host tensor
    with pytest.raises(TypeError):
        classify(np.zeros((4, 18), np.float32), m, cols=[0, 1])
    for name in ("classifier.py", "main.py"):
        assert "oracle" not in (REPO / "amcpy_amd" / name).read_text()
    if not torch.cuda.is_available():
        with pytest.raises(_lib.AmcxError) as ei:
            run_classification(Config(paths=Paths(root=Path("/nonexistent"))), "abc")
        assert ei.value.code == _lib.ENODEV


def test_classify_command_parses_and_resolves_models(tmp_path, capsys):
    from amcpy_amd.classifier import resolve_model_path
    from amcpy_amd.config import Config, Paths
    from amcpy_amd.main import build_parser
    with pytest.raises(SystemExit) as ei:
        build_parser().parse_args(["classify", "--help"])
    assert ei.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--root", "--model", "--mode", "--from-iq", "--device"):
        assert flag in text
    a = build_parser().parse_args(["classify", "--root", str(tmp_path), "--model", "1a2b3c4d", "--from-iq"])
    assert a.command == "classify" and a.mode == "test" and a.from_iq and a.device is None
    assert build_parser().parse_args(["classify", "--model", "x", "--mode", "training"]).mode == "training"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["classify", "--root", str(tmp_path)])       # --model is required
    cfg = Config(paths=Paths(root=tmp_path))
    assert resolve_model_path(cfg, "1a2b3c4d") == tmp_path / "ann" / "model-1a2b3c4d.pt"
    assert resolve_model_path(cfg, str(tmp_path / "m.npz")) == tmp_path / "m.npz"
    assert resolve_model_path(cfg, "some/dir/model-x.pt") == Path("some/dir/model-x.pt")
    e = build_parser().parse_args(["extract", "--root", str(tmp_path)])       # `extract` is untouched
    assert e.command == "extract" and e.features == "all"


def test_accuracy_table_equals_a_direct_count():
    """acc and confusion of hand-made counts (3 modulations, 2 SNRs, 3 classes and the bin of the rows without a label), two
    modulations of one class: against the counts read off directly."""
    from amcpy_amd.classifier import accuracy_table
    n_frames, labels = 10, [2, 0, 2]
    counts = np.array([[[1, 2, 6, 1], [0, 0, 10, 0]],
                       [[7, 0, 1, 2], [3, 3, 3, 1]],
                       [[5, 1, 4, 0], [0, 2, 5, 3]]], dtype=np.int64)
    assert counts.shape == (3, 2, 4) and (counts.sum(axis=2) == n_frames).all() and counts[:, :, 3].sum() > 0
    acc, confusion = accuracy_table(counts, labels, n_frames)
    assert acc.dtype == np.float64 and acc.shape == (3, 2)
    assert np.array_equal(acc, np.array([[6, 10], [7, 3], [4, 5]]) / 10.0)
    assert confusion.dtype == np.int64 and confusion.shape == (3, 4)
    want = np.zeros((3, 4), dtype=np.int64)
    for mod, lab in enumerate(labels):
        for snr in range(2):
            for predicted in range(4):
                want[lab, predicted] += counts[mod, snr, predicted]
    assert np.array_equal(confusion, want)
    assert np.array_equal(confusion, [[10, 3, 4, 3], [0, 0, 0, 0], [6, 5, 25, 4]]) and confusion.sum() == counts.sum()
