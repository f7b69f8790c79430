"""Feature subsets on the GPU (include/amcx.h, ABI 7): every column in the mask bit-identical to the 18-feature path, every
other column NaN -- for the plan kernels (128 ... 4096), the column-mask fallback (other sizes, the block variant), the host
entries, the extraction driver and the command line."""
import json

import numpy as np
import pytest

from amcpy_amd import _lib
from tests.conftest import GOLDEN, load_npz

pytestmark = pytest.mark.gpu

PLAN_SIZES = [128, 256, 512, 1024, 2048, 4096]
MASKS = {"no_spectral": _lib.FEATURES_NO_SPECTRAL, "cumulants": _lib.FEATURES_CUMULANTS, "used": 0x5154,
         "id13": 1 << 12, "id4": 1 << 3, "all": _lib.FEATURES_ALL}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible to torch")
    return torch


def _ids(mask):
    return [j + 1 for j in range(18) if (mask >> j) & 1]


def _inputs(N):
    """The golden fixtures of this size, synth arenas of all six modulations, noiseless balanced QPSK (the cancellation
    path), rows longer than the frame."""
    from amcpy_amd import synth
    blocks = []
    for name in (f"frames_n{N}.npz", f"edges_n{N}.npz", f"range_n{N}.npz", f"range_extreme_n{N}.npz"):
        if (GOLDEN / name).exists():
            blocks.append(np.asarray(load_npz(name)["iq"], np.complex64)[:, :N])
    blocks += [synth.host_block(m, snr, 7, N, seed=N + 31 * i + j)
               for i, m in enumerate(synth.MODS6) for j, snr in enumerate((-10.0, 10.0, 40.0))]
    rng = np.random.default_rng(N)
    pts = np.exp(1j * (np.pi / 4 + np.pi / 2 * np.arange(4)))
    n_sym = N // 8
    for _ in range(6):
        sym = np.concatenate([rng.choice([0, 2], n_sym // 2), rng.choice([1, 3], n_sym - n_sym // 2)])
        rng.shuffle(sym)
        blocks.append((np.repeat(pts[sym], 8) * np.exp(1j * rng.uniform(0, 2 * np.pi)))[None, :].astype(np.complex64))
    blocks.append(np.zeros((1, N), np.complex64))
    return np.concatenate(blocks).astype(np.complex64)


def _check(got, full, mask, what):
    cols = np.array([(mask >> j) & 1 == 1 for j in range(18)])
    assert np.array_equal(got[:, cols], full[:, cols], equal_nan=True), (what, np.argwhere(
        ~((got[:, cols] == full[:, cols]) | (np.isnan(got[:, cols]) & np.isnan(full[:, cols])))).tolist()[:8])
    assert np.isnan(got[:, ~cols]).all(), what


def _run(x, N, variant, mask, *, stride=None, out_cols=18):
    torch = _torch()
    from amcpy_amd.features import features18
    F = x.shape[0]
    L = N if stride is None else stride
    pad = np.full((F, L), 7.0 + 3.0j, np.complex64)
    pad[:, :N] = x
    xd = torch.from_numpy(pad).cuda()
    out = torch.full((F, out_cols), -5.0, dtype=torch.float32, device="cuda")
    features18(xd, out=out, frame_size=N, variant=variant, feature_ids=None if mask is None else _ids(mask))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:, 18:] == -5.0).all()
    return got[:, :18]


@pytest.mark.parametrize("N", PLAN_SIZES)
def test_plans_are_bit_identical(N):
    x = _inputs(N)
    full = _run(x, N, "wave", None)
    for name, mask in MASKS.items():
        _check(_run(x, N, "wave", mask), full, mask, (N, name))
        _check(_run(x, N, "auto", mask), full, mask, (N, name, "auto"))
    # odd row stride, an output wider than 18, a ragged frame count (not a multiple of any batch)
    for F in (1, 37, x.shape[0] - 1):
        for mask in (MASKS["no_spectral"], MASKS["cumulants"], MASKS["used"]):
            _check(_run(x[:F], N, "wave", mask, stride=N + 13, out_cols=21), full[:F], mask, (N, F))


@pytest.mark.parametrize("N,variant", [(1000, "auto"), (8192, "auto"), (16384, "auto"), (32767, "auto"), (2048, "block")])
def test_fallback_sizes(N, variant):
    from amcpy_amd import synth
    x = np.concatenate([synth.host_block(m, 8.0, 3, N, seed=N + i) for i, m in enumerate(synth.MODS6)]).astype(np.complex64)
    full = _run(x, N, variant, None)
    for mask in (MASKS["no_spectral"], MASKS["cumulants"], MASKS["used"], MASKS["id13"]):
        _check(_run(x, N, variant, mask), full, mask, (N, variant))


def test_subset_launch_inside_a_graph_capture():
    torch = _torch()
    from amcpy_amd.features import features18
    x = _inputs(2048)
    xd = torch.from_numpy(x).cuda()
    full = features18(xd, variant="wave").cpu().numpy()
    out = torch.empty((x.shape[0], 18), dtype=torch.float32, device="cuda")
    for mask in (MASKS["no_spectral"], MASKS["cumulants"]):
        features18(xd, out=out, feature_ids=_ids(mask))          # warm (one call per kernel and device before capture)
        torch.cuda.synchronize()
        out.fill_(-1.0)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                features18(xd, out=out, feature_ids=_ids(mask))
        g.replay()
        torch.cuda.synchronize()
        _check(out.cpu().numpy(), full, mask, ("graph", mask))


def test_host_paths_and_calculate_features():
    from amcpy_amd.feature_extraction import HipEngine
    from amcpy_amd.features import calculate_features, features18_host
    x = _inputs(1024)
    full = features18_host(x)
    for mask in (MASKS["used"], MASKS["cumulants"], MASKS["id4"]):
        _check(features18_host(x, feature_ids=_ids(mask)), full, mask, ("host", mask))
        _check(features18_host(x.astype(np.complex128), feature_ids=_ids(mask)), full, mask, ("host c128", mask))
    assert np.array_equal(features18_host(x), full, equal_nan=True)      # the context goes back to all 18
    for f in (0, 5, x.shape[0] - 1):
        ids = [13, 3, 13, 15]
        got = calculate_features(ids, x[f])
        assert got == [float(full[f, i - 1]) for i in ids]
    # HipEngine over a Fortran-ordered complex128 container (the layout loadmat returns)
    cont = np.asfortranarray((x[:24].reshape(2, 12, 1024)).astype(np.complex128))
    from amcpy_amd.feature_extraction import FrameRows
    eng_full = HipEngine(1024, 0)
    ref = eng_full(FrameRows(cont, 2, 12))
    eng_full.close()
    for mask in (MASKS["used"], MASKS["cumulants"]):
        eng = HipEngine(1024, 0, feature_ids=_ids(mask))
        _check(eng(FrameRows(cont, 2, 12)), ref, mask, ("engine", mask))
        eng.close()


def test_run_extraction_and_cli_features_used(tmp_path):
    """configs[0]-shaped containers (2 SNRs x 500 frames x 1024 samples): `extract --features used` writes files whose
    columns 3, 5, 7, 9, 13, 15 are bit-identical to a full run's and NaN elsewhere."""
    import subprocess
    import sys

    import scipy.io
    from amcpy_amd import synth
    from amcpy_amd.config import Config, Paths, SignalConfig
    from amcpy_amd.feature_extraction import run_extraction
    roots = {k: tmp_path / k for k in ("full", "used")}
    sig = SignalConfig(snr_values={0: "0", 1: "10"}, num_frames=500, frame_size=1024)
    mods = list(Config(signals=sig).signals.modulations_with_noise)
    data = {}
    for i, m in enumerate(mods):
        key = Config(signals=sig).signals.mat_info[m]
        data[key] = np.stack([synth.host_block(synth.MODS6[i % 6], snr, 500, 1100, seed=10 * i + k)
                              for k, snr in enumerate((0.0, 10.0))]).astype(np.complex128)
    for r in roots.values():
        cfg = Config(paths=Paths(root=r), signals=sig)
        cfg.paths.ensure_dirs()
        scipy.io.savemat(str(cfg.paths.mat_data / cfg.paths.mat_filename), data)
    run_extraction(Config(paths=Paths(root=roots["full"]), signals=sig), verbose=False)
    r = subprocess.run([sys.executable, "-m", "amcpy_amd", "extract", "--root", str(roots["used"]), "--frame-size", "1024",
                        "--num-frames", "500", "--snr-values", "0", "10", "--features", "used"],
                       capture_output=True, text=True, timeout=600, cwd=str(GOLDEN.parents[1]))
    assert r.returncode == 0, r.stderr[-3000:]
    cols = [2, 4, 6, 8, 12, 14]
    for m in mods:
        cf, cu = (Config(paths=Paths(root=roots[k]), signals=sig) for k in ("full", "used"))
        key = cf.signals.mat_info[m]
        full = scipy.io.loadmat(str(cf.paths.calculated_features / f"{m}_features.mat"))[key]
        used = scipy.io.loadmat(str(cu.paths.calculated_features / f"{m}_features.mat"))[key]
        assert used.shape == full.shape == (2, 500, 18) and used.dtype == np.float32
        assert np.array_equal(used[..., cols], full[..., cols])
        assert np.isnan(np.delete(used, cols, axis=-1)).all()
        rec = json.loads((cu.paths.calculated_features / f"{m}_features.provenance.json").read_text())
        assert rec["features"] == [3, 5, 7, 9, 13, 15]
