"""Feature subsets (include/amcx.h, ABI 7) on the host: argument checks of the new entries, which kernel a mask selects,
the CLI's `--features used`, and the provenance / --resume rules of a subset run.  Needs no GPU."""
import ctypes as C
import json

import numpy as np
import pytest

from amcpy_amd import _lib

FULL = {128: "amcx_features18_short_kernel<128>", 256: "amcx_features18_short_kernel<256>",
        512: "amcx_features18_short_kernel<512>", 1024: "amcx_features18_wave_kernel<1024>",
        2048: "amcx_features18_wave_kernel<2048>", 4096: "amcx_features18_wave_kernel<4096>"}


def test_constants_and_masks():
    assert (_lib.FEATURES_ALL, _lib.FEATURES_NO_SPECTRAL, _lib.FEATURES_CUMULANTS) == (0x3FFFF, 0x3FFFE, 0x3FE00)
    assert _lib.feature_mask(range(1, 19)) == _lib.FEATURES_ALL
    assert _lib.feature_mask(range(10, 19)) == _lib.FEATURES_CUMULANTS
    assert _lib.feature_mask([3, 5, 7, 9, 13, 15, 3]) == 0x5154
    for bad in ([0], [19], [2, 19], [1.0], ["3"], [True]):
        with pytest.raises(KeyError):
            _lib.feature_mask(bad)
    with pytest.raises(ValueError):
        _lib.feature_mask([])


def test_subset_entry_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    f = lib.amcx_features_c64_subset
    buf = (C.c_float * 64)()
    dummy = C.addressof(buf)
    for mask in (0, 1 << 18, 0x7FFFF, 0xFFFFFFFF):
        assert f(dummy, 4, 2048, 2048, dummy, 18, None, 0, mask, None, 0) == _lib.EINVAL, hex(mask)
    assert f(None, 4, 2048, 2048, dummy, 18, None, 0, 0x5154, None, 0) == _lib.EINVAL        # null input
    assert f(dummy, 4, 2048, 2048, None, 18, None, 0, 0x5154, None, 0) == _lib.EINVAL        # null output
    assert f(dummy, 4, 2048, 2047, dummy, 18, None, 0, 0x5154, None, 0) == _lib.EINVAL       # stride below frame_size
    assert f(dummy, 4, 2048, 2048, dummy, 17, None, 0, 0x5154, None, 0) == _lib.EINVAL       # output narrower than 18
    assert f(dummy, -1, 2048, 2048, dummy, 18, None, 0, 0x5154, None, 0) == _lib.EINVAL
    assert f(dummy, 4, 1, 2048, dummy, 18, None, 0, 0x5154, None, 0) == _lib.EINVAL          # frame_size out of range
    assert f(dummy, 4, 1000, 1000, dummy, 18, None, 2, 0x5154, None, 0) == _lib.ENOTSUP      # wave variant, not a power of two
    assert f(None, 0, 2048, 2048, None, 18, None, 0, 0x5154, None, 0) == _lib.OK             # n_frames = 0: a no-op
    assert f(None, 0, 2048, 2048, None, 18, None, 0, 0, None, 0) == _lib.EINVAL              # ... but the mask is checked first
    assert lib.amcx_ctx_set_feature_mask(None, 0x5154) == _lib.EINVAL


@pytest.mark.parametrize("N", sorted(FULL))
def test_kernel_name_subset_picks_the_plan(N):
    short = N <= 512
    stem = "amcx_features_subset_short_kernel" if short else "amcx_features_subset_wave_kernel"
    for variant in (_lib.VARIANT_AUTO, _lib.VARIANT_WAVE):
        assert _lib.kernel_name_subset(N, variant, _lib.FEATURES_NO_SPECTRAL) == f"{stem}<{N}, 1>"
        assert _lib.kernel_name_subset(N, variant, 0x5154) == f"{stem}<{N}, 1>"
        assert _lib.kernel_name_subset(N, variant, 1 << 3) == f"{stem}<{N}, 1>"          # id 4 alone: the envelope
        assert _lib.kernel_name_subset(N, variant, _lib.FEATURES_CUMULANTS) == f"{stem}<{N}, 2>"
        assert _lib.kernel_name_subset(N, variant, 1 << 12) == f"{stem}<{N}, 2>"         # id 13 alone
        # gamma_max asked for: the 18-feature kernel
        for mask in (_lib.FEATURES_ALL, 1, 1 | (1 << 12)):
            assert _lib.kernel_name_subset(N, variant, mask) == FULL[N] == _lib.kernel_name(N, variant)


@pytest.mark.parametrize("N,variant", [(1000, _lib.VARIANT_AUTO), (8192, _lib.VARIANT_AUTO), (32767, _lib.VARIANT_AUTO),
                                       (16384, _lib.VARIANT_WAVE), (2048, _lib.VARIANT_BLOCK)])
def test_kernel_name_subset_falls_back(N, variant):
    for mask in (_lib.FEATURES_NO_SPECTRAL, _lib.FEATURES_CUMULANTS, 0x5154):
        assert _lib.kernel_name_subset(N, variant, mask) == _lib.kernel_name(N, variant)
    with pytest.raises(ValueError):
        _lib.kernel_name_subset(N, variant, 0)
    with pytest.raises(ValueError):
        _lib.kernel_name_subset(N, variant, 1 << 18)


def test_features_used_resolves_to_the_reference_columns():
    from amcpy_amd.config import Config
    from amcpy_amd.main import build_parser, resolve_features
    cfg = Config()
    ids = resolve_features("used", cfg)
    assert ids == (3, 5, 7, 9, 13, 15)
    assert _lib.feature_mask(ids) == sum(1 << c for c in cfg.features.used) == 0x5154
    assert resolve_features("all", cfg) is None
    assert resolve_features("15,3,3", cfg) == (3, 15)
    assert resolve_features(",".join(map(str, range(1, 19))), cfg) is None
    for bad in ("0", "19", "x", ""):
        with pytest.raises(SystemExit):
            resolve_features(bad, cfg)
    assert build_parser().parse_args(["extract"]).features == "all"
    assert "plot" in build_parser()._subparsers._group_actions[0].choices["extract"].format_help()


def test_unknown_ids_raise_before_anything_runs():
    from amcpy_amd.features import calculate_features, features18_host
    with pytest.raises(KeyError):
        features18_host(np.zeros((1, 128), np.complex64), feature_ids=[3, 19])
    with pytest.raises(KeyError):
        calculate_features([0], np.zeros(128, np.complex64))
    from amcpy_amd.feature_extraction import HipEngine
    with pytest.raises(KeyError):
        HipEngine(128, 0, feature_ids=[25])


def _stand_in(block):
    """A CPU stand-in for the engine: 18 distinct, deterministic columns per frame."""
    b = np.asarray(block)
    base = np.abs(b).sum(axis=1, dtype=np.float64)[:, None]
    return (base + np.arange(1, 19)[None, :]).astype(np.float32)


def _setup(tmp_path):
    import scipy.io
    from amcpy_amd.config import Config, Paths, SignalConfig
    rng = np.random.default_rng(3)
    cfg = Config(paths=Paths(root=tmp_path), signals=SignalConfig(snr_values={0: "0", 1: "10"}, num_frames=4, frame_size=16))
    cfg.paths.ensure_dirs()
    mods = list(cfg.signals.modulations_with_noise)
    scipy.io.savemat(str(cfg.paths.mat_data / cfg.paths.mat_filename),
                     {cfg.signals.mat_info[m]: rng.standard_normal((2, 5, 20)) + 1j * rng.standard_normal((2, 5, 20)) for m in mods})
    return cfg, mods


def test_subset_files_provenance_and_resume(tmp_path):
    import scipy.io
    from amcpy_amd import feature_extraction as fe
    cfg, mods = _setup(tmp_path)
    calls = []

    def compute(block):
        calls.append(block.shape[0])
        return _stand_in(block)

    out = cfg.paths.calculated_features
    load = {m: (lambda m=m: scipy.io.loadmat(str(out / f"{m}_features.mat"))[cfg.signals.mat_info[m]]) for m in mods}
    rec = {m: (lambda m=m: json.loads((out / f"{m}_features.provenance.json").read_text())) for m in mods}

    fe.run_extraction(cfg, compute=compute, verbose=False)                         # full run: no "features" in the record
    full = {m: load[m]() for m in mods}
    assert all("features" not in rec[m]() for m in mods)
    full_rec = {m: (out / f"{m}_features.provenance.json").read_bytes() for m in mods}

    used = (3, 5, 7, 9, 13, 15)
    calls.clear()
    fe.run_extraction(cfg, compute=compute, verbose=False, resume=True, feature_ids=used)   # covered by the full files
    assert calls == []
    fe.run_extraction(cfg, compute=compute, verbose=False, feature_ids=used)              # computed: a subset file
    for m in mods:
        got = load[m]()
        assert got.shape == full[m].shape == (2, 4, 18) and got.dtype == np.float32
        cols = [i - 1 for i in used]
        assert np.array_equal(got[..., cols], full[m][..., cols])
        assert np.isnan(np.delete(got, cols, axis=-1)).all()
        assert rec[m]()["features"] == list(used)
    calls.clear()
    fe.run_extraction(cfg, compute=compute, verbose=False, resume=True, feature_ids=(5, 13))    # covered by the subset
    assert calls == []
    fe.run_extraction(cfg, compute=compute, verbose=False, resume=True, feature_ids=(5, 14))    # 14 is not in it
    assert len(calls) == len(mods)
    calls.clear()
    fe.run_extraction(cfg, compute=compute, verbose=False, resume=True)                         # never for a full request
    assert len(calls) == len(mods)
    for m in mods:                                                                              # ... whose record is as before
        assert (out / f"{m}_features.provenance.json").read_bytes() == full_rec[m]
        assert np.array_equal(load[m](), full[m])
    with pytest.raises(KeyError):
        fe.run_extraction(cfg, compute=compute, verbose=False, feature_ids=(3, 42))


def test_extract_entries_take_feature_ids(tmp_path):
    from amcpy_amd import feature_extraction as fe
    from amcpy_amd.config import Config, SignalConfig
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 3, 20)) + 1j * rng.standard_normal((2, 3, 20))).astype(np.complex64)
    cfg = Config(signals=SignalConfig(snr_values={0: "0", 1: "10"}, num_frames=3, frame_size=16))
    got = fe.extract_modulation(x, cfg, compute=_stand_in, feature_ids=[13])
    want = fe.extract_modulation(x, cfg, compute=_stand_in)
    assert np.array_equal(got[..., 12], want[..., 12]) and np.isnan(np.delete(got, 12, axis=-1)).all()
    raw = tmp_path / "s.bin"
    x.reshape(-1).tofile(raw)
    got = fe.extract_raw_stream(raw, 20, compute=_stand_in, feature_ids=[4])
    want = fe.extract_raw_stream(raw, 20, compute=_stand_in)
    assert got.shape == (6, 18) and np.isnan(np.delete(got, 3, axis=-1)).all() and np.array_equal(got[:, 3], want[:, 3])
    pairs = np.stack([x.real, x.imag], axis=-1).reshape(6, 20, 2).astype(np.float32)
    got = fe.extract_iq_pairs(pairs, 16, compute=_stand_in, feature_ids=[2, 18])
    want = fe.extract_iq_pairs(pairs, 16, compute=_stand_in)
    assert np.isnan(np.delete(got, [1, 17], axis=-1)).all() and np.array_equal(got[:, [1, 17]], want[:, [1, 17]])
