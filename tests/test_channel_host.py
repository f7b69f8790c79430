"""The fading multipath channel (include/amcx.h, ABI 16.2.1) on the host: the ABI and the tables, the entry's refusals in the
header's order, the plan by brute force, the profile builders, the data set and the `synth` command over the injected numpy
computes, and the statistics of the numpy restatement (tests/channel_ref.py).  Needs no GPU."""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib, channel as ch, waveform as wf
from tests import channel_ref as ref, synth_ref
from tests.test_synth_host import fake_features, synth_args

REPO = Path(__file__).resolve().parents[1]
NEW = ["amcx_channel_c64", "amcx_channel_plan", "amcx_kernel_name_channel", "amcx_abi_patch"]
SEED = 0x5EED5EED1234ABCD          # of every statistic below: a constant
KERNEL = "amcx_channel_c64_kernel"


def test_abi_16_2_1_in_header_binding_and_library():
    lib = _lib.load()
    assert (_lib.ABI_VERSION, _lib.ABI_MINOR) == (16, 2) == (lib.amcx_abi_version(), lib.amcx_abi_minor())
    assert _lib.ABI_PATCH >= 1 and lib.amcx_abi_patch() >= 1
    header = (REPO / "include" / "amcx.h").read_text()
    assert re.search(r"^#define AMCX_ABI_VERSION 16$", header, re.M) and re.search(r"^#define AMCX_ABI_MINOR 2$", header, re.M)
    assert int(re.search(r"^#define AMCX_ABI_PATCH (\d+)$", header, re.M).group(1)) >= 1
    assert header.index("ABI 16.2.1: AMCX_ABI_PATCH 1") < header.index("ABI 16.2: AMCX_ABI_MINOR 2")
    for define, value in (("RANDOM_PHASE 1u", _lib.CHANNEL_RANDOM_PHASE), ("MAX_PATHS 16", _lib.CHANNEL_MAX_PATHS),
                          ("MAX_SINUSOIDS 32", _lib.CHANNEL_MAX_SINUSOIDS), ("MAX_DELAY 1024", _lib.CHANNEL_MAX_DELAY)):
        assert f"#define AMCX_CHANNEL_{define}" in header and int(define.split()[1].rstrip("u")) == value
    assert (ref.RANDOM_PHASE, ref.MAX_PATHS, ref.MAX_SINUSOIDS, ref.MAX_DELAY) == (1, 16, 32, 1024) and ch.RECORD == ref.RECORD
    assert ref.RECORD.itemsize == 16
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header) and re.search(rf" T {name}$", exported, re.M), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    flat = " ".join(header.split())
    for prototype in (
            "int amcx_channel_c64(uint64_t seed, uint64_t row_index0, int64_t sample_index0, int64_t n_rows, int64_t row_samples, "
            "const void* in_c64_dev, int64_t in_row_stride, const void* paths_host, int32_t n_paths, int32_t n_sinusoids, "
            "int32_t interp_log2, uint32_t doppler_max, uint32_t flags, const float* sigma_dev, int64_t frames_per_group, "
            "void* out_c64_dev, int64_t out_row_stride, void* hip_stream);",
            "int amcx_channel_plan(int32_t n_paths, int32_t n_sinusoids, int32_t interp_log2, int32_t max_delay, "
            "int32_t* tile_outputs, int32_t* lds_bytes);",
            "const char* amcx_kernel_name_channel(void);", "int amcx_abi_patch(void);"):
        assert prototype in flat, prototype
    assert _lib.kernel_name_channel() == KERNEL


def test_channel_kernel_is_in_the_resource_table_without_spill_and_older_kernels_kept_their_bytes():
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    assert table[KERNEL]["spill"] == 0 and table[KERNEL]["scratch"] == 0
    listing = (REPO / "profiles" / "r34_channel_codeobj_kernels.txt").read_text()
    assert "DIFFERENT" not in listing and "ONLY IN A" not in listing and "101 kernels / device functions identical" in listing
    assert re.findall(r"ONLY IN B\s+amcx::(.+)", listing) == [KERNEL]
    text = (REPO / "amcpy_amd" / "csrc" / "amcx_channel_kernel.h").read_text()
    assert text.count("__global__") == 1 and "syn_finish(" in text and "ddc_stage_span<DdcC64" in text and "atomic" not in text.lower().replace("no atomics", "")
    assert "asm" not in text


PLAN_SWEEP = [(L, S, b, H) for L in (1, 3, 16) for S in (1, 32) for b in (0, 4, 12, 16) for H in (0, 17, 1024)]


@pytest.mark.parametrize("L,S,b,H", PLAN_SWEEP)
def test_plan_nodes_fit_for_every_first_sample(L, S, b, H):
    """The tile is 1 ... 2048 and even where more than one; for EVERY first sample a tile can have relative to the node raster
    the nodes of all paths stay within the budget of 2048, by brute force over the definition; the LDS holds the staged span,
    those nodes and the draws and stays under the 64 KiB that need no attribute."""
    tile, lds = _lib.channel_plan(L, S, b, H)
    B = 1 << b
    assert 1 <= tile <= 2048 and (tile == 1 or tile % 2 == 0)
    assert tile <= ((2048 // L) - 2) << b
    first = np.arange(min(B, 1 << 12), dtype=np.int64)                     # every residue, or -- beyond 4096 -- the first 4096 ...
    first = np.unique(np.concatenate([first, B - 1 - first, [0, B - 1]]))  # ... and the last: the count is monotone in between
    nodes = ((first + tile - 1) >> b) - (first >> b) + 2
    worst = int(nodes.max())
    assert L * worst <= 2048
    staged = 8 * (tile + H + (tile + H - 1) // 32)                         # the down-converter's padded image
    assert staged + 8 * L * worst + 16 * (L * S + L) <= lds <= staged + 15 + 8 * L * worst + 16 * (L * S + L)
    assert lds <= 65536


def test_plan_refuses_what_the_entry_refuses():
    for bad in ((0, 1, 0, 0), (17, 1, 0, 0), (1, 0, 0, 0), (1, 33, 0, 0), (1, 1, -1, 0), (1, 1, 17, 0), (1, 1, 0, -1), (1, 1, 0, 1025)):
        with pytest.raises(ValueError):
            _lib.channel_plan(*bad)
    assert _lib.load().amcx_channel_plan(1, 1, 0, 0, None, None) == _lib.OK
    assert max(_lib.channel_plan(L, 32, b, 1024)[1] for L in range(1, 17) for b in range(17)) <= 52 * 1024


def test_refusals_come_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_channel_c64
    buf = (C.c_float * 4096)()
    dummy = C.addressof(buf)
    dummy += -dummy % 16
    far = dummy + 8192                                                     # never read: every call below is refused
    paths = ref.records_of([(0, 1.0, 0.0, 0), (5, 0.5, 0.5, 1 << 30)])
    ok = dict(i0=0, R=4, S=100, x=dummy, xs=105, paths=paths.ctypes.data, L=2, Ns=8, b=3, flags=1, sigma=dummy, fpg=1, out=far, os=100)

    def call(**kw):
        a = {**ok, **kw}
        return f(1, 0, a["i0"], a["R"], a["S"], a["x"], a["xs"], a["paths"], a["L"], a["Ns"], a["b"], 1000, a["flags"], a["sigma"],
                 a["fpg"], a["out"], a["os"], None)

    nothing = dict(R=0, x=None, sigma=None, out=None)
    late = ref.records_of([(1025, 1.0, 0.0, 0)]).ctypes.data
    negative = ref.records_of([(-1, 1.0, 0.0, 0)])
    # 1. shape and ranges, in front of the no-op
    for kw in (dict(L=0), dict(L=17), dict(Ns=0), dict(Ns=33), dict(b=-1), dict(b=17), dict(flags=2), dict(flags=3), dict(paths=None),
               dict(paths=late, L=1), dict(paths=negative.ctypes.data, L=1), dict(S=0), dict(i0=-1), dict(i0=(1 << 40) - 100),
               dict(S=1 << 40, xs=1 << 41, os=1 << 40, R=1), dict(R=-1), dict(xs=104), dict(os=99), dict(fpg=0),
               dict(R=1 << 30, xs=(1 << 28) + 1), dict(R=1 << 30, os=(1 << 28) + 1), dict(R=1 << 31)):
        assert call(**kw) == _lib.EINVAL, kw
        assert call(**{**nothing, **kw}) == _lib.EINVAL, kw
    assert call(i0=(1 << 40) - 101, **nothing) == _lib.OK                  # the last sample is 2^40 - 2
    # 2. no rows: fine with null pointers
    assert call(**nothing) == _lib.OK and call(R=0) == _lib.OK
    # 3. null pointers (sigma may be null: no noise), alignment, overlap
    assert call(x=None) == _lib.EINVAL and call(out=None) == _lib.EINVAL
    assert call(x=dummy + 4) == _lib.EINVAL and call(out=far + 4) == _lib.EINVAL and call(sigma=dummy + 2) == _lib.EINVAL
    assert call(R=0, x=dummy + 4, out=far + 4) == _lib.OK                  # nothing is read or written
    last_in = dummy + 8 * (3 * 105 + 105)                                  # the first byte behind the input
    for out in (dummy, dummy + 8, last_in - 8, dummy - 8 * (3 * 100 + 100) + 8):
        assert call(out=out) == _lib.EINVAL and call(out=out, sigma=None) == _lib.EINVAL, out - dummy


# ---- the profiles ---------------------------------------------------------------------------------------------------------------
def test_builders_have_unit_power_and_the_records_fold_the_sinusoids_in():
    for p in (ch.rayleigh(), ch.rician(6.0), ch.rician(-3.0, 0.7), ch.exponential(6, 3, 3.0), ch.exponential(16, 64, 1.0), ch.two_ray(40, -6.0),
              ch.Profile([0, 7], [1.0, 0.5], [2.0, 0.0], [1.0, 0.0])):
        assert abs(p.power - 1.0) <= 1e-12
        for S in (1, 16, 32):
            rec = p.records(S)
            assert rec.dtype == ref.RECORD and rec.shape == p.delays.shape
            power = S * (rec["diffuse_gain"].astype(np.float64) ** 2).sum() + (rec["los_gain"].astype(np.float64) ** 2).sum()
            assert abs(power - 1.0) <= 4 * len(rec) * 2.0 ** -24          # float32 gains
    k = ch.rician(6.0)
    assert abs(10 * np.log10(k.los_gain[0] ** 2 / k.diffuse_gain[0] ** 2) - 6.0) < 1e-9
    e = ch.exponential(3, 5, 3.0)
    assert e.delays.tolist() == [0, 5, 10] and e.history == 10 and abs(20 * np.log10(e.diffuse_gain[1] / e.diffuse_gain[0]) + 3.0) < 1e-9
    assert ch.rician(0.0, 0.5).records(4)["los_doppler_q31"].tolist() == [1 << 30] and ch.rician(0.0, 1.0).records(4)["los_doppler_q31"].tolist() == [(1 << 31) - 1]
    s = ch.static([9, 0], [-0.5, 2.0])
    assert s.records(16).tolist() == [(0, 0.0, 2.0, 0), (9, 0.0, -0.5, 0)]
    for bad in (lambda: ch.Profile([], []), lambda: ch.Profile([1025], [1.0]), lambda: ch.Profile([-1], [1.0]), lambda: ch.Profile([0], [0.0]),
                lambda: ch.Profile(list(range(17)), 1.0), lambda: ch.Profile([0], [1.0], [0.0], [1.5]), lambda: ch.rayleigh().records(33),
                lambda: ch.parse_profile("cost207"), lambda: ch.parse_profile("rician")):
        with pytest.raises(ValueError):
            bad()
    assert ch.parse_profile("exp:3:5:3").delays.tolist() == [0, 5, 10] and ch.parse_profile("tworay:40:-6").history == 40
    assert ch.parse_profile("rician:6").spec == "rician:6" and ch.parse_profile("rayleigh").history == 0


def test_default_interp_log2_and_doppler_units():
    assert ch.default_interp_log2(0.0) == 16 and ch.default_interp_log2(1e-3) == 3 and ch.default_interp_log2(1.0 / 256) == 2
    assert ch.default_interp_log2(1.0 / 64) == 0 and ch.default_interp_log2(0.4) == 0 and ch.default_interp_log2(2.0 ** -22) == 16
    for f in (1e-5, 1e-3, 0.01):
        b = ch.default_interp_log2(f)
        assert f * 2 ** b <= 1 / 64 < f * 2 ** (b + 1)
    assert ch.doppler_max_of(0.25) == 1 << 31 and ch.doppler_max_of(0.0) == 0
    with pytest.raises(ValueError):
        ch.doppler_max_of(0.5)


# ---- the restatement's integers and statistics ------------------------------------------------------------------------------------
def test_draws_follow_the_generators_counter_layout():
    from tests.train_ref import philox4x32_10
    seed, r = (7 << 32) | 5, (3 << 32) | 9
    rec = ref.records_of([(0, 1.0, 0.0, 0), (4, 0.5, 0.5, -(1 << 30))])
    phase0, step, los0, los_step = ref.draws(seed, r, rec, 3, 1000, ref.RANDOM_PHASE)
    X = [int(w) for w in philox4x32_10((32 * 1 + 2, 3 << 28, 9, 3), (5, 7))]
    c = float(ref.mixer32(np.array([X[1]]))[0][0])
    assert int(phase0[1, 2]) == X[0] << 32 and int(step[1, 2]) == (int(c * 2.0 ** 31) * 1000) % (1 << 64)
    XL = [int(w) for w in philox4x32_10((512 + 1, 3 << 28, 9, 3), (5, 7))]
    assert int(los0[1]) == XL[0] << 32 and int(los_step[1]) == (-(1 << 30) * 1000) % (1 << 64) and int(los_step[0]) == 0
    assert not ref.draws(seed, r, rec, 3, 1000, 0)[2].any()
    rows = np.array([r, r + 1, 1 << 40])                                   # an array of rows draws what each row draws
    many = ref.draws(seed, rows, rec, 3, 1000, ref.RANDOM_PHASE)
    for i, row in enumerate(rows):
        for a, b in zip(many, ref.draws(seed, int(row), rec, 3, 1000, ref.RANDOM_PHASE)):
            assert np.array_equal(a[i], b)
    for w, v in zip(ref.channel_words(seed, np.array([5, 600]), r), synth_ref.words(seed, 3, np.array([5, 600]), r)):
        assert np.array_equal(w, v)


def test_reference_statistics():
    """Checked on the restatement's definition first: one Rayleigh path of 16 sinusoids at f_d = 1 / 256 over 4096 rows.  The
    mean power within 5 sqrt((1 - 1 / S) / R) of 1 (|c|^2 - 1 is a sum of S (S - 1) uncorrelated unit-modulus cross terms over
    S^2), the autocorrelation within 5 / sqrt(R) of J0(2 pi f_d tau)."""
    from scipy.special import j0
    S, R, fd = 16, 4096, 1.0 / 256
    taus = np.array([0, 49, 98, 156, 250, 400])
    g = ref.gain64(SEED, np.arange(R), ch.rayleigh().records(S), S, ch.doppler_max_of(fd), ref.RANDOM_PHASE, 1000 + taus)[:, 0, :]
    power = float((np.abs(g[:, 0]) ** 2).mean())
    print(f"channel statistics: power off by {abs(power - 1) / np.sqrt((1 - 1 / S) / R):.2f} standard errors")
    assert abs(power - 1.0) <= 5 * np.sqrt((1 - 1 / S) / R)
    for i, tau in enumerate(taus[1:], start=1):
        corr = complex((np.conj(g[:, 0]) * g[:, i]).mean())
        print(f"channel statistics: lag {tau}: off by {abs(corr - j0(2 * np.pi * fd * tau)) * np.sqrt(R):.2f} / sqrt(R)")
        assert abs(corr - j0(2 * np.pi * fd * tau)) <= 5 / np.sqrt(R)


def test_restated_gains_meet_the_closed_form_within_the_derived_bound():
    S, fd = 16, 1.0 / 256
    rec, dm, n = ch.rayleigh().records(S), ch.doppler_max_of(fd), 1000 + np.arange(700)
    g = ref.gain64(SEED, 3, rec, S, dm, ref.RANDOM_PHASE, n)[0]
    for b in (0, ch.default_interp_log2(fd)):
        re, im = ref.sample_gains(SEED, 3, rec, S, b, dm, ref.RANDOM_PHASE, n)
        assert np.abs((re.astype(np.float64) + 1j * im.astype(np.float64)) - g).max() <= ref.physics_bound(S, fd, b)
    ones = ref.restate(np.ones(700, np.complex64), rec, S, 2, dm, ref.RANDOM_PHASE, seed=SEED, r=3, n0=1000)
    re, im = ref.sample_gains(SEED, 3, rec, S, 2, dm, ref.RANDOM_PHASE, n)
    assert np.array_equal(ones.real, re[0]) and np.array_equal(ones.imag, im[0])


# ---- apply, the fader, the data set and the command over the injected computes ---------------------------------------------------
def _signal(R, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, n)) + 1j * rng.standard_normal((R, n))).astype(np.complex64)


def test_apply_and_fader_cut_anywhere_equal_one_call_on_the_restatement():
    p = ch.exponential(3, 5, 3.0)
    kw = dict(doppler=2e-3, sinusoids=8, seed=5, snr_db=10.0, compute=ref.numpy_apply)
    x = _signal(3, 300 + p.history, 1)
    whole = ch.apply(x, p, row_index0=1 << 33, **kw)
    assert whole.shape == (3, 300) and whole.dtype == np.complex64
    rows = np.concatenate([ch.apply(x[:1], p, row_index0=1 << 33, **kw), ch.apply(x[1:], p, row_index0=(1 << 33) + 1, **kw)])
    assert rows.tobytes() == whole.tobytes()
    late = ch.apply(x[:, 100:], p, row_index0=1 << 33, sample_index0=100, **kw)
    assert late.tobytes() == whole[:, 100:].tobytes()
    fader = ch.Fader(p, row=(1 << 33) + 2, **kw)
    stream = np.concatenate([np.zeros(p.history, np.complex64), x[2]])
    want = ch.apply(stream[None], p, row_index0=(1 << 33) + 2, **kw)[0]
    parts = [fader.push(x[2][a:b]) for a, b in ((0, 1), (1, 1), (1, 64), (64, 310))]
    assert [q.shape for q in parts] == [(1,), (0,), (63,), (246,)] and fader.index == 310
    assert np.concatenate(parts).tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        ch.apply(x, p, snr_db=[1.0, 2.0], frames_per_group=1, compute=ref.numpy_apply)
    with pytest.raises(ValueError):
        ch.apply(x[:, :p.history], p, compute=ref.numpy_apply)
    with pytest.raises(ValueError):
        ch.Fader(p, sample_index0=3)


FADE = dict(profile=ch.two_ray(3, -3.0), doppler=2e-3, sinusoids=4, compute=ref.numpy_apply)


def test_faded_dataset_rows_are_the_same_for_every_subset():
    kw = dict(sps=(2, 1), taps=wf.design_rrc(2, 4), seed=9, cfo=0.01, compute=synth_ref.numpy_generate, channel=FADE)
    full = wf.dataset(["BPSK", "WGN"], [0.0, 12.5], 4, 40, **kw)
    assert full["BPSK"].shape == (2, 4, 40) and full["BPSK"].dtype == np.complex64
    part = wf.dataset(["BPSK"], [12.5], 2, 40, first_frame=2, **kw)       # frames 2 ... 3 asked alone
    assert np.array_equal(part["BPSK"][0], full["BPSK"][1, 2:4])
    plain = wf.dataset(["BPSK"], [12.5], 4, 40, **{k: v for k, v in kw.items() if k != "channel"})
    assert not np.array_equal(plain["BPSK"][0], full["BPSK"][1])
    # the faded row is the clean row, history in front, through the channel with the same seed, row and sigma
    row = wf.dataset_row("BPSK", 12.5, 1)
    clean = wf.generate("BPSK", 1, 43, row_index0=row, **{k: v for k, v in kw.items() if k != "channel"})
    want = ch.apply(clean, FADE["profile"], doppler=2e-3, sinusoids=4, seed=9, row_index0=row, sigma=wf.sigma_of(12.5), compute=ref.numpy_apply)
    assert np.array_equal(full["BPSK"][1, 1], want[0])
    feats = wf.dataset_features(["BPSK"], [0.0, 12.5], 4, 40, chunk_frames=3, features=fake_features, **kw)
    assert feats["BPSK"].tobytes() == np.stack([fake_features(full["BPSK"][s]) for s in range(2)]).tobytes()
    with pytest.raises(ValueError):
        wf.dataset(["BPSK"], [0.0], 1, 40, **dict(kw, channel=dict(doppler=1e-3)))


def test_synth_command_with_a_channel_writes_the_files_extract_reads(tmp_path):
    import scipy.io
    from amcpy_amd import feature_extraction as fe
    from amcpy_amd.main import run_synth, synth_config
    args = synth_args(tmp_path, "--channel", "rayleigh", "--doppler", "0.002", "--sinusoids", "4")
    assert (args.channel, args.doppler, args.sinusoids) == ("rayleigh", 0.002, 4)
    assert (synth_args(tmp_path).channel, synth_args(tmp_path).doppler, synth_args(tmp_path).sinusoids) == (None, 0.0, 16)
    written = run_synth(args, compute=synth_ref.numpy_generate, channel_compute=ref.numpy_apply)
    mat = scipy.io.loadmat(str(written[0]))
    fade = dict(profile=ch.rayleigh(), doppler=0.002, sinusoids=4, compute=ref.numpy_apply)
    kw = dict(sps=(2, 1), taps=wf.design_rrc(2, 4), seed=4, compute=synth_ref.numpy_generate)
    want = wf.dataset(["BPSK"], [0.0, 10.0], 3, 64, channel=fade, **kw)
    assert mat["signal_bpsk"].shape == (2, 3, 64) and np.array_equal(mat["signal_bpsk"], want["BPSK"])
    assert not np.array_equal(want["BPSK"], wf.dataset(["BPSK"], [0.0, 10.0], 3, 64, **kw)["BPSK"])
    only = synth_args(tmp_path, "--features-only", "--channel", "rician:6", "--doppler", "0.002")
    files = run_synth(only, compute=synth_ref.numpy_generate, features=fake_features, channel_compute=ref.numpy_apply)
    cfg, _ = synth_config(only)
    mat_path = cfg.paths.mat_data / cfg.paths.mat_filename
    for mod, path in zip(("BPSK", "WGN"), files):
        key = cfg.signals.mat_info[mod]
        assert fe._already_extracted(path, key, (2, 3, 18), fe._provenance(cfg, mat_path, key))
        record = json.loads(fe._provenance_path(path).read_text())["channel"]
        assert (record["profile"], record["doppler"], record["sinusoids"], record["delays"]) == ("rician:6", 0.002, 16, [0])
    bad = synth_args(tmp_path, "--channel", "cost207")
    with pytest.raises(SystemExit):
        run_synth(bad, compute=synth_ref.numpy_generate, channel_compute=ref.numpy_apply)
