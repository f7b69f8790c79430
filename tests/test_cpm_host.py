"""The continuous-phase generator (include/amcx.h, ABI 16.2.2) on the host: the ABI and the tables, the entry's refusals in the
header's order, the plan by brute force, the two forms of the phase (tests/cpm_ref.py), the pulse designers, the names and
their rows, the data set, the stream and the `synth` command over the injected numpy compute.  Needs no GPU."""
import ctypes as C
import json
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib, waveform as wf
from tests import cpm_ref as ref, synth_ref
from tests.test_synth_host import fake_features

REPO = Path(__file__).resolve().parents[1]
NEW = ["amcx_synth_cpm_c64", "amcx_synth_cpm_plan", "amcx_kernel_name_synth_cpm"]
KERNEL = "amcx_synth_cpm_c64_kernel"
SEED = 0x5EED5EED1234ABCD


def test_abi_16_2_2_in_header_binding_and_library():
    lib = _lib.load()
    assert (_lib.ABI_VERSION, _lib.ABI_MINOR) == (16, 2) == (lib.amcx_abi_version(), lib.amcx_abi_minor())
    assert _lib.ABI_PATCH >= 2 and lib.amcx_abi_patch() >= 2
    header = (REPO / "include" / "amcx.h").read_text()
    assert re.search(r"^#define AMCX_ABI_VERSION 16$", header, re.M) and re.search(r"^#define AMCX_ABI_MINOR 2$", header, re.M)
    assert int(re.search(r"^#define AMCX_ABI_PATCH (\d+)$", header, re.M).group(1)) >= 2
    assert header.index("ABI 16.2.2: AMCX_ABI_PATCH 2") < header.index("ABI 16.2.1: AMCX_ABI_PATCH 1") < header.index("ABI 16.2: AMCX_ABI_MINOR 2")
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header) and re.search(rf" T {name}$", exported, re.M), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    flat = " ".join(header.split())
    for prototype in (
            "int amcx_synth_cpm_plan(int32_t n_taps, int32_t up, int32_t down, int64_t n_rows, int64_t row_samples, "
            "int32_t* tile_outputs, int32_t* lds_bytes, int32_t* segments);",
            "int amcx_synth_cpm_c64(uint64_t seed, uint64_t row_index0, int64_t sample_index0, int64_t n_rows, int64_t row_samples, "
            "int64_t row_stride, int32_t order, const uint32_t* phase_taps_dev, int32_t n_taps, uint32_t phase_full, int32_t up, "
            "int32_t down, int32_t tau0, uint64_t phase_step, uint32_t cfo_max, uint32_t flags, const float* sigma_dev, "
            "int64_t frames_per_group, const uint32_t* acc_in_dev, uint32_t* acc_out_dev, int32_t segments, void* out, "
            "void* hip_stream);",
            "const char* amcx_kernel_name_synth_cpm(void);"):
        assert prototype in flat, prototype
    assert _lib.kernel_name_synth_cpm() == KERNEL


def test_cpm_kernel_is_in_the_resource_table_without_spill_and_older_kernels_kept_their_bytes():
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    assert table[KERNEL]["spill"] == 0 and table[KERNEL]["scratch"] == 0
    listing = (REPO / "profiles" / "r35_cpm_codeobj_kernels.txt").read_text()
    assert "DIFFERENT" not in listing and "ONLY IN A" not in listing and "102 kernels / device functions identical" in listing
    assert re.findall(r"ONLY IN B\s+amcx::(.+)", listing) == [KERNEL]
    text = (REPO / "amcpy_amd" / "csrc" / "amcx_synth_cpm_kernel.h").read_text()
    assert text.count("__global__") == 1 and "syn_finish(" in text and "poly_stage_taps(" in text and "asm" not in text
    hip = (REPO / "amcpy_amd" / "csrc" / "amcx.hip").read_text()
    assert hip.index('#include "amcx_synth_cpm_kernel.h"') < hip.index('#include "amcx_channel_kernel.h"')


PLAN_SWEEP = [(1, 1, 1), (8, 8, 1), (8, 8, 3), (32, 8, 1), (4096, 256, 255), (7, 3, 4096), (4096, 1, 4096), (5, 8, 1)]


@pytest.mark.parametrize("T,U,V", PLAN_SWEEP)
def test_plan_spans_fit_for_every_first_sample(T, U, V):
    """The tile is the linear generator's; for EVERY timing and every remainder a tile can begin at, the symbols of its span --
    the first window's first to the last window's last -- fit what the LDS holds beside the scan, the taps and the reduction's
    words, by brute force over the definition; nothing passes the 64 KiB that need no attribute."""
    tile, lds, seg = _lib.synth_cpm_plan(T, U, V, 4096, 1 << 20)
    assert tile == _lib.synth_plan(2, T, U, V)[0] and seg == 1 and lds <= 65536
    P = -(-T // U)
    tau = np.arange(U, dtype=np.int64)[:, None]
    k = np.arange(2 * U, dtype=np.int64)[None, :]
    t_first = k * tile * V + tau
    span = ((P - 1) + (t_first + (tile - 1) * V) // U) - t_first // U + 1
    pitch = P | 1
    assert int(span.max()) <= 5120 and lds >= 8 * int(span.max()) + 4 + 4 * U * pitch + 32


def test_plan_cuts_rows_into_segments_only_where_the_rows_do_not_fill_the_device():
    tile = _lib.synth_cpm_plan(8, 8, 1, 1, 1)[0]
    assert tile == 4096
    assert _lib.synth_cpm_plan(8, 8, 1, 1, 1)[2] == 1                      # one tile: one segment
    assert _lib.synth_cpm_plan(8, 8, 1, 1, 3 * tile + 1)[2] == 4           # never more than the row's tiles
    assert _lib.synth_cpm_plan(8, 8, 1, 1, 1 << 22)[2] == 64               # never more than 64
    assert _lib.synth_cpm_plan(8, 8, 1, 1 << 20, 1 << 22)[2] == 1          # the rows alone fill the device
    few = _lib.synth_cpm_plan(8, 8, 1, 100, 1 << 22)[2]
    assert 2 <= few <= 64
    # 65 tiles in at most 64 segments: runs of 2 tiles, 33 of them, none empty
    assert _lib.synth_cpm_plan(8, 8, 1, 1, 65 * tile)[2] == 33
    for bad in ((0, 8, 1, 1, 1), (4097, 8, 1, 1, 1), (8, 0, 1, 1, 1), (8, 257, 1, 1, 1), (8, 8, 0, 1, 1), (8, 8, 4097, 1, 1),
                (8, 8, 1, -1, 1), (8, 8, 1, 1, 0), (8, 8, 1, 1, 1 << 40)):
        with pytest.raises(ValueError):
            _lib.synth_cpm_plan(*bad)
    assert _lib.load().amcx_synth_cpm_plan(8, 8, 1, 1, 1, None, None, None) == _lib.OK


def test_refusals_come_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_synth_cpm_c64
    buf = (C.c_float * 256)()
    dummy = C.addressof(buf)
    dummy += -dummy % 16
    ok = dict(i0=0, R=4, S=100, stride=100, order=4, taps=dummy, T=5, U=2, V=3, tau0=0, flags=3, sigma=dummy, fpg=1, ain=None, aout=None,
              seg=0, out=dummy)

    def call(**kw):
        a = {**ok, **kw}
        return f(1, 0, a["i0"], a["R"], a["S"], a["stride"], a["order"], a["taps"], a["T"], 1 << 30, a["U"], a["V"], a["tau0"], 0, 0,
                 a["flags"], a["sigma"], a["fpg"], a["ain"], a["aout"], a["seg"], a["out"], None)

    nothing = dict(R=0, taps=None, sigma=None, out=None)
    # 1. ranges, in front of the no-op: the shape (order from 2), tau0 and the flags, the row's samples, the rows, the groups, the segments
    for kw in (dict(order=-1), dict(order=0), dict(order=1), dict(order=257), dict(U=0), dict(U=257), dict(V=0), dict(V=4097), dict(T=0),
               dict(T=4097), dict(tau0=-1), dict(tau0=2), dict(flags=4), dict(flags=7),
               dict(S=0, stride=0), dict(i0=-1), dict(i0=(1 << 40) - 100), dict(S=1 << 40, stride=1 << 40, R=1),
               dict(R=-1), dict(stride=99), dict(R=1 << 30, stride=(1 << 28) + 1), dict(fpg=0), dict(fpg=-3), dict(seg=-1), dict(seg=65),
               dict(R=1 << 31, S=1, stride=1)):
        assert call(**kw) == _lib.EINVAL, kw
        assert call(**{**nothing, **kw}) == _lib.EINVAL, kw
    assert call(i0=(1 << 40) - 101, **nothing) == _lib.OK                  # the last sample is 2^40 - 2; no rows, so no acc_in either
    # 2. no rows: fine with null pointers
    assert call(**nothing) == _lib.OK and call(R=0) == _lib.OK and call(R=0, i0=5) == _lib.OK
    # 3. null pointers (acc_in where the call begins behind sample 0), alignment, the two acc arrays' overlap
    for key in ("out", "taps", "sigma"):
        assert call(**{key: None}) == _lib.EINVAL, key
    assert call(i0=1) == _lib.EINVAL and call(i0=1, aout=dummy) == _lib.EINVAL
    assert call(out=dummy + 4) == _lib.EINVAL and call(taps=dummy + 2) == _lib.EINVAL and call(sigma=dummy + 1) == _lib.EINVAL
    assert call(i0=1, ain=dummy + 2) == _lib.EINVAL and call(aout=dummy + 2) == _lib.EINVAL
    for aout in (dummy, dummy + 4, dummy + 12, dummy - 12):                # four rows: 16 bytes each
        assert call(i0=1, ain=dummy, aout=aout) == _lib.EINVAL and call(ain=dummy, aout=aout) == _lib.EINVAL, aout - dummy
    assert call(R=0, out=dummy + 4, taps=dummy + 2, ain=dummy, aout=dummy) == _lib.OK      # nothing is read or written


# ---- the two forms of the phase -------------------------------------------------------------------------------------------------
def random_pulse(rng, T):
    taps = np.sort(rng.integers(0, 1 << 32, T, dtype=np.uint64)).astype(np.uint32)
    return taps, int(rng.integers(0, 1 << 32))


def test_definition_equals_the_computed_form_on_random_shapes():
    rng = np.random.default_rng(35)
    for case in range(24):
        U, V = int(rng.integers(1, 9)), int(rng.integers(1, 12))
        T = int(rng.integers(1, 4 * U + 2))
        order = int(rng.choice([2, 3, 4, 8, 255, 256]))
        taps, full = random_pulse(rng, T)
        tau = int(rng.integers(0, U))
        r = int(rng.integers(0, 1 << 62))
        want = ref.phi_definition(SEED, r, np.arange(40), order, taps, full, U, V, tau)
        got, _ = ref.phi_computed(SEED, r, 0, 40, order, taps, full, U, V, tau)
        assert np.array_equal(got, want), (case, T, U, V, order, tau)
        # any cut: the second part from the state the first leaves, which is A at a symbol the timing does not move
        cut = int(rng.integers(1, 40))
        first, acc = ref.phi_computed(SEED, r, 0, cut, order, taps, full, U, V, tau)
        second, end = ref.phi_computed(SEED, r, cut, 40 - cut, order, taps, full, U, V, tau, acc)
        assert np.array_equal(np.concatenate([first, second]), want), (case, cut)
        assert acc == ref.prefix(SEED, r, cut * V // U, order) and end == ref.prefix(SEED, r, 40 * V // U, order)


def test_symbols_are_the_linear_generator_s_indices():
    j = np.arange(1000)
    for order in (2, 4, 7, 256):
        a = ref.alphas(SEED, 9, j, order)
        assert np.array_equal(a, 2 * synth_ref.symbol_indices(SEED, 9, j, order) - (order - 1))
        assert set(np.unique(a)) <= set(range(-(order - 1), order, 2))
        assert order > 8 or len(np.unique(a)) == order                     # (1000 draws need not meet every one of 256 values)


# ---- the designers ----------------------------------------------------------------------------------------------------------------
def test_designers_are_monotone_end_at_phase_full_and_give_a_quarter_turn_at_h_one_half():
    for U in (1, 2, 3, 8, 255, 256):
        for pulse in (wf.design_cpfsk(U), wf.design_cpfsk(U, 1), wf.design_cpfsk(U, Fraction(1, 3)), wf.design_gmsk(U),
                      wf.design_gfsk(U, Fraction(7, 10), 0.5, 3), wf.design_gmsk(U, 0.25, 6)):
            taps = pulse.phase_taps.astype(np.int64)
            assert pulse.phase_taps.dtype == np.uint32 and np.all(np.diff(taps) >= 0) and taps[0] >= 0
            assert int(taps[-1]) == pulse.phase_full
        assert wf.design_cpfsk(U).phase_full == 1 << 30 == wf.design_gmsk(U).phase_full == wf.cpm_pulse("MSK", U).phase_full
        assert wf.design_cpfsk(U, 1).phase_full == 1 << 31 == wf.cpm_pulse("4FSK", U).phase_full
        assert len(wf.design_cpfsk(U).phase_taps) == U and len(wf.design_gmsk(U, span_symbols=3).phase_taps) == 3 * U
    assert list(wf.design_cpfsk(4).phase_taps) == [1 << 28, 2 << 28, 3 << 28, 4 << 28]
    g = wf.design_gmsk(8).phase_taps.astype(np.float64) / (1 << 30)
    assert abs(g[15] - 0.5) < 0.05 and g[3] < 0.01 and g[27] > 0.99         # half the phase at the pulse's middle, flat ends
    for bad in (lambda: wf.design_cpfsk(0), lambda: wf.design_cpfsk(257), lambda: wf.design_cpfsk(8, 2), lambda: wf.design_cpfsk(8, 0),
                lambda: wf.design_gfsk(256, 1, 0.3, 17), lambda: wf.design_gfsk(8, 1, 0.0), lambda: wf.CpmPulse(np.zeros(0, np.uint32), 0),
                lambda: wf.CpmPulse(np.zeros(4, np.uint32), 1 << 32)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("order,U", [(2, 8), (4, 8), (8, 5), (2, 1)])
def test_cpfsk_phase_steps_are_the_values_the_taps_imply(order, U):
    """Sample to sample the phase of a CPFSK row moves by alpha times one tap's worth: M values, each of them taken."""
    pulse = wf.design_cpfsk(U, 1 if order > 2 else Fraction(1, 2))
    phi, _ = ref.phi_computed(SEED, 3, 0, 4000, order, pulse.phase_taps, pulse.phase_full, U, 1, 0)
    steps = np.diff(phi.astype(np.int64)) & ref.M32
    taps = np.concatenate(([0], pulse.phase_taps.astype(np.int64)))
    per_sample = np.unique(np.diff(taps))                                  # the rounding may give two neighbours
    allowed = {(int(a) * int(d)) & ref.M32 for a in range(-(order - 1), order, 2) for d in per_sample}
    assert set(int(s) for s in steps) <= allowed
    if pulse.phase_full % U == 0:
        assert len(per_sample) == 1 and len(set(int(s) for s in steps)) == order


# ---- names, rows, data sets -------------------------------------------------------------------------------------------------------
def test_names_and_rows():
    old = {"BPSK": 2, "QPSK": 4, "8PSK": 8, "16QAM": (1 << 12) | 16, "64QAM": (1 << 12) | 64, "WGN": 2 << 12, "NOISE": 2 << 12}
    for name, code in old.items():
        assert wf.mod_code(name) == code and wf.cpm_order(name) is None, name
    assert wf.mod_code("2FSK") == (3 << 12) | 2 and wf.mod_code("4fsk") == (3 << 12) | 4 and wf.mod_code("256FSK") == (3 << 12) | 256
    assert wf.mod_code("MSK") == (4 << 12) | 2 and wf.mod_code("GMSK") == (5 << 12) | 2
    assert (wf.cpm_order("MSK"), wf.cpm_order("gmsk"), wf.cpm_order("8FSK")) == (2, 2, 8)
    for bad in ("1FSK", "257FSK", "0FSK"):
        with pytest.raises(ValueError):
            wf.cpm_order(bad)
    wf._grid(["MSK", "GMSK", "2FSK", "BPSK"], [0])                         # four names of order 2, four different rows
    with pytest.raises(TypeError):
        wf.generate("GMSK", 1, 8, taps=wf.design_rect(8), compute=ref.numpy_compute)
    with pytest.raises(TypeError):
        wf.generate("BPSK", 1, 8, taps=wf.design_gmsk(8), compute=ref.numpy_compute)
    with pytest.raises(TypeError):
        wf.generate("BPSK", 1, 8, segments=2, compute=ref.numpy_compute)
    with pytest.raises(ValueError):
        wf.generate("MSK", 1, 8, sample_index0=3, compute=ref.numpy_compute)


def test_generate_hands_the_compute_the_pulse_of_the_name():
    seen = []

    def spy(order, taps, full, U, V, R, S, sigma, fpg, **kw):
        seen.append((order, list(taps), full, U, V, R, S, [float(s) for s in sigma], fpg, kw["acc_in"], kw["flags"]))
        return np.zeros((R, S), np.complex64)
    wf.generate("GMSK", 2, 5, sps=(8, 3), snr_db=0, compute=spy)
    wf.generate("4FSK", 2, 5, sps=(2, 1), compute=spy, random_timing=False)
    wf.generate("MSK", 1, 5, sps=(2, 1), taps=wf.design_cpfsk(2, Fraction(1, 4)), compute=spy)
    g = wf.design_gmsk(8)
    assert seen[0] == (2, list(g.phase_taps), 1 << 30, 8, 3, 2, 5, [1.0], 2, None, 3)
    assert seen[1] == (4, [1 << 30, 1 << 31], 1 << 31, 2, 1, 2, 5, [0.0], 2, None, 1)
    assert seen[2][:3] == (2, [1 << 28, 1 << 29], 1 << 29)


def test_cuts_in_rows_and_samples_and_a_stream_equal_one_call_on_the_reference():
    kw = dict(sps=(8, 3), snr_db=7.0, seed=SEED, cfo=0.01, compute=ref.numpy_generate)
    whole = wf.generate("GMSK", 3, 200, row_index0=(1 << 40) + 5, **kw)
    rows = np.concatenate([wf.generate("GMSK", 1, 200, row_index0=(1 << 40) + 5 + f, **kw) for f in range(3)])
    assert np.array_equal(whole, rows)
    acc = np.zeros(3, np.uint32)
    left = wf.generate("GMSK", 3, 77, row_index0=(1 << 40) + 5, acc_out=acc, **kw)
    right = wf.generate("GMSK", 3, 123, row_index0=(1 << 40) + 5, sample_index0=77, acc_in=acc, **kw)
    assert np.array_equal(np.concatenate([left, right], axis=1), whole)
    for chunk in (1, 2, 63):
        s = wf.Stream("4FSK", row=4, sps=(8, 3), snr_db=3.0, seed=SEED, compute=ref.numpy_generate)
        parts = [s.push(min(chunk, 200 - at)) for at in range(0, 200, chunk)]
        assert s.index == 200
        assert np.array_equal(np.concatenate(parts), wf.generate("4FSK", 1, 200, row_index0=4, sps=(8, 3), snr_db=3.0, seed=SEED,
                                                                 compute=ref.numpy_generate)[0])


def test_the_reference_has_unit_envelope_and_msk_walks_the_quarter_turns():
    y, _ = ref.restate(SEED, 1, 0, 500, 2, np.array([1 << 30], np.uint32), 1 << 30, 1, 1, flags=0)
    a = ref.alphas(SEED, 1, np.arange(500), 2)
    assert np.array_equal(y, (1j ** np.cumsum(a)).astype(np.complex64))
    g = wf.design_gmsk(8)
    y, _ = ref.restate(SEED, 2, 0, 2000, 2, g.phase_taps, g.phase_full, 8, 1, cfo_max=1 << 20)
    assert np.abs(np.abs(y.astype(np.complex128)) - 1.0).max() <= 2.5 * np.sqrt(2.0) * 2.0 ** -24


def test_dataset_mixes_linear_and_continuous_names_and_the_command_names_the_pulse(tmp_path):
    import scipy.io
    from amcpy_amd import feature_extraction as fe
    from amcpy_amd.main import build_parser, run_synth, synth_config
    data = wf.dataset(["GMSK", "BPSK"], [0.0, 10.0], 2, 64, sps=(4, 1), seed=4, compute=ref.numpy_compute)
    assert data["GMSK"].shape == (2, 2, 64) and not np.array_equal(data["GMSK"], data["BPSK"])
    one = wf.generate("GMSK", 2, 64, sps=(4, 1), snr_db=10.0, seed=4, row_index0=wf.dataset_row("GMSK", 10.0), compute=ref.numpy_compute)
    assert np.array_equal(data["GMSK"][1], one)
    args = build_parser().parse_args(["synth", "--root", str(tmp_path), "--mods", "BPSK,GMSK", "4FSK", "--sps", "4/1", "--span", "4", "--frames", "3",
                                      "--frame-size", "64", "--snr", "0:10:10", "--seed", "4", "--bt", "0.5", "--cpm-h", "1/2", "--features-only"])
    written = run_synth(args, compute=ref.numpy_compute, features=fake_features)
    assert [p.name for p in written] == ["BPSK_features.mat", "GMSK_features.mat", "4FSK_features.mat"]
    cfg, _ = synth_config(args)
    assert cfg.signals.mat_info["GMSK"] == "signal_gmsk" and cfg.signals.mat_info["4FSK"] == "signal_4fsk" and cfg.signals.mat_info["BPSK"] == "signal_bpsk"
    record = json.loads(fe._provenance_path(written[1]).read_text())
    assert record["cpm"] == {"order": 2, "taps": 16, "phase_full": 1 << 30, "h": "1/2", "bt": 0.5, "span": 4}
    assert json.loads(fe._provenance_path(written[2]).read_text())["cpm"]["phase_full"] == 1 << 30      # --cpm-h 1/2 on the FSK name
    assert "cpm" not in json.loads(fe._provenance_path(written[0]).read_text())
    mat_path = cfg.paths.mat_data / cfg.paths.mat_filename
    assert fe._already_extracted(written[1], "signal_gmsk", (2, 3, 18), fe._provenance(cfg, mat_path, "signal_gmsk"))   # --resume ignores the key
    got = scipy.io.loadmat(str(written[1]))
    assert got["signal_gmsk"].shape == (2, 3, 18) and str(got["Modulation"][0]) == "GMSK"
    want = wf.dataset_features(["GMSK"], [0.0, 10.0], 3, 64, sps=(4, 1), taps=wf.design_gmsk(4, 0.5), seed=4, compute=ref.numpy_compute,
                               features=fake_features)["GMSK"]
    assert np.array_equal(got["signal_gmsk"], want)


def test_train_and_classify_take_the_classes_the_command_named():
    from amcpy_amd.config import SignalConfig, with_modulations
    from amcpy_amd.main import build_parser, split_mods
    sig = with_modulations(SignalConfig(), ["BPSK", "GMSK", "4FSK"])
    assert sig.modulations_with_noise == ("BPSK", "GMSK", "4FSK") and sig.labels == (0, 1, 2) and sig.mat_info["4FSK"] == "signal_4fsk"
    assert sig.mat_info["BPSK"] == "signal_bpsk" and SignalConfig().mat_info.keys() <= sig.mat_info.keys()
    with pytest.raises(ValueError):
        with_modulations(SignalConfig(), ["BPSK", "BPSK"])
    for command in (["train"], ["classify", "--model", "x"], ["quantize", "--model", "x"]):
        assert split_mods(build_parser().parse_args(command + ["--mods", "BPSK,GMSK", "4FSK"]).mods) == ["BPSK", "GMSK", "4FSK"]
        assert build_parser().parse_args(command).mods is None
