"""The waveform generator (include/amcx.h, ABI 16.2) on the host: the ABI and the resource table, the entry's refusals in the
header's order, the integers and the statistics of the numpy reference (tests/synth_ref.py), the pulse designers, the rows of a
data set and the `synth` command over the injected numpy compute.  Needs no GPU."""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib, waveform as wf
from tests import synth_ref as ref

REPO = Path(__file__).resolve().parents[1]
NEW = ["amcx_synth_c64", "amcx_synth_plan", "amcx_kernel_name_synth", "amcx_abi_minor"]
SEED = 0x5EED5EED1234ABCD          # of every statistic below: a constant
N_NOISE, N_SYMBOLS = 1 << 20, 1 << 16
ORDERS = (2, 3, 64, 255, 256)


def test_abi_16_2_in_header_binding_and_library():
    lib = _lib.load()
    assert (_lib.ABI_VERSION, _lib.ABI_MINOR) == (16, 2) and (lib.amcx_abi_version(), lib.amcx_abi_minor()) == (16, 2)
    header = (REPO / "include" / "amcx.h").read_text()
    assert re.search(r"^#define AMCX_ABI_VERSION 16$", header, re.M) and re.search(r"^#define AMCX_ABI_MINOR 2$", header, re.M)
    assert header.index("ABI 16.2: AMCX_ABI_MINOR 2") < header.index("ABI 16.1: AMCX_ABI_MINOR 1") < header.index("ABI 16: the line above")
    assert "#define AMCX_SYNTH_RANDOM_PHASE 1u" in header and "#define AMCX_SYNTH_RANDOM_TIMING 2u" in header
    assert (_lib.SYNTH_RANDOM_PHASE, _lib.SYNTH_RANDOM_TIMING) == (1, 2) == (ref.RANDOM_PHASE, ref.RANDOM_TIMING)
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header) and re.search(rf" T {name}$", exported, re.M), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    flat = " ".join(header.split())
    assert ("int amcx_synth_c64(uint64_t seed, uint64_t row_index0, int64_t sample_index0, int64_t n_rows, int64_t row_samples, "
            "int64_t row_stride, const void* table_c64_dev, int32_t order, const float* taps_dev, int32_t n_taps, int32_t up, "
            "int32_t down, int32_t tau0, uint64_t phase_step, uint32_t cfo_max, uint32_t flags, const float* sigma_dev, "
            "int64_t frames_per_group, void* out_c64_dev, void* hip_stream);") in flat
    assert _lib.kernel_name_synth() == "amcx_synth_c64_kernel"


def test_synth_kernel_is_in_the_resource_table_without_spill_and_older_kernels_kept_their_bytes():
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    assert table["amcx_synth_c64_kernel"]["spill"] == 0 and table["amcx_synth_c64_kernel"]["scratch"] == 0
    listing = (REPO / "profiles" / "r28_synth_codeobj_kernels.txt").read_text()
    assert "DIFFERENT" not in listing and "ONLY IN A" not in listing and "100 kernels / device functions identical" in listing
    assert re.findall(r"ONLY IN B\s+amcx::(.+)", listing) == ["amcx_synth_c64_kernel"]


def test_sharing_the_polyphase_routines_left_every_kernel_its_bytes():
    """amcx_polyphase.h (the tap image, the sum and the plan arithmetic the generator and the resampler now both call): the parent
    commit's library against the tree's, per kernel."""
    listing = (REPO / "profiles" / "r29_polyphase_codeobj_kernels.txt").read_text()
    assert "101 kernels / device functions identical" in listing
    assert "DIFFERENT" not in listing and "ONLY IN A" not in listing and "ONLY IN B" not in listing
    csrc = REPO / "amcpy_amd" / "csrc"
    assert "__global__" not in (csrc / "amcx_polyphase.h").read_text()
    for header in ("amcx_synth_kernel.h", "amcx_resample_kernel.h"):
        text = (csrc / header).read_text()
        assert "poly_stage_taps(" in text and "poly_taps_sum(" in text and "__builtin_fmaf" not in text, header
    assert '#include "amcx_resample_kernel.h"' not in (csrc / "amcx_synth_kernel.h").read_text()


PLAN_SWEEP = [(1, 1, 1), (1, 256, 1), (4096, 1, 4096), (4096, 256, 1), (4095, 7, 4096), (4096, 1, 1), (8, 8, 1), (33, 2, 1),
              (129, 8, 3), (4096, 256, 255), (7, 3, 4096), (4096, 255, 256), (4081, 255, 1), (2, 3, 50)]


@pytest.mark.parametrize("T,U,V", PLAN_SWEEP)
def test_plan_spans_fit_for_every_phase(T, U, V):
    """Every tile -- every tau and every remainder a tile can begin at -- needs at most the symbols the stage holds, by brute
    force over the definition; the LDS stays under the 64 KiB that need no attribute, with the largest table."""
    tile, lds, grid = _lib.synth_plan(256, T, U, V)
    P = -(-T // U)
    assert 1 <= tile <= 4096 and (tile == 1 or tile % 2 == 0) and grid >= 1 and lds <= 65536
    tau = np.arange(U, dtype=np.int64)[:, None]
    k = np.arange(2 * U, dtype=np.int64)[None, :]                          # odd and even first samples, every remainder
    t_first = k * tile * V + tau
    span = ((P - 1) + (t_first + (tile - 1) * V) // U) - t_first // U + 1
    assert int(span.max()) <= 5120
    assert lds >= 8 * int(span.max()) + 4 * T + 8 * 256
    assert _lib.synth_plan(0, T, U, V)[1] == lds - 8 * 256
    for bad in ((-1, T, U, V), (257, T, U, V), (4, 0, U, V), (4, 4097, U, V), (4, T, 0, V), (4, T, 257, V), (4, T, U, 0), (4, T, U, 4097)):
        with pytest.raises(ValueError):
            _lib.synth_plan(*bad)


def test_refusals_come_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_synth_c64
    buf = (C.c_float * 256)()
    dummy = C.addressof(buf)
    dummy += -dummy % 16
    ok = dict(i0=0, R=4, S=100, stride=100, table=dummy, order=4, taps=dummy, T=5, U=2, V=3, tau0=0, flags=3, sigma=dummy, fpg=1, out=dummy)

    def call(**kw):
        a = {**ok, **kw}
        return f(1, 0, a["i0"], a["R"], a["S"], a["stride"], a["table"], a["order"], a["taps"], a["T"], a["U"], a["V"], a["tau0"], 0, 0,
                 a["flags"], a["sigma"], a["fpg"], a["out"], None)

    nothing = dict(R=0, table=None, taps=None, sigma=None, out=None)
    # 1. ranges, in front of the no-op: the shape, tau0 and the flags, the row's samples, the rows, the groups
    for kw in (dict(order=-1), dict(order=257), dict(U=0), dict(U=257), dict(V=0), dict(V=4097), dict(T=0), dict(T=4097),
               dict(tau0=-1), dict(tau0=2), dict(flags=4), dict(flags=7),
               dict(S=0, stride=0), dict(i0=-1), dict(i0=(1 << 40) - 100), dict(S=1 << 40, stride=1 << 40, R=1),
               dict(R=-1), dict(stride=99), dict(R=1 << 30, stride=(1 << 28) + 1), dict(fpg=0), dict(fpg=-3)):
        assert call(**kw) == _lib.EINVAL, kw
        assert call(**{**nothing, **kw}) == _lib.EINVAL, kw
    assert call(i0=(1 << 40) - 101, **{k: v for k, v in nothing.items()}) == _lib.OK          # the last sample is 2^40 - 2
    # 2. no rows: fine with null pointers
    assert call(**nothing) == _lib.OK and call(R=0) == _lib.OK
    # 3. null pointers (the table only where there are symbols), then alignment
    for key in ("out", "taps", "sigma", "table"):
        assert call(**{key: None}) == _lib.EINVAL, key
    assert call(out=dummy + 4) == _lib.EINVAL and call(taps=dummy + 2) == _lib.EINVAL
    assert call(table=dummy + 2) == _lib.EINVAL and call(sigma=dummy + 1) == _lib.EINVAL
    assert call(order=0, table=None, out=dummy + 4) == _lib.EINVAL                             # ... still the other pointers'
    assert call(R=0, out=dummy + 4, taps=dummy + 2) == _lib.OK                                 # nothing is read or written


# ---- the reference's integers -----------------------------------------------------------------------------------------------------
def test_counter_layout_and_key():
    """counter(s, j, r) = (j low, (s << 28) | (j >> 32), r low, r high), key = the seed's two words: against Philox called by hand."""
    from tests.train_ref import philox4x32_10
    seed, r, j = (7 << 32) | 5, (3 << 32) | 9, (11 << 32) | 13
    want = philox4x32_10((13, (2 << 28) | 11, 9, 3), (5, 7))
    got = ref.words(seed, ref.STREAM_NOISE, np.array([j], dtype=np.uint64), r)
    assert [int(w[0]) for w in got] == [int(w) for w in want]
    w1, w2 = ref.noise_words(seed, r, np.array([2 * j, 2 * j + 1]))
    assert [int(w1[0]), int(w2[0]), int(w1[1]), int(w2[1])] == [int(w) for w in want]
    sym = philox4x32_10((13, (1 << 28) | 11, 9, 3), (5, 7))
    idx = ref.symbol_indices(seed, r, np.array([4 * j + c for c in range(4)]), 64)
    assert idx.tolist() == [(int(w) * 64) >> 32 for w in sym]
    W = [int(w) for w in philox4x32_10((0, 0, 9, 3), (5, 7))]
    phase0, step, tau = ref.row_params(seed, r, 8, phase_step=100, cfo_max=1000)
    w1s = W[1] - (1 << 32) if W[1] >= 1 << 31 else W[1]
    assert (phase0, step, tau) == (W[0] << 32, (100 + w1s * 1000) % (1 << 64), (W[2] * 8) >> 32)
    assert ref.row_params(seed, r, 8, phase_step=100, flags=0, tau0=5) == (0, 100, 5)


def test_reference_integers_stay_in_range():
    k = np.arange(N_SYMBOLS)
    for order in ORDERS:
        idx = ref.symbol_indices(SEED, 3, k, order)
        assert idx.min() >= 0 and idx.max() < order and idx.max() == order - 1
    assert ref.mulhi32(0xFFFFFFFF, 256) == 255 and ref.mulhi32(0, 256) == 0 and ref.mulhi32(0xFFFFFFFF, 3) == 2
    for U in (1, 2, 3, 255, 256):
        taus = [ref.row_params(SEED, r, U)[2] for r in range(200)]
        assert 0 <= min(taus) and max(taus) < U and (U == 1 or len(set(taus)) > 1)
    w1, _ = ref.noise_words(SEED, 1, np.arange(N_NOISE))
    u = ref.uniform_of(w1)
    assert u.min() > 0.0 and u.max() <= 1.0 and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert ref.uniform_of(np.array([0xFF], dtype=np.uint64))[0] == 2.0 ** -24 and ref.uniform_of(np.array([0xFFFFFFFF], dtype=np.uint64))[0] == 1.0


def noise_statistics_ok(z, sigma):
    """mean, variance and fourth moment of both components within 5 standard errors of a complex Gaussian's of power sigma^2
    (a component's variance s = sigma^2 / 2: var of x^2 is 2 s^2, of x^4 is 96 s^4)"""
    n, s = z.shape[0], sigma * sigma / 2.0
    for x in (z.real.astype(np.float64), z.imag.astype(np.float64)):
        assert abs(x.mean()) <= 5 * np.sqrt(s / n)
        assert abs((x * x).mean() - s) <= 5 * np.sqrt(2.0 / n) * s
        assert abs((x ** 4).mean() - 3 * s * s) <= 5 * np.sqrt(96.0 / n) * s * s
    assert abs((z.real.astype(np.float64) * z.imag.astype(np.float64)).mean()) <= 5 * s / np.sqrt(n)


def histogram_ok(idx, order):
    n = idx.shape[0]
    counts = np.bincount(idx, minlength=order)
    assert counts.shape[0] == order
    assert np.abs(counts - n / order).max() <= 5 * np.sqrt(n * (1.0 / order) * (1 - 1.0 / order))


def test_reference_statistics():
    """Checked on the reference first, so that the GPU test's caps are ones the reference alone meets."""
    z, _ = ref.noise64(SEED, 0, np.arange(N_NOISE), 0.5)
    noise_statistics_ok(z, 0.5)
    for order in ORDERS:
        histogram_ok(ref.symbol_indices(SEED, order, np.arange(N_SYMBOLS), order), order)


def test_B_is_what_the_docstring_derives():
    assert ref.B_NOISE == 9.0 and 3 + 1 + 1 + 2.5 + 1 <= ref.B_NOISE


# ---- the designers ---------------------------------------------------------------------------------------------------------------
def test_designers_have_unit_symbol_energy():
    for U in (1, 2, 3, 8, 64, 255):
        g = wf.design_rrc(U, 16)
        assert g.dtype == np.float32 and g.shape == (16 * U + 1,) and np.array_equal(g, g[::-1])
        # T roundings to float32, each within 2^-24 relative of a tap: sum g^2 moves by at most 2^-23 sum g^2
        assert abs(float((g.astype(np.float64) ** 2).sum()) - U) <= 2.0 ** -22 * U
        r = wf.design_rect(U)
        assert r.dtype == np.float32 and r.tolist() == [1.0] * U
    assert wf.design_rrc(255, 16).shape == (4081,)
    for bad in (lambda: wf.design_rrc(256, 16), lambda: wf.design_rrc(8, 512), lambda: wf.design_rrc(8, 16, 0.0), lambda: wf.design_rect(257)):
        with pytest.raises(ValueError):
            bad()


def test_rrc_matched_cascade_has_little_intersymbol_interference():
    """g * g sampled once per symbol: the raised cosine's zero crossings.  Truncated to +-8 symbols at beta = 0.35 the textbook
    figure is an ISI below -40 dB: the pulse's tails fall as 1 / t^2 and what is cut off beyond 8 symbols is under 1 % in sum."""
    g = wf.design_rrc(2, 16, 0.35).astype(np.float64)
    h = np.convolve(g, g) / 2.0
    mid = h.shape[0] // 2
    at_symbols = h[mid % 2::2]
    main = h[mid]
    others = np.delete(at_symbols, np.argmax(np.abs(at_symbols)))
    assert abs(main - 1.0) <= 1e-6
    assert np.abs(others).sum() <= 0.01 and (others ** 2).sum() <= 1e-4


def test_constellation_tables():
    for mod, order in (("BPSK", 2), ("QPSK", 4), ("8PSK", 8), ("16QAM", 16), ("64QAM", 64), ("256QAM", 256)):
        t = wf.constellation_table(mod)
        assert t.dtype == np.complex64 and t.shape == (order,) and abs(float((np.abs(t.astype(np.complex128)) ** 2).mean()) - 1) < 1e-6
    assert wf.constellation_table("WGN").shape == (0,)


# ---- data sets ------------------------------------------------------------------------------------------------------------------
def test_dataset_rows_are_the_same_for_every_subset():
    kw = dict(sps=(2, 1), taps=wf.design_rrc(2, 4), seed=9, cfo=0.01, compute=ref.numpy_generate)
    full = wf.dataset(["BPSK", "16QAM", "WGN"], [0.0, 6.0, 12.5], 3, 40, **kw)
    assert set(full) == {"BPSK", "16QAM", "WGN"} and full["BPSK"].shape == (3, 3, 40) and full["BPSK"].dtype == np.complex64
    part = wf.dataset(["16QAM"], [12.5, 0.0], 2, 40, **kw)
    assert np.array_equal(part["16QAM"][0], full["16QAM"][2, :2]) and np.array_equal(part["16QAM"][1], full["16QAM"][0, :2])
    later = wf.dataset(["WGN"], [6.0], 1, 40, first_frame=2, **kw)
    assert np.array_equal(later["WGN"][0, 0], full["WGN"][1, 2])
    rows = {wf.dataset_row(m, s, f) for m in ("BPSK", "QPSK", "8PSK", "16QAM", "64QAM", "WGN") for s in (-10.0, 0.0, 0.125, 30.0) for f in (0, 1, 999)}
    assert len(rows) == 6 * 4 * 3 and max(rows) < 1 << 64
    assert not np.array_equal(full["BPSK"][0, 0], full["BPSK"][0, 1]) and not np.array_equal(full["BPSK"][0, 0], full["BPSK"][1, 0])
    # noise of unit power for the noise class, whatever the label
    assert abs(float((np.abs(wf.dataset(["WGN"], [20.0], 8, 512, **kw)["WGN"]) ** 2).mean()) - 1.0) < 0.1


def test_dataset_refuses_two_names_for_the_same_rows():
    kw = dict(sps=(2, 1), taps=wf.design_rrc(2, 4), compute=ref.numpy_generate)
    assert wf.snr_code(3.0) == wf.snr_code(3.05) != wf.snr_code(3.125) and wf.mod_code("8PSK") != wf.mod_code("16PSK") != wf.mod_code("16QAM")
    for mods, snrs in ((["BPSK"], [3.0, 3.05]), (["BPSK"], [1.0, 2.0, 1.0]), (["BPSK", "QPSK", "bpsk"], [0.0]), (["WGN", "NOISE"], [0.0])):
        with pytest.raises(ValueError, match="same rows"):
            wf.dataset(mods, snrs, 1, 16, **kw)
        with pytest.raises(ValueError, match="same rows"):
            wf.dataset_features(mods, snrs, 1, 16, features=fake_features, **kw)
    assert wf.dataset(["BPSK"], [3.0, 3.125], 1, 16, **kw)["BPSK"].shape == (2, 1, 16)


def test_generate_cut_in_rows_and_samples_equals_one_call_on_the_reference():
    kw = dict(sps=(8, 3), taps=wf.design_rrc(8, 4), seed=3, cfo=0.01, compute=ref.numpy_generate)
    whole = wf.generate("QPSK", 3, 50, snr_db=[10.0, 0.0, 5.0], row_index0=1 << 33, **kw)
    rows = np.concatenate([wf.generate("QPSK", 1, 50, snr_db=[10.0], row_index0=1 << 33, **kw),
                           wf.generate("QPSK", 2, 50, snr_db=[0.0, 5.0], row_index0=(1 << 33) + 1, **kw)])
    assert np.array_equal(whole, rows)
    s = wf.Stream("QPSK", row=(1 << 33) + 1, snr_db=0.0, **kw)
    assert np.array_equal(np.concatenate([s.push(n) for n in (1, 0, 7, 42)]), whole[1]) and s.index == 50
    with pytest.raises(ValueError):
        wf.generate("QPSK", 3, 50, snr_db=[1.0, 2.0], frames_per_group=1, **kw)
    with pytest.raises(ValueError):
        wf.generate("QPSK", 1, 50, cfo=0.5, compute=ref.numpy_generate)


# ---- one operand path, one walk: the data set, its features and the stream over the injected compute ---------------------------------
WALK_MODS, WALK_SNRS, WALK_F, WALK_N = ["BPSK", "WGN"], [0.0, 10.0], 5, 64


def walk_kw(compute=ref.numpy_generate):
    return dict(sps=(2, 1), taps=wf.design_rrc(2, 4), seed=11, cfo=0.01, compute=compute)


def sample_features(x):
    """18 columns that tell frames and samples apart: the first nine samples of every frame, real parts then imaginary parts"""
    x = np.asarray(x)
    return np.concatenate([x[:, :9].real, x[:, :9].imag], axis=1).astype(np.float32)


def test_dataset_features_in_chunks_are_the_features_of_the_dataset_s_frames():
    data = wf.dataset(WALK_MODS, WALK_SNRS, WALK_F, WALK_N, **walk_kw())
    feats = wf.dataset_features(WALK_MODS, WALK_SNRS, WALK_F, WALK_N, chunk_frames=2, features=sample_features, **walk_kw())
    assert list(feats) == list(data) == WALK_MODS
    for mod in WALK_MODS:
        assert data[mod].shape == (2, WALK_F, WALK_N) and data[mod].dtype == np.complex64
        want = np.stack([sample_features(data[mod][s]) for s in range(len(WALK_SNRS))])
        assert feats[mod].dtype == np.float32 and feats[mod].shape == (2, WALK_F, 18) and feats[mod].tobytes() == want.tobytes()
    assert data["BPSK"][0].tobytes() != data["BPSK"][1].tobytes() and np.abs(data["WGN"]).max() > 0
    whole = wf.dataset_features(WALK_MODS, WALK_SNRS, WALK_F, WALK_N, features=sample_features, **walk_kw())
    assert all(whole[mod].tobytes() == feats[mod].tobytes() for mod in WALK_MODS)


def test_stream_in_chunks_equals_one_call():
    for mod, noise in (("BPSK", dict(snr_db=10.0)), ("WGN", dict(snr_db=0.0)), ("BPSK", dict(sigma=0.25)), ("BPSK", {})):
        whole = wf.generate(mod, 1, WALK_N, row_index0=7, **noise, **walk_kw())
        s = wf.Stream(mod, row=7, **noise, **walk_kw())
        chunks = [s.push(n) for n in (3, 0, 61)]
        assert [c.shape for c in chunks] == [(3,), (0,), (61,)] and all(c.dtype == np.complex64 for c in chunks) and s.index == WALK_N
        assert np.concatenate(chunks).tobytes() == whole[0].tobytes()


def test_dataset_hands_the_compute_what_generate_by_name_hands_it():
    """The table, the taps, the sigmas and frames_per_group (and every other argument) an injected compute receives from the
    data set's walk, which passes the table and one resident sigma, against those of generate(mod, snr_db=snr) called directly."""
    calls = []

    def recording(table, taps, U, V, n_rows, row_samples, sigma, frames_per_group, **where):
        calls.append((None if table is None else np.array(table), np.array(taps), (U, V, n_rows, row_samples), np.array(sigma),
                      frames_per_group, dict(where)))
        return ref.numpy_generate(table, taps, U, V, n_rows, row_samples, sigma, frames_per_group, **where)

    wf.dataset(WALK_MODS, WALK_SNRS, WALK_F, WALK_N, first_frame=3, **walk_kw(recording))
    walked, calls[:] = list(calls), []
    for mod in WALK_MODS:
        for snr in WALK_SNRS:
            wf.generate(mod, WALK_F, WALK_N, snr_db=snr, row_index0=wf.dataset_row(mod, snr, 3), **walk_kw(recording))
    assert len(walked) == len(calls) == len(WALK_MODS) * len(WALK_SNRS)                      # one call per (modulation, SNR)
    for got, want in zip(walked, calls):
        for g, w in zip(got[:2] + got[3:4], want[:2] + want[3:4]):                           # table, taps, sigma
            assert (g is None and w is None) or (g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes())
        assert got[2] == want[2] and got[4] == want[4] == WALK_F and got[5] == want[5]
    assert walked[0][0].shape == (2,) and walked[2][0] is None and walked[2][3].tolist() == [1.0] and walked[3][3].tolist() == [1.0]
    assert walked[1][3].tolist() == wf.sigma_of(10.0).tolist() and walked[0][5]["row_index0"] == wf.dataset_row("BPSK", 0.0, 3)


# ---- the command -----------------------------------------------------------------------------------------------------------------
def fake_features(x):
    x = np.asarray(x)
    return np.repeat(np.abs(x).mean(axis=1, keepdims=True), 18, axis=1).astype(np.float32)


def synth_args(root, *more):
    from amcpy_amd.main import build_parser
    return build_parser().parse_args(["synth", "--root", str(root), "--mods", "BPSK", "WGN", "--sps", "2/1", "--span", "4", "--frames", "3",
                                      "--frame-size", "64", "--snr", "0:10:10", "--seed", "4", *more])


def test_synth_command_writes_the_container(tmp_path):
    import scipy.io
    from amcpy_amd.main import run_synth, synth_config
    args = synth_args(tmp_path, "--cfo", "0.01")
    assert (args.command, args.pulse, args.beta, args.features_only, args.device) == ("synth", "rrc", 0.35, False, None)
    written = run_synth(args, compute=ref.numpy_generate)
    cfg, snr = synth_config(args)
    assert written == [tmp_path / "mat-data" / "all_modulations.mat"] and snr == [0.0, 10.0] and cfg.signals.snr_values == {0: "0", 1: "10"}
    mat = scipy.io.loadmat(str(written[0]))
    assert {k for k in mat if not k.startswith("__")} == {"signal_bpsk", "signal_noise"}
    for key in ("signal_bpsk", "signal_noise"):
        assert mat[key].shape == (2, 3, 64) and mat[key].dtype == np.complex64
    want = wf.dataset(["BPSK"], [0.0, 10.0], 3, 64, sps=(2, 1), taps=wf.design_rrc(2, 4), seed=4, cfo=0.01, compute=ref.numpy_generate)
    assert np.array_equal(mat["signal_bpsk"], want["BPSK"])
    assert wf.parse_snr("-10:20:2") == [float(v) for v in range(-10, 21, 2)] and wf.parse_sps("8/3") == (8, 3) and wf.parse_sps("4") == (4, 1)


def test_synth_features_only_files_are_what_resume_trusts(tmp_path):
    import scipy.io
    from amcpy_amd import feature_extraction as fe
    from amcpy_amd.main import run_synth, synth_config
    args = synth_args(tmp_path, "--features-only")
    written = run_synth(args, compute=ref.numpy_generate, features=fake_features)
    cfg, _ = synth_config(args)
    assert [p.name for p in written] == ["BPSK_features.mat", "WGN_features.mat"] and not (tmp_path / "mat-data" / "all_modulations.mat").exists()
    mat_path = cfg.paths.mat_data / cfg.paths.mat_filename
    for mod, path in zip(("BPSK", "WGN"), written):
        key = cfg.signals.mat_info[mod]
        assert fe._already_extracted(path, key, (2, 3, 18), fe._provenance(cfg, mat_path, key))
        got = scipy.io.loadmat(str(path))
        assert got[key].dtype == np.float32 and got[key].shape == (2, 3, 18) and str(got["Modulation"][0]) == mod
    assert fe._modulations_to_do(cfg, mat_path, 0, 1, True, None, False) == [m for m in cfg.signals.modulations_with_noise if m not in ("BPSK", "WGN")]
    # another frame size is another data set: not trusted
    other, _ = synth_config(synth_args(tmp_path, "--features-only", "--frame-size", "128"))
    assert not fe._already_extracted(written[0], "signal_bpsk", (2, 3, 18), fe._provenance(other, mat_path, "signal_bpsk"))


def test_synth_refuses_a_container_above_two_gib(tmp_path):
    from amcpy_amd.main import build_parser, run_synth
    args = build_parser().parse_args(["synth", "--root", str(tmp_path), "--frames", "1000", "--frame-size", "4096"])
    with pytest.raises(SystemExit) as e:
        run_synth(args, compute=ref.numpy_generate)
    text = str(e.value)
    assert "--features-only" in text and "16 x 1000 x 4096" in text and str(6 * 16 * 1000 * 4096 * 8) in text
    assert not (tmp_path / "mat-data" / "all_modulations.mat").exists()
