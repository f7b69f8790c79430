"""Blind carrier recovery (include/amcx.h, ABI 16.2.3) on the host: the ABI and the tables, the entry's refusals in the header's
order, the plan, the numpy restatement (tests/carrier_ref.py) against a plain float64 version of the same estimator, the integer
words against Python integers, `combine` on hand-made records, and the float64 estimator on the generator's own rows held to
the caps the GPU test holds the kernel to.  Needs no GPU."""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib, carrier, waveform as wf
from tests import carrier_ref as ref, synth_ref

REPO = Path(__file__).resolve().parents[1]
NEW = ["amcx_carrier_c64", "amcx_carrier_plan", "amcx_kernel_name_carrier"]
KERNEL = "amcx_carrier_c64_kernel"
LISTING = "r36_carrier_codeobj_kernels.txt"
# The generator's seed of the end-to-end rows.  The contract sets frac to 0 where |frac| > 0.5: a row whose line stands within a few
# hundredths of a bin of a half bin, and whose noisy interpolation lands beyond 0.5, is then half a bin off (about 3 rows in 64 at
# RRC 2 / 1 and 20 dB under most seeds: 0x5EED5EED1234ABCD has three, 36 two, 2036 one).  Under this seed no row's drawn offset
# lies within 0.04 bin of a half bin of x^4 (0.015 of x^2), and the float64 estimator meets the caps on all 64 rows of each set.
SEED = 2080
SIZES = (64, 128, 256, 512, 1024, 2048, 4096)


def test_abi_16_2_3_in_header_binding_and_library():
    lib = _lib.load()
    assert (_lib.ABI_VERSION, _lib.ABI_MINOR) == (16, 2) == (lib.amcx_abi_version(), lib.amcx_abi_minor())
    assert _lib.ABI_PATCH >= 3 and lib.amcx_abi_patch() >= 3
    header = (REPO / "include" / "amcx.h").read_text()
    assert re.search(r"^#define AMCX_ABI_VERSION 16$", header, re.M) and re.search(r"^#define AMCX_ABI_MINOR 2$", header, re.M)
    assert int(re.search(r"^#define AMCX_ABI_PATCH (\d+)$", header, re.M).group(1)) >= 3
    assert header.index("ABI 16.2.3: AMCX_ABI_PATCH 3") < header.index("ABI 16.2.2: AMCX_ABI_PATCH 2") < \
        header.index("ABI 16.2.1: AMCX_ABI_PATCH 1") < header.index("ABI 16.2: AMCX_ABI_MINOR 2")
    exported = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header) and re.search(rf" T {name}$", exported, re.M), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    flat = " ".join(header.split())
    for prototype in (
            "int amcx_carrier_plan(int32_t n, int32_t* rows_per_workgroup, int32_t* lds_bytes);",
            "int amcx_carrier_c64(const void* in_c64_dev, int64_t n_rows, int32_t n, int64_t in_row_stride, int32_t order, "
            "int32_t search_bins, uint32_t flags, void* est_dev, void* out_c64_dev, int64_t out_row_stride, void* hip_stream);",
            "const char* amcx_kernel_name_carrier(void);"):
        assert prototype in flat, prototype
    for name, value in (("GAIN", 1), ("FREQ", 2), ("PHASE", 4), ("GIVEN", 8)):
        assert re.search(rf"^#define AMCX_CARRIER_{name} {value}u$", header, re.M) and getattr(_lib, "CARRIER_" + name) == value
    assert "M-FOLD AMBIGUITY" in header
    assert _lib.kernel_name_carrier() == KERNEL
    assert np.dtype(_lib.CARRIER_RECORD) == ref.RECORD and ref.RECORD.itemsize == 32 == carrier.RECORD_BYTES
    assert [ref.RECORD.fields[n][1] for n in ref.RECORD.names] == [0, 8, 12, 16, 20, 24, 28]


def test_carrier_kernel_is_in_the_resource_table_without_spill_and_older_kernels_kept_their_bytes():
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    assert table[KERNEL]["spill"] == 0 and table[KERNEL]["scratch"] == 0
    listing = (REPO / "profiles" / LISTING).read_text()
    assert "DIFFERENT" not in listing and "ONLY IN A" not in listing and "103 kernels / device functions identical" in listing
    assert re.findall(r"ONLY IN B\s+amcx::(.+)", listing) == [KERNEL]
    text = (REPO / "amcpy_amd" / "csrc" / "amcx_carrier_kernel.h").read_text()
    code = text[text.index("#pragma once"):]
    assert code.count("__global__") == 1 and "asm" not in code and "atomic" not in code and "persistent_grid(" not in code
    for called in ("psd_pass<4>(", "psd_pass<3>(", "psd_pad(", "psd_mul(", "ddc_mixer("):
        assert called in code, called
    hip = (REPO / "amcpy_amd" / "csrc" / "amcx.hip").read_text()
    assert hip.index('#include "amcx_carrier_kernel.h"') < hip.index('#include "amcx_synth_cpm_kernel.h"')


def test_plan_at_all_seven_sizes():
    for N in SIZES:
        rows, lds = _lib.carrier_plan(N)
        assert rows == 4096 // N and 0 < lds < 65536
    for bad in (0, 32, 63, 65, 96, 8192, -64, 1 << 20):
        with pytest.raises(ValueError):
            _lib.carrier_plan(bad)
    assert _lib.load().amcx_carrier_plan(64, None, None) == _lib.OK


def test_refusals_come_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_carrier_c64
    buf = (C.c_float * 8192)()
    dummy = C.addressof(buf)
    dummy += -dummy % 16
    far = dummy + 16384                                                      # 4 rows of 100 complex64 are 3200 bytes
    ok = dict(inp=dummy, R=4, N=64, istr=100, order=4, sb=4, flags=7, est=dummy, out=far, ostr=100)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["inp"], a["R"], a["N"], a["istr"], a["order"], a["sb"], a["flags"], a["est"], a["out"], a["ostr"], None)

    nothing = dict(R=0, inp=None, est=None, out=None)
    # 1. shapes, ranges and flags, in front of the no-op
    for kw in (dict(N=0), dict(N=32), dict(N=96), dict(N=8192), dict(N=-64), dict(order=0), dict(order=3), dict(order=16), dict(order=-1),
               dict(sb=-1), dict(sb=32), dict(N=4096, istr=4096, ostr=4096, sb=2048), dict(flags=16), dict(flags=0x80000000),
               dict(R=-1), dict(istr=63), dict(R=1 << 30, istr=(1 << 28) + 1)):
        assert call(**kw) == _lib.EINVAL, kw
        assert call(**{**nothing, **kw}) == _lib.EINVAL, kw
    assert call(ostr=63) == _lib.EINVAL and call(R=0, ostr=63) == _lib.EINVAL       # out's stride counts where out is given ...
    assert call(R=0, out=None, ostr=0) == _lib.OK                                   # ... and only there
    assert call(flags=8 | 7, out=None) == _lib.EINVAL and call(flags=8, out=None, R=0) == _lib.EINVAL      # GIVEN needs out
    assert call(sb=31, **nothing) == _lib.OK and call(N=4096, istr=4096, sb=2047, **nothing) == _lib.OK
    # 2. no rows: fine with null pointers
    assert call(**nothing) == _lib.OK and call(R=0) == _lib.OK
    # 3. null pointers, alignment, out overlapping in
    assert call(inp=None) == _lib.EINVAL and call(est=None) == _lib.EINVAL
    assert call(inp=dummy + 4) == _lib.EINVAL and call(est=dummy + 4) == _lib.EINVAL and call(out=far + 4) == _lib.EINVAL
    for out in (dummy, dummy + 8, dummy + 2904, dummy - 2904):                      # three strides and 64 samples: 2912 bytes touched
        assert call(out=out) == _lib.EINVAL, out - dummy
    assert call(R=0, inp=dummy + 4, est=dummy + 2, out=dummy) == _lib.OK           # nothing is read or written


def test_python_layer_refuses_what_the_entry_refuses():
    with pytest.raises(ValueError):
        carrier.search_bins(96)
    with pytest.raises(ValueError):
        carrier.search_bins(64, 3)
    with pytest.raises(ValueError):
        carrier.search_bins(64, 4, -0.1)
    assert [carrier.search_bins(N) for N in SIZES] == [N // 16 for N in SIZES]
    assert carrier.search_bins(2048, 4, 0.004) == 33 and carrier.search_bins(2048, 2, 0.004) == 17
    assert carrier.search_bins(2048, 8, 0.5) == 1023 and carrier.search_bins(64, 1, 0.0) == 0
    with pytest.raises(ValueError):
        carrier.recover_frames(None, dict(search_hz=3.0))
    with pytest.raises(ValueError):
        carrier.recover_frames(None, dict(order=4, per="band"))
    with pytest.raises(ValueError):
        carrier.recover_frames(None, dict(order=4, search_hz=10.0))                  # no sample rate


# ---- the restatement against float64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,order", [(64, 1), (128, 2), (512, 4), (1024, 8), (4096, 4)])
def test_restatement_agrees_with_the_float64_estimator(N, order):
    """bin equal wherever the float64 peak leads the runner-up by 1 % or more; frac within the bound derived in carrier_ref from
    psd_ref's stage bound; the offset and the phase the words encode within what frac's bound and the phase bound allow."""
    R = 48 if N <= 1024 else 12
    sb = N // 16
    x, f = ref.qpsk_rows(R, N, seed=N + order, cfo=0.8 * sb / (order * N), level=37.5)
    got, want = ref.estimate32(x, order, sb), ref.estimate64(x, order, sb)
    rec = got["rec"]
    clear = want["lead"] >= 1.01
    assert clear.sum() >= R // 2
    assert np.array_equal(rec["bin"][clear], want["bin"][clear])
    same = (rec["bin"] == want["bin"]) & ~want["cut"] & (np.abs(want["frac"]) + want["frac_bound"] < 0.5)
    assert same.sum() >= R // 2
    ratio = np.abs(rec["frac"][same].astype(np.float64) - want["frac"][same]) / want["frac_bound"][same]
    print(f"N={N} M={order}: worst |frac32 - frac64| / bound = {ratio.max():.3g} over {same.sum()} rows "
          f"(largest bound {want['frac_bound'][same].max():.3g})")
    assert ratio.max() <= 1.0
    assert np.allclose(rec["power"], want["power"], rtol=1e-5) and np.allclose(rec["gain"], want["power"] ** -0.5, rtol=1e-5)
    # the words say what the float64 estimator says: frac's bound plus the 2^-31 of F, in cycles per sample
    tol = (want["frac_bound"][same] + 2.0 ** -31) / (order * N) + 2.0 ** -60
    assert np.all(np.abs(ref.words_cycles(rec)[same] - want["cycles"][same]) <= tol)
    if order == 4:                                                                   # QPSK through order 4: the line is the carrier
        assert np.all(np.abs(want["cycles"] - f) * order * N <= 0.25)


def test_tree_is_the_pairwise_one_and_fma_any_matches_fma():
    q = np.array([1e8, 1.0, -1e8, 1.0, 3.0, 5.0, 7.0, 9.0], np.float32)
    assert ref.tree32(q) == np.float32(np.float32(np.float32(np.float32(1e8) + np.float32(1)) + np.float32(np.float32(-1e8) + np.float32(1)))
                                       + np.float32(np.float32(8) + np.float32(16)))
    rng = np.random.default_rng(3)
    a, b, c = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    assert np.array_equal(ref.fma32_any(a, b, c), ref.fma32(a, b, c))
    assert np.isinf(ref.fma32_any(np.float32(np.inf), np.float32(1), np.float32(0)))


# ---- the words against Python integers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 4096])
def test_integer_words_against_python_integers(N):
    lg = N.bit_length() - 1
    for order in ref.ORDERS:
        lm = ref.ORDERS.index(order)
        for bin_ in (0, 1, -1, N // 2 - 1, -(N // 2 - 1), 5, -7):
            for frac in (0.0, 0.5, -0.5, 0.25, -0.25, 2.0 ** -31, -(2.0 ** -31), 0.3, -0.3, -1e-12):
                F = ref.frac_word(frac)
                assert F == int(np.rint(float(np.float32(frac)) * 2 ** 31)) and abs(F) <= 1 << 30
                exact = (bin_ * 2 ** 31 + F) * 2 ** (33 - lg)                        # (bin + F 2^-31) / N cycles in 2^-64
                assert -(1 << 63) <= exact < 1 << 63                                 # it fits: no wrap at these limits
                step = ref.step_word(bin_, frac, N, order)
                assert step == exact >> lm == exact // order                         # arithmetic: toward minus infinity
                if exact < 0 and exact % order:
                    assert step != -((-exact) >> lm)                                 # ... which a shift of the magnitude is not
                # numpy int64 does what Python does
                with np.errstate(over="ignore"):
                    as_np = ((np.int64(bin_) << np.int64(64 - lg)) + (np.int64(F) << np.int64(33 - lg))) >> np.int64(lm)
                assert int(as_np) == step
                for w in (0, 1, -1, (1 << 31) - 1, -(1 << 31), 123456789, -987654321):
                    corr = (F * (N - 1)) >> lg
                    assert corr == (F * (N - 1)) // N
                    theta = (w - corr) % (1 << 32)
                    ph = ref.phase_word(w, frac, N, order)
                    assert ph == theta >> lm == theta // order and 0 <= ph < (1 << 32) // order      # logical: of the uint32
    # negative words: the shifts differ exactly where they should
    assert ref.step_word(-1, 0.0, 64, 8) == -(1 << 58) >> 3 and ref.step_word(0, -(2.0 ** -31), 4096, 8) == -(1 << 21) >> 3
    assert ref.phase_word(-1, 0.0, 64, 2) == 0x7FFFFFFF and ref.phase_word(-1, 0.0, 64, 1) == 0xFFFFFFFF
    assert ref.phase0_distance(0, (1 << 30) - 1, 4) == 1 and ref.phase0_distance(5, 9, 1) == 4


def test_phase_words_reproduce_a_planted_tone():
    """A float64 tone at a fractional bin with a known phase: the words of the restatement give its offset within the complex
    interpolator's own bias on a rectangular window, and the output of apply32 is a constant near 1 + 0j."""
    N, order = 1024, 1
    n = np.arange(N)
    for fbin, phase in ((37.3, 0.11), (-12.75, 0.83), (0.4, 0.5), (-0.1, 0.02)):
        x = (0.02 * np.exp(2j * np.pi * (phase + fbin / N * n)))[None, :].astype(np.complex64)
        got = ref.estimate32(x, order, N // 16)
        rec = got["rec"]
        assert abs(ref.words_cycles(rec)[0] * N - fbin) < 1e-3                        # a lone tone: the form is exact but for rounding
        assert min(abs(float(rec["phase0"][0]) * 2.0 ** -32 - phase), 1 - abs(float(rec["phase0"][0]) * 2.0 ** -32 - phase)) < 1e-3
        assert abs(float(rec["power"][0]) - 4e-4) < 1e-9 and rec["quality"][0] > 0.3
        y = ref.apply32(x, rec, ref.GAIN | ref.FREQ | ref.PHASE)
        assert np.abs(y - 1.0).max() < 5e-3
        assert np.array_equal(ref.apply32(x, rec, 0), x)                             # no flag: the product by 1 + 0j changes nothing


# ---- combine ----------------------------------------------------------------------------------------------------------------------
def test_combine_takes_the_group_median_and_keeps_the_phase_at_the_centre():
    N, order = 64, 4
    rec = np.zeros(7, ref.RECORD)
    rec["phase_step"] = [100 << 40, 104 << 40, 90 << 40, -(5 << 40), -(7 << 40), -(6 << 40), 1 << 50]
    rec["phase0"] = [0, 1 << 29, (1 << 30) - 1, 5, 1 << 20, 77, 12345]
    rec["gain"], rec["power"], rec["quality"] = 2.0, 0.25, np.arange(7) / 8.0
    rec["bin"], rec["frac"] = np.arange(7), 0.125
    est = carrier.Estimates.from_numpy(rec, N, order)
    assert np.array_equal(est.numpy(), rec) and len(est) == 7
    assert est.phase_step.tolist() == rec["phase_step"].tolist() and est.phase0.tolist() == rec["phase0"].tolist()
    assert est.bin.tolist() == list(range(7)) and est.gain.tolist() == [2.0] * 7 and est.quality.tolist() == (np.arange(7) / 8.0).tolist()
    assert est.cycles.tolist() == (rec["phase_step"].astype(np.float64) * 2.0 ** -64).tolist()
    groups = [0, 0, 0, 1, 1, 1, 2]
    out = carrier.combine(est, groups).numpy()
    med = {0: 100 << 40, 1: -(6 << 40), 2: 1 << 50}
    for r in range(7):
        m = med[groups[r]]
        assert int(out["phase_step"][r]) == m
        want = ((int(rec["phase0"][r]) << 32) + (((int(rec["phase_step"][r]) - m) * (N - 1)) >> 1)) >> 32
        assert int(out["phase0"][r]) == want % (1 << 30)
    for name in ("bin", "frac", "power", "gain", "quality"):
        assert np.array_equal(out[name], rec[name]), name
    # an int: that many consecutive rows per emitter; an even group takes the lower middle
    out2 = carrier.combine(est, 2).numpy()
    assert out2["phase_step"].tolist() == [100 << 40, 100 << 40, -(5 << 40), -(5 << 40), -(7 << 40), -(7 << 40), 1 << 50]
    with pytest.raises(ValueError):
        carrier.combine(est, [0, 1])
    with pytest.raises(ValueError):
        carrier.combine(est, 0)


# ---- the caps of the end-to-end GPU test, on the generator's own rows in float64 --------------------------------------------------
E2E = [("QPSK", 4, (8, 1), None), ("QPSK", 4, (2, 1), "rrc"), ("BPSK", 2, (8, 1), None)]
E2E_ROWS, E2E_N, E2E_CFO, E2E_SNR = 64, 2048, 0.004, 20.0


def e2e_rows(mod, sps, pulse, cfo, compute=synth_ref.numpy_generate, **kw):
    taps = wf.design_rrc(sps[0]) if pulse == "rrc" else None
    return wf.generate(mod, E2E_ROWS, E2E_N, sps=sps, taps=taps, snr_db=E2E_SNR, cfo=cfo, seed=SEED, compute=compute, **kw)


def drawn_offsets(sps, cfo=E2E_CFO) -> np.ndarray:
    """The offset every row of e2e_rows drew, cycles per sample, from the generator's own row words."""
    steps = [synth_ref.row_params(SEED, r, sps[0], cfo_max=wf.cfo_max_of(cfo))[1] for r in range(E2E_ROWS)]
    return np.array([ref.wrap_i64(s) for s in steps], dtype=np.float64) * 2.0 ** -64


def feature12(x) -> np.ndarray:
    from oracle import iq_features_oracle as orc
    return np.asarray(orc.features18_batch(np.asarray(x).astype(np.complex64)), dtype=np.float64)[:, 11]


@pytest.mark.parametrize("mod,order,sps,pulse", E2E)
def test_float64_estimator_meets_the_end_to_end_caps_on_the_generators_rows(mod, order, sps, pulse):
    x, x0 = e2e_rows(mod, sps, pulse, E2E_CFO), e2e_rows(mod, sps, pulse, 0.0)
    f = drawn_offsets(sps)
    sb = E2E_N // 16
    est = ref.estimate64(x, order, sb)
    err_bins = np.abs(est["cycles"] - f) * order * E2E_N
    far = np.abs(f) * 4 * E2E_N >= 2.0
    assert far.sum() >= E2E_ROWS // 2
    f12_0, f12_raw, f12_rec = feature12(x0), feature12(x), feature12(ref.recover64(x, order, sb))
    print(f"{mod} {sps} {pulse}: worst offset error {err_bins.max():.3f} bin; feature 12 untouched / clean at most "
          f"{(f12_raw[far] / f12_0[far]).max():.3f}; recovered within {np.abs(f12_rec[far] / f12_0[far] - 1).max():.2%}")
    assert err_bins.max() <= 0.25
    assert np.all(f12_raw[far] < 0.5 * f12_0[far])
    assert np.all(np.abs(f12_rec[far] / f12_0[far] - 1.0) <= 0.05)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_synth_features_only_recover_is_named_in_the_provenance_record_and_resume_ignores_it(tmp_path):
    import scipy.io
    from amcpy_amd import feature_extraction as fe
    from amcpy_amd.main import build_parser, run_synth
    from tests.test_synth_host import fake_features
    base = ["synth", "--root", str(tmp_path), "--mods", "QPSK", "--sps", "4/1", "--pulse", "rect", "--frames", "3", "--frame-size", "64",
            "--snr", "10:20:10", "--seed", "4", "--cfo", "0.002"]
    seen = []

    def recover_compute(x, recover):
        seen.append(dict(recover))
        return ref.recover64(x, recover["order"], x.shape[1] // 16).astype(np.complex64)

    args = build_parser().parse_args(base + ["--features-only", "--recover", "4"])
    written = run_synth(args, compute=synth_ref.numpy_generate, features=fake_features, recover_compute=recover_compute)
    assert [p.name for p in written] == ["QPSK_features.mat"] and seen and all(s == {"order": 4} for s in seen)
    record = json.loads(fe._provenance_path(written[0]).read_text())
    assert record["recover"] == {"order": 4}
    from amcpy_amd.main import synth_config
    cfg, _ = synth_config(args)
    mat_path = cfg.paths.mat_data / cfg.paths.mat_filename
    var = cfg.signals.mat_info["QPSK"]
    assert fe._already_extracted(written[0], var, (2, 3, 18), fe._provenance(cfg, mat_path, var))           # --resume ignores the key
    got = scipy.io.loadmat(str(written[0]))[var]
    assert np.all((got > 0.95) & (got <= 1.0 + 1e-6))            # fake_features is mean |x| <= sqrt(mean |x|^2), which recovery made 1
    plain = run_synth(build_parser().parse_args(base + ["--features-only"]), compute=synth_ref.numpy_generate, features=fake_features)
    assert "recover" not in json.loads(fe._provenance_path(plain[0]).read_text())
    with pytest.raises(SystemExit):
        run_synth(build_parser().parse_args(base + ["--recover", "4"]), compute=synth_ref.numpy_generate, features=fake_features)
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--features-only", "--recover", "3"])


def test_recording_recover_flags_are_parsed_and_need_the_tuning_flags(tmp_path):
    from amcpy_amd.main import build_parser, run_recording
    ap = build_parser()
    a = ap.parse_args(["recording", "x.sigmf-meta", "--frame-size", "2048", "--shift-hz=-1e3", "--decimate", "8", "--recover", "4",
                       "--recover-search-hz", "500"])
    assert a.recover == 4 and a.recover_search_hz == 500.0
    assert ap.parse_args(["recording", "x.sigmf-meta", "--frame-size", "2048"]).recover is None
    with pytest.raises(SystemExit):
        ap.parse_args(["recording", "x.sigmf-meta", "--frame-size", "2048", "--recover", "16"])
    with pytest.raises(SystemExit, match="--recover needs the tuning flags"):
        run_recording(ap.parse_args(["recording", str(tmp_path / "x.sigmf-meta"), "--frame-size", "2048", "--recover", "4"]))
    with pytest.raises(SystemExit, match="--recover-search-hz needs --recover"):
        run_recording(ap.parse_args(["recording", str(tmp_path / "x.sigmf-meta"), "--frame-size", "2048", "--recover-search-hz", "5"]))
    from amcpy_amd import sigmf
    (tmp_path / "none.sigmf-data").write_bytes(np.zeros(4096, np.complex64).tobytes())
    (tmp_path / "none.sigmf-meta").write_text(json.dumps({"global": {"core:datatype": "cf32_le", "core:version": "1.0.0"},
                                                          "captures": [{"core:sample_start": 0}], "annotations": []}))
    with pytest.raises(TypeError):                                   # the signature is the parent's: recover is a key of the tune dict
        sigmf.extract_sigmf(tmp_path / "none", 2048, recover=dict(order=4))
    with pytest.raises(ValueError, match="recover runs on the device"):
        sigmf.extract_sigmf(tmp_path / "none", 2048, tune=dict(shift_hz=0.0, decimate=1, taps=1, recover=dict(order=4)),
                            tune_compute=lambda *a, **k: None, compute=lambda x: np.zeros((len(x), 18), np.float32))
    import inspect
    assert "recover" not in inspect.signature(sigmf.extract_sigmf).parameters
