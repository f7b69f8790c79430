"""The Welch spectrogram and the scan of a recording (include/amcx.h, ABI 15) on the host: the new symbols and their argument
checks in the order the header states, the row count, the numpy restatement of the kernel's operation sequence against the
float64 definition, the streaming class over ragged cuts, bands and emitters on hand-made masks, and the scan of a synthetic
two-capture SigMF recording over injected numpy computes with the annotation round trip.  Needs no GPU."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from amcpy_amd import _lib, occupancy, psd
from tests import psd_ref as ref
from tests.stream_inputs import aligned as _aligned

REPO = Path(__file__).resolve().parents[1]
NEW = ["amcx_spectrogram_out_rows", "amcx_spectrogram", "amcx_spectrogram_plan", "amcx_psd_detect_f32", "amcx_kernel_name_psd",
       "amcx_kernel_name_psd_detect"]
KERNELS = ["amcx_spectrogram_c64_kernel", "amcx_spectrogram_sc16_kernel", "amcx_spectrogram_iq8_kernel", "amcx_psd_detect_kernel"]


def test_abi_15_symbols_exist_and_bind():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 15 and lib.amcx_abi_version() >= 15
    header = (REPO / "include" / "amcx.h").read_text()
    assert "#define AMCX_ABI_VERSION 15" in header
    lines = [header.index(f"#define AMCX_ABI_VERSION {v}") for v in (15, 14, 13, 12, 11, 10)]
    assert lines == sorted(lines)                                            # the live one first, the older lines kept
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    flat = " ".join(header.split())
    assert "int64_t amcx_spectrogram_out_rows(int64_t n_samples, int32_t nfft, int32_t hop, int32_t averages);" in flat
    assert ("int amcx_spectrogram(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, const float* window_dev, "
            "int32_t nfft, int32_t hop, int32_t averages, float* psd_dev, int64_t row_stride, int64_t n_rows, void* hip_stream);") in flat
    assert ("int amcx_spectrogram_plan(int32_t nfft, int32_t hop, int32_t averages, int32_t* segments_per_pass, "
            "int32_t* lds_bytes, int32_t* max_workgroups);") in flat
    assert ("int amcx_psd_detect_f32(const float* psd_dev, int64_t n_rows, int32_t bins, int64_t row_stride, int32_t floor_rank, "
            "float threshold, float* floor_dev, uint8_t* mask_dev, void* hip_stream);") in flat
    assert "int amcx_kernel_name_psd(int32_t src_kind, char* buf, int32_t buf_len);" in flat
    assert "const char* amcx_kernel_name_psd_detect(void);" in flat
    names = [_lib.kernel_name_psd(k) for k in (_lib.SRC_C64, _lib.SRC_SC16, _lib.SRC_CI8, _lib.SRC_CU8)]
    assert names == [KERNELS[0], KERNELS[1], KERNELS[2], KERNELS[2]] and _lib.kernel_name_psd_detect() == KERNELS[3]
    for kind in (-1, 1, 5, 10):
        with pytest.raises(ValueError):
            _lib.kernel_name_psd(kind)
    assert [_lib.kernel_name_occupancy(i) for i in range(6)][-1] == "amcx_occupancy_scatter_kernel"      # its range stays 0 ... 5
    with pytest.raises(ValueError):
        _lib.kernel_name_occupancy(6)
    # the committed resource table knows the kernels by the names the queries give: nothing spilled, LDS below 64 KiB
    table = json.loads((REPO / "amcpy_amd" / "csrc" / "kernel_resources.json").read_text())
    for name in KERNELS:
        assert table[name]["spill"] == 0 and table[name]["scratch"] == 0, name
    # the per-kernel listing against the parent: every kernel that existed kept its bytes, the four are new
    listing = (REPO / "profiles" / "r22_psd_codeobj_kernels.txt").read_text()
    assert "identical" in listing.splitlines()[0] and "DIFFER" not in listing.upper().replace("IDENTICAL", "")
    assert sorted(l.split("::")[-1] for l in listing.splitlines() if l.startswith("ONLY IN B")) == sorted(KERNELS)
    assert "ONLY IN A" not in listing
    for nfft in (64, 128, 1024, 4096):
        segs, lds, grid = _lib.spectrogram_plan(nfft, nfft // 2, 4)
        assert segs == 4096 // nfft and 0 < lds < 65536 and grid >= 1
    with pytest.raises(ValueError):
        _lib.spectrogram_plan(96, 48, 1)


def test_spectrogram_refusals_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_spectrogram
    keep, p = _aligned()
    nul = dict(src=None, win=None, out=None)

    def call(**kw):
        a = {**dict(src=p, kind=_lib.SRC_C64, S=1000, scale=1.0, win=p, nfft=64, hop=32, A=3, out=p, stride=64, R=10), **kw}
        return f(a["src"], a["kind"], a["S"], a["scale"], a["win"], a["nfft"], a["hop"], a["A"], a["out"], a["stride"], a["R"], None)
    assert _lib.load().amcx_spectrogram_out_rows(1000, 64, 32, 3) == 10
    # 1. the source kind and, for the integer kinds, the scale -- also where the call would otherwise be the no-op
    for kw in (dict(kind=5), dict(kind=-1), dict(kind=1), dict(kind=_lib.SRC_SC16, scale=0.0), dict(kind=_lib.SRC_CI8, scale=float("nan")),
               dict(kind=_lib.SRC_CU8, scale=float("inf")), dict(kind=_lib.SRC_SC16, scale=-1.0)):
        assert call(**kw) == _lib.EINVAL and call(**{"R": 0, **kw}, **nul) == _lib.EINVAL, kw
    assert call(R=0, scale=float("nan"), **nul) == _lib.OK                    # complex64 has no scale: it is not read
    # 2. the limits, the row count and the stride
    for kw in (dict(nfft=63), dict(nfft=96), dict(nfft=32), dict(nfft=8192), dict(nfft=0), dict(nfft=-64), dict(hop=0),
               dict(hop=65537), dict(A=0), dict(A=65537), dict(S=-1), dict(S=1 << 40), dict(S=(1 << 63) - 1)):
        assert call(**kw) == _lib.EINVAL and call(**{"R": 0, **kw}, **nul) == _lib.EINVAL, kw
    for kw in (dict(R=-1), dict(R=11), dict(S=63, R=1), dict(stride=63), dict(stride=0), dict(stride=-64), dict(stride=1 << 57)):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(R=0, stride=63, **nul) == _lib.EINVAL
    # 3. nothing to do: no pointer is looked at
    assert call(R=0, **nul) == _lib.OK and call(S=63, R=0, **nul) == _lib.OK and call(S=0, R=0, stride=1 << 60, **nul) == _lib.OK
    assert call(R=0, nfft=4096, hop=65536, A=65536, S=(1 << 40) - 1, stride=4096, **nul) == _lib.OK
    # 4. null pointers and alignment: a sample's for the source, 4 bytes for the window and the rows
    for kw in (dict(src=None), dict(win=None), dict(out=None), dict(src=p + 4), dict(kind=_lib.SRC_SC16, src=p + 2),
               dict(kind=_lib.SRC_CI8, src=p + 1), dict(win=p + 2), dict(out=p + 2)):
        assert call(**kw) == _lib.EINVAL, kw
    del keep


def test_detect_refusals_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_psd_detect_f32
    keep, p = _aligned()
    nul = dict(psd=None, floor=None, mask=None)

    def call(**kw):
        a = {**dict(psd=p, R=4, bins=16, stride=16, rank=3, thr=4.0, floor=p, mask=p), **kw}
        return f(a["psd"], a["R"], a["bins"], a["stride"], a["rank"], a["thr"], a["floor"], a["mask"], None)
    # 1. the limits, in front of the no-op
    for kw in (dict(R=-1), dict(bins=1), dict(bins=4097), dict(bins=0), dict(rank=-1), dict(rank=16), dict(thr=0.0), dict(thr=-1.0),
               dict(thr=float("inf")), dict(thr=float("nan"))):
        assert call(**kw) == _lib.EINVAL, kw
        if "R" not in kw:
            assert call(**{"R": 0, **kw}, **nul) == _lib.EINVAL, kw
    # 2. the stride
    for kw in (dict(stride=15), dict(stride=0), dict(R=1 << 40, stride=1 << 40)):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(R=0, stride=15, **nul) == _lib.EINVAL
    # 3. nothing to do
    assert call(R=0, **nul) == _lib.OK and call(R=0, bins=4096, rank=4095, stride=1 << 60, **nul) == _lib.OK
    # 4. null pointers and alignment (the mask is bytes, and may be left out: it is looked at by the launch alone)
    for kw in (dict(psd=None), dict(floor=None), dict(psd=p + 2), dict(floor=p + 1)):
        assert call(**kw) == _lib.EINVAL, kw
    del keep


def test_out_rows_against_a_brute_force_count_and_at_the_extremes():
    rows = _lib.load().amcx_spectrogram_out_rows
    for nfft in (64, 256):
        for hop in (1, nfft // 2, nfft, nfft + 3):
            for A in (1, 3):
                for S in list(range(nfft - 2, nfft + 3)) + [nfft + hop - 1, nfft + hop, nfft + A * hop - 1, nfft + A * hop,
                                                             7 * nfft + 5, 3 * A * hop + nfft + 1]:
                    want = ref.out_rows_brute(S, nfft, hop, A)
                    assert rows(S, nfft, hop, A) == want == ref.out_rows(S, nfft, hop, A) == psd.out_rows(S, nfft, hop, A), (S, nfft, hop, A)
    big = (1 << 40) - 1
    assert rows(big, 64, 1, 1) == big - 63 and rows(big, 4096, 65536, 65536) == ((big - 4096) // 65536 + 1) // 65536
    for S in (-1, 1 << 40, (1 << 63) - 1, -(1 << 63)):
        assert rows(S, 64, 32, 1) == -1
    for nfft, hop, A in ((63, 1, 1), (96, 1, 1), (32, 1, 1), (8192, 1, 1), (64, 0, 1), (64, 65537, 1), (64, 1, 0), (64, 1, 65537),
                         (-64, 1, 1), ((1 << 31) - 1, 1, 1)):
        assert rows(1000, nfft, hop, A) == -1, (nfft, hop, A)
    with pytest.raises(ValueError):
        psd.out_rows(1000, 100, 50, 1)
    with pytest.raises(ValueError):
        psd.out_rows(1 << 70, 64, 32, 1)


def test_the_table_and_the_fused_multiply_add_of_the_restatement():
    """The stored twiddles are within TW_UNITS 2^-24 of the exact ones (the bound's derivation relies on it), 1 and -j are
    exact, and fma32 rounds once (against exact rational arithmetic)."""
    from fractions import Fraction
    twr, twi = ref.twiddles32()
    k = np.arange(2048)
    err = np.abs((twr.astype(np.float64) + 1j * twi.astype(np.float64)) - np.exp(-2j * np.pi * k / 4096.0))
    assert err.max() <= ref.TW_UNITS * ref.U
    assert (twr[0], twi[0], twr[1024], twi[1024]) == (1.0, 0.0, 0.0, -1.0)
    rng = np.random.default_rng(2)
    a, b = (rng.standard_normal(400).astype(np.float32) for _ in range(2))
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1.0 + rng.standard_normal(400) * 1e-6)).astype(np.float32)   # cancellation
    got = ref.fma32(a, b, c)
    for i in range(400):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        d = abs(Fraction(float(got[i])) - exact)
        for other in (np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))):
            assert d <= abs(Fraction(float(other)) - exact), i


@pytest.mark.parametrize("nfft", [64, 128, 1024])
def test_restatement_meets_the_bound_and_the_exact_cases(nfft):
    """What the GPU must equal bit for bit is itself within the bound of the float64 definition, exact where the kernel's
    exact cases are, and loses the bound when one butterfly is lost."""
    w = psd.window(nfft, "hann")
    for hop, A in ((nfft // 2, 3), (nfft + 3, 1)):
        x = ref.spread_signal((3 * A - 1) * hop + nfft + 5, nfft, nfft + hop)
        P = ref.float32_rows(x, w, nfft, hop, A)
        assert P.shape == (3, nfft) and P.dtype == np.float32
        frac = ref.worst_fraction(P, x, w, nfft, hop, A)
        assert 0.0 < frac <= 1.0, frac
        lost = P.copy()
        lost[1, 5] = P[1, 6]                                                  # a permuted bin cannot hide
        assert ref.worst_fraction(lost, x, w, nfft, hop, A) > 1.0
    rect = psd.window(nfft, "rect")
    x = np.zeros(6 * nfft, np.complex64)
    x[::nfft] = 1.0
    assert np.array_equal(ref.float32_rows(x, rect, nfft, nfft, 3), np.full((2, nfft), 3.0, np.float32))
    x = np.array([1, 1j, -1, -1j], np.complex64)[np.arange(6 * nfft) % 4]
    want = np.zeros((2, nfft), np.float32)
    want[:, nfft // 4] = 3 * nfft ** 2
    assert np.array_equal(ref.float32_rows(x, rect, nfft, nfft, 3), want)


def test_window_scale_and_frequencies():
    w = psd.window(64)
    assert w.dtype == np.float32 and w[0] == 0.0 and w[32] == 1.0 and np.array_equal(w[1:], w[1:][::-1])      # periodic Hann
    assert np.array_equal(psd.window(8, "rect"), np.ones(8, np.float32))
    with pytest.raises(ValueError):
        psd.window(64, "hamming")
    assert psd.power_scale(psd.window(64, "rect"), 4) == 1.0 / (4 * 64)
    assert psd.power_scale(w, 1) == pytest.approx(1.0 / (64 * 0.375))
    assert psd.row_samples(64, 32, 3) == 128
    f = psd.bin_frequencies(8, 8.0, 100.0)
    assert f.tolist() == [100.0, 101.0, 102.0, 103.0, 96.0, 97.0, 98.0, 99.0]
    from amcpy_amd.bank import channel_frequencies
    assert np.array_equal(psd.bin_frequencies(64, 2.0e6, 1.0e8), channel_frequencies(64, 2.0e6, 1.0e8))


@pytest.mark.parametrize("fmt", ["cf32", "sc16", "cu8"])
def test_push_over_ragged_cuts_equals_one_call(fmt):
    rng = np.random.default_rng(4)
    S = 1200
    if fmt == "cf32":
        x = (rng.standard_normal(S) + 1j * rng.standard_normal(S)).astype(np.complex64)
    else:
        info = np.iinfo(ref.FORMATS[fmt])
        x = rng.integers(info.min, info.max + 1, (S, 2)).astype(ref.FORMATS[fmt])
    for nfft, hop, A in ((64, 32, 3), (64, 67, 2), (128, 128, 1)):
        base = ref.numpy_psd(x, nfft, hop=hop, averages=A)
        step, span = A * hop, psd.row_samples(nfft, hop, A)
        assert base.shape == (ref.out_rows(S, nfft, hop, A), nfft) and base.shape[0] >= 3
        cuts = {"ones": [1] * S, "primes": [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53] * 12,
                "inside a segment": [span + nfft // 3, S], "row less one": [span - 1] * (S // (span - 1) + 1)}
        for name, sizes in cuts.items():
            sp = psd.Spectrogram(nfft, hop, A, fmt=fmt, compute=ref.numpy_psd)
            rows, at = [], 0
            for n in sizes:
                if at >= S:
                    break
                rows.append(sp.push(x[at:at + n]))
                at = min(S, at + n)
                done = ref.out_rows(at, nfft, hop, A)
                assert sp.rows_done == done and sp.index == done * step and sp.held == max(0, at - done * step), (name, at)
            assert at == S and np.array_equal(np.concatenate(rows), base), (fmt, nfft, hop, A, name)
    with pytest.raises(TypeError):
        psd.Spectrogram(64, fmt="sc16", compute=ref.numpy_psd).push(np.zeros(10, np.complex64))
    with pytest.raises(ValueError):
        psd.Spectrogram(100, compute=ref.numpy_psd)


def _row(n, *on):
    m = np.zeros(n, bool)
    m[[b % n for b in on]] = True
    return m


def test_bands():
    assert psd.bands(_row(16, -1, 0, 1)) == [(-1, 1)]                                     # a run across DC joins
    assert psd.bands(_row(16, 6, 7, -8, -7)) == [(-8, -7), (6, 7)]                        # +1/2 does not wrap to -1/2
    assert psd.bands(_row(16, 1, 2, 5, 6)) == [(1, 6)] and psd.bands(_row(16, 1, 2, 5, 6), merge_bins=1) == [(1, 2), (5, 6)]
    assert psd.bands(_row(16, 1, 2, 6, 7)) == [(1, 2), (6, 7)]                            # three free bins: not joined
    assert psd.bands(_row(16, 3)) == [] and psd.bands(_row(16, 3), min_bins=1) == [(3, 3)]
    assert psd.bands(_row(16, 1, 4)) == [(1, 4)]                                          # joined first, then long enough
    assert psd.bands(_row(16, 1, 4), merge_bins=0) == []
    assert psd.bands(np.zeros(16, bool)) == [] and psd.bands(np.ones(16, bool)) == [(-8, 7)]
    with pytest.raises(ValueError):
        psd.bands(np.zeros((2, 16), bool))


def test_emitters():
    n = 32
    m = np.zeros((6, n), bool)
    m[0:3, 2:6] = True                           # rows 0 ... 2, bins 2 ... 5
    m[1, 6:9] = True                             # wider in row 1
    m[2:5, [-10, -9, -8]] = True                 # rows 2 ... 4 at negative bins
    m[5, 20 - n:24 - n] = True                   # one row alone (bins -12 ... -9: overlaps nothing in row 4? it does: -10, -9)
    got = psd.emitters(m)
    assert got == [(0, 2, 2, 8), (2, 5, -12, -8)]
    assert psd.emitters(m, min_rows=4) == [(2, 5, -12, -8)] and psd.emitters(m, min_rows=5) == []
    # a band that splits in the next row stays one emitter; two that join too
    s = np.zeros((3, n), bool)
    s[0, 0:11] = True
    s[1, 0:4] = True
    s[1, 7:11] = True
    s[2, 7:11] = True
    assert psd.emitters(s) == [(0, 2, 0, 10)] and psd.emitters(s[::-1]) == [(0, 2, 0, 10)]
    # not consecutive rows, or no common bin: apart
    a = np.zeros((3, n), bool)
    a[0, 0:3] = True
    a[2, 0:3] = True
    a[2, 6:9] = True
    assert psd.emitters(a) == [(0, 0, 0, 2), (2, 2, 0, 2), (2, 2, 6, 8)]
    assert psd.emitters(np.zeros((4, n), bool)) == [] and psd.emitters(np.ones((4, n), bool)) == [(0, 3, -16, 15)]
    assert psd.emitters(np.zeros((0, n), bool)) == []
    with pytest.raises(ValueError):
        psd.emitters(np.zeros(n, bool))


# ---- the scan of a recording, over injected computes -------------------------------------------------------------------------
SCAN = dict(S=1 << 18, nfft=256, A=16, seed=0)
INJECTED = dict(psd_compute=ref.numpy_psd, detect_compute=ref.numpy_psd_detect)


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    x = ref.synthetic_recording(SCAN["S"], SCAN["seed"])
    return {dt: ref.write_recording(tmp_path_factory.mktemp(dt), x, dt) for dt in ("cf32_le", "ci16_le")}


def _check_emitters(found, nfft, step, span, n_rows_per_capture):
    """The planted ones: two in the first capture, three in the second, every edge within 2 bins, spans the whole capture."""
    fs, half = ref.SAMPLE_RATE, SCAN["S"] // 2
    want = [(0, lo, hi) for lo, hi in ref.planted_bands(nfft, False)] + [(1, lo, hi) for lo, hi in ref.planted_bands(nfft, True)]
    assert len(found) == len(want) == 5
    for e, (cap, lo, hi) in zip(found, want):
        fc = ref.CAPTURE_FREQUENCIES[cap]
        assert e["sample_start"] == cap * half and e["sample_count"] == (n_rows_per_capture - 1) * step + span
        assert abs(e["freq_lower_edge"] - (fc + lo * fs / nfft)) <= 2.0 * fs / nfft
        assert abs(e["freq_upper_edge"] - (fc + hi * fs / nfft)) <= 2.0 * fs / nfft
        assert 6.0 < e["snr_db"] < 25.0


@pytest.mark.parametrize("datatype", ["cf32_le", "ci16_le"])
def test_scan_sigmf_with_injected_computes(recordings, datatype):
    from amcpy_amd import sigmf
    stem, held = recordings[datatype]
    nfft, A = SCAN["nfft"], SCAN["A"]
    hop, half = nfft // 2, SCAN["S"] // 2
    step, span = A * hop, psd.row_samples(nfft, hop, A)
    got = sigmf.scan_sigmf(stem, nfft=nfft, averages=A, detect={}, **INJECTED)
    assert set(got) == {"psd", "row_start", "row_samples", "freq_hz", "floor", "occupied", "snr_db", "emitters"}
    per = ref.out_rows(half, nfft, hop, A)
    R = 2 * per
    assert got["psd"].shape == (R, nfft) and got["psd"].dtype == np.float32 and got["row_samples"] == span
    # row_start, and no row straddles a capture
    assert got["row_start"].dtype == np.int64
    assert np.array_equal(got["row_start"], np.concatenate([step * np.arange(per), half + step * np.arange(per)]))
    assert np.all(got["row_start"][:per] + span <= half) and np.all(got["row_start"][per:] + span <= SCAN["S"])
    for cap in (0, 1):
        assert np.array_equal(got["psd"][cap * per:(cap + 1) * per],
                              ref.numpy_psd(held[cap * half:(cap + 1) * half], nfft, averages=A))
    assert np.array_equal(got["freq_hz"], psd.bin_frequencies(nfft, ref.SAMPLE_RATE, ref.CAPTURE_FREQUENCIES[0]))
    # the conditions, on the float64 reference alone: every row's band count is the planted count for its half, every edge
    # within 2 bins, and no cell of the reference sits within 1e-4 of the threshold (the GPU test relies on that)
    rank, thr = occupancy.floor_rank_of(nfft, 0.25), occupancy.threshold_of(6.0)
    w = psd.window(nfft)
    for cap in (0, 1):
        P64 = ref.reference(held[cap * half:(cap + 1) * half], w, nfft, hop, A)
        margin = P64 / (float(thr) * np.sort(P64, axis=1)[:, rank][:, None])
        assert not np.any(np.abs(margin - 1.0) < 1e-4)
        assert np.array_equal(got["occupied"][cap * per:(cap + 1) * per], margin > 1.0)
        planted = ref.planted_bands(nfft, bool(cap))
        for r in range(per):
            found = psd.bands(got["occupied"][cap * per + r])
            assert len(found) == len(planted), (cap, r, found)
            for (lo, hi), (tlo, thi) in zip(found, planted):
                assert abs(lo - 0.5 - tlo) <= 2.0 and abs(hi + 0.5 - thi) <= 2.0, (cap, r, lo, hi)
    _check_emitters(got["emitters"], nfft, step, span, per)
    assert [e["rows"] for e in got["emitters"]] == [(0, per - 1)] * 2 + [(per, R - 1)] * 3
    # however the capture is read; and without detect
    again = sigmf.scan_sigmf(stem, nfft=nfft, averages=A, detect={"threshold_db": 6.0}, chunk_samples=4099, **INJECTED)
    assert np.array_equal(again["psd"], got["psd"]) and again["emitters"] == got["emitters"]
    plain = sigmf.scan_sigmf(stem, nfft=nfft, averages=A, **INJECTED)
    assert set(plain) == {"psd", "row_start", "row_samples", "freq_hz"} and np.array_equal(plain["psd"], got["psd"])
    with pytest.raises(ValueError):
        sigmf.scan_sigmf(stem, psd_compute=ref.numpy_psd)                                  # the two go together
    with pytest.raises(ValueError):
        sigmf.scan_sigmf(stem, detect={"threshold": 6.0}, **INJECTED)


def test_scan_command_annotations_read_back_by_tune_from_annotation(recordings, tmp_path):
    from scipy.io import loadmat
    from amcpy_amd import main as cli, sigmf
    stem, _ = recordings["cf32_le"]
    nfft, A = SCAN["nfft"], SCAN["A"]
    parse = cli.build_parser().parse_args
    noted = tmp_path / "noted.sigmf-meta"
    args = parse(["scan", str(stem), "--nfft", str(nfft), "--averages", str(A), "--annotate", str(noted), "--out", str(tmp_path / "s.mat")])
    assert (args.hop, args.window, args.threshold_db, args.floor_quantile, args.min_bins, args.merge_bins, args.min_rows) == \
        (None, "hann", 6.0, 0.25, 2, 2, 1)
    mat = loadmat(cli.run_scan(args, **INJECTED))
    per = ref.out_rows(SCAN["S"] // 2, nfft, nfft // 2, A)
    assert mat["psd"].shape == (2 * per, nfft) and mat["occupied"].shape == (2 * per, nfft) and mat["floor"].size == 2 * per
    assert mat["emitter_sample_start"].size == 5 and mat["emitter_freq_lower_edge"].size == 5 and mat["freq_hz"].size == nfft
    # the written meta: the input's own annotation and captures survive; one annotation per emitter, which tune_from_annotation reads
    meta_in = json.loads(Path(str(stem) + ".sigmf-meta").read_text())
    meta = json.loads(noted.read_text())
    assert meta["global"] == meta_in["global"] and meta["captures"] == meta_in["captures"]
    anns = meta["annotations"]
    assert ref.OWN_ANNOTATION in anns and len(anns) == 6
    fs, half = ref.SAMPLE_RATE, SCAN["S"] // 2
    seen = []
    for k, ann in enumerate(anns):
        if ann == ref.OWN_ANNOTATION:
            continue
        assert set(ann) == {"core:sample_start", "core:sample_count", "core:freq_lower_edge", "core:freq_upper_edge", "core:comment"}
        assert "snr_db=" in ann["core:comment"]
        cap = int(ann["core:sample_start"] >= half)
        centre = (ann["core:freq_lower_edge"] + ann["core:freq_upper_edge"]) / 2.0 - ref.CAPTURE_FREQUENCIES[cap]
        j = int(np.argmin([abs(centre - fc * fs) for fc, _, _ in ref.PLANTED]))
        fc, width, _ = ref.PLANTED[j]
        seen.append((cap, j))
        shift_hz, (L, D) = sigmf.tune_from_annotation(meta, k, oversample=2.0, rational=True)
        assert abs(shift_hz - (-fc * fs)) <= fs / nfft                                     # within one bin width of -f_planted
        # every edge within 2 bins (and half a bin of rounding outwards each): the bandwidth within 5 bins, L / D within 2 x that
        assert abs(L / D - 2.0 * width) <= 2.0 * 5.0 / nfft + 0.002 * 2.0 * width, (k, L, D)
    assert sorted(seen) == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]
    # refusals, by name: no sample rate (in a process of its own: refused before anything of the device is loaded), and --format
    x = ref.synthetic_recording(1 << 12, 1)
    norate, _ = ref.write_recording(tmp_path, x, "cf32_le", name="norate", sample_rate=None)
    with pytest.raises(SystemExit, match="sample_rate"):
        cli.run_scan(parse(["scan", str(norate), "--annotate", str(tmp_path / "n.sigmf-meta")]), **INJECTED)
    r = subprocess.run([sys.executable, "-m", "amcpy_amd", "scan", str(norate), "--annotate", str(tmp_path / "n.sigmf-meta")],
                       cwd=str(REPO), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "sample_rate" in r.stderr and not (tmp_path / "n.sigmf-meta").exists()
    with pytest.raises(SystemExit, match="--format"):
        cli.run_scan(parse(["scan", str(stem), "--format", "cf32"]), **INJECTED)
    with pytest.raises(SystemExit, match="--format"):
        cli.run_scan(parse(["scan", str(norate) + ".sigmf-data.raw"]), **INJECTED)
    # without a sample rate the scan itself works: edges in cycles per sample, no freq_hz
    got = sigmf.scan_sigmf(norate, nfft=64, averages=8, detect={}, **INJECTED)
    assert "freq_hz" not in got and all(-0.51 <= e["freq_lower_edge"] < e["freq_upper_edge"] <= 0.51 for e in got["emitters"])
    # a raw stream through --format
    raw = tmp_path / "plain.cf32"
    raw.write_bytes(x.tobytes())
    mat = loadmat(cli.run_scan(parse(["scan", str(raw), "--format", "cf32", "--nfft", "64", "--averages", "8"]), **INJECTED))
    assert np.array_equal(mat["psd"], ref.numpy_psd(x, 64, averages=8)) and (tmp_path / "plain_scan.mat").exists()


def test_annotate_segments_shares_the_writer_and_keeps_its_output():
    from amcpy_amd import main as cli
    import inspect
    assert "with_annotations(" in inspect.getsource(cli.annotate_segments) and "with_annotations(" in inspect.getsource(cli.annotate_emitters)
    meta = {"global": {"core:sample_rate": 8.0}, "captures": [{}],
            "annotations": [{"core:sample_start": 40, "x": 1}, {"core:sample_start": 0, "x": 2}]}
    out = cli.annotate_segments(meta, [(1, 0, 1), (0, 2, 2)], np.array([0, 20, 40]), 10, 2, np.array([0.0, 4.0]))
    assert out["annotations"] == [
        {"core:sample_start": 0, "x": 2},
        {"core:sample_start": 0, "core:sample_count": 40, "core:freq_lower_edge": 2.0, "core:freq_upper_edge": 6.0},
        {"core:sample_start": 40, "x": 1},
        {"core:sample_start": 40, "core:sample_count": 20, "core:freq_lower_edge": -2.0, "core:freq_upper_edge": 2.0}]
    assert meta["annotations"] == [{"core:sample_start": 40, "x": 1}, {"core:sample_start": 0, "x": 2}]      # a copy
