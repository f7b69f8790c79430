"""The inputs of the index sweeps (tests/index_sweeps.py), checked without a GPU: a sweep is only as good as its frames.
The tone frames peak where they say, by a factor of 1000; the index sets hold what their docstrings promise and keep
the 8 M-sample cap; and the two comparisons the GPU tests apply can fail -- for the frame that should, and no other."""
import numpy as np
import pytest

from oracle import iq_features_oracle as orc
from tests import index_sweeps as sw


def _id(case):
    return "-".join(str(v) for v in case)


# ---------------------------------------------------------------------------------------------------------------------
# tone frames
# ---------------------------------------------------------------------------------------------------------------------
def _checked_bins(N, kind):
    """every bin of the case, or for N > 4096 a seeded 256 of them (first and last always)"""
    bins = sw.case_bins(N, kind)
    if N <= 4096 or len(bins) <= 256:
        return bins
    rng = np.random.default_rng([N, 11])
    pick = rng.choice(np.arange(1, len(bins) - 1), size=254, replace=False)
    return bins[np.sort(np.concatenate([[0], pick, [len(bins) - 1]]))]


@pytest.mark.parametrize("N,kind", sorted({(c[0], c[3]) for c in sw.BIN_CASES}, key=str))
def test_tone_frames_peak_in_their_bin(N, kind):
    """Conditions on the INPUT, in the feature's own unit |X|^2: the float64 spectrum of frame i has its maximum at k_i
    and nothing above 1e-3 of it anywhere else -- so a kernel that loses bin k_i is off 1000-fold, not by a tolerance."""
    bins = _checked_bins(N, kind)
    for part in sw.chunks(bins, N):
        x = sw.tone_frames(N, part, sw.BIN_SEED)
        assert x.dtype == np.complex64 and x.shape == (len(part), N)
        P = sw.power_spectrum(x)
        assert np.array_equal(P.argmax(axis=1), part)
        peak = P.max(axis=1)
        P[np.arange(len(part)), part] = 0.0
        assert (P.max(axis=1) <= 1e-3 * peak).all(), (N, part[(P.max(axis=1) > 1e-3 * peak)][:8])
        # the peak is the tone's: N A^2 with A in [0.5, 2], up to the noise under it
        assert ((peak >= 0.24 * N) & (peak <= 4.1 * N)).all()
        assert np.array_equal(sw.peak_reference(x), peak.astype(np.float32))


def test_tone_frames_do_not_depend_on_the_other_bins_asked_for():
    a = sw.tone_frames(1000, [3, 999, 500], 20)
    b = sw.tone_frames(1000, [500, 3], 20)
    assert np.array_equal(a[2], b[0]) and np.array_equal(a[0], b[1])
    assert not np.array_equal(a[0], sw.tone_frames(1000, [3], 21)[0])
    amp = np.abs(a.astype(np.complex128)).mean(axis=1)
    assert ((amp > 0.49) & (amp < 2.01)).all() and len(set(amp.round(3))) == 3


@pytest.mark.parametrize("N", sw.POW2_SIZES)
def test_half_bin_tones_straddle_two_bins(N):
    """A tone at k + 1/2: the two bins next to it carry (2 / pi)^2 of N A^2 each, and the spectrum falls off from there."""
    ks = sw.half_bins(N, sw.BIN_SEED)
    assert len(ks) == 64 and len(set(ks.tolist())) == 64 and ks.min() >= 0 and ks.max() < N
    x = sw.tone_frames(N, ks, sw.BIN_SEED, half_bin=True)
    P = sw.power_spectrum(x)
    top = P.argmax(axis=1)
    assert (((top - ks) % N == 0) | ((top - ks) % N == 1)).all()
    two = np.sort(np.stack([P[np.arange(64), ks], P[np.arange(64), (ks + 1) % N]]), axis=0)
    assert (two[0] >= 0.97 * two[1]).all()                              # equal up to the noise under the tone
    P[np.arange(64), ks] = 0
    P[np.arange(64), (ks + 1) % N] = 0
    assert (P.max(axis=1) <= 0.12 * two[1]).all()                       # the next pair: (2 / (3 pi))^2 / (2 / pi)^2 = 1 / 9


# ---------------------------------------------------------------------------------------------------------------------
# index sets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sw.BIN_CASES, ids=_id)
def test_bin_sets(case):
    N, how, kernel, kind = case
    bins = sw.case_bins(N, kind)
    assert bins.min() >= 0 and bins.max() < N and len(np.unique(bins)) == len(bins)
    if kind == "all":
        assert np.array_equal(bins, np.arange(N))
    elif kind == "group":
        W = N // 2048
        assert len(bins) == 2050                                                     # N/2 = k_1024 and N - 1 = k_2047 come once
        assert np.array_equal(np.sort(bins[:2048] // W), np.arange(2048))            # every output index j of a wave's FFT
        assert (np.bincount(bins[:2048] % W, minlength=W) == 2048 // W).all()        # every wave residue, evenly
        assert np.array_equal((bins[:2048] // W) % W, bins[:2048] % W)               # k_j = W j + (j mod W)
        assert {1, N // 2, N // 2 + 1, N - 1} <= set(bins.tolist())
    else:
        assert len(bins) == kind
        edge = min(64, kind // 8)
        assert set(range(edge)) <= set(bins.tolist()) and set(range(N - edge, N)) <= set(bins.tolist())
        assert np.array_equal(bins, sw.case_bins(N, kind))                             # seeded: the same set every time
    for part in sw.chunks(bins, N):
        assert len(part) * N <= sw.MAX_SAMPLES
    assert np.array_equal(np.concatenate(sw.chunks(bins, N)), bins)


def test_bin_cases_are_the_table():
    """sizes, paths and bin counts of the table the sweep was specified with"""
    got = {(N, how): len(sw.case_bins(N, kind)) for N, how, _, kind in sw.BIN_CASES}
    want = {(N, "wave"): N for N in (128, 256, 512, 1024, 2048, 4096, 8192)}
    want.update({(2048, "block"): 2048, (16384, "wave"): 2050, (32768, "wave"): 2050})
    want.update({(N, "auto"): N for N in (3, 10, 63, 64, 65, 1000, 4095, 4097)})
    want.update({(8191, "auto"): 2048, (8193, "auto"): 1024, (16385, "auto"): 1024, (32767, "auto"): 1024, (8193, "ws0"): 64})
    assert got == want and len(sw.BIN_CASES) == len(want)


def _has_triples(pos, stride, lo, hi):
    have = set(pos.tolist())
    want = {p for m in range(0, hi + stride, stride) for p in (m - 1, m, m + 1) if lo <= p < hi}
    return want <= have, sorted(want - have)[:8]


@pytest.mark.parametrize("N", sorted({c[0] for c in sw.POSITION_CASES}))
def test_seam_positions(N):
    pos = sw.seam_positions(N)
    assert pos.min() >= 0 and pos.max() < N and len(np.unique(pos)) == len(pos) and np.array_equal(pos, np.sort(pos))
    assert np.array_equal(pos, sw.seam_positions(N))
    have = set(pos.tolist())
    if N <= 512:
        assert np.array_equal(pos, np.arange(N))
        return
    assert set(range(66)) <= have and set(range(N - 66, N)) <= have
    if N < 8192:
        strides = [(64, 0, N)]
    else:
        strides = [(2048, 0, N), (64, 0, 2048), (64, N - 2048, N)]
    if N in (8193, 16385):
        strides += [(8192, 0, N), (1024, 0, N), (16384, 0, N)]
    for stride, lo, hi in strides:
        ok, missing = _has_triples(pos, stride, lo, hi)
        assert ok, (N, stride, missing)
    seeded = len(pos) - len(sw.seams(N))
    assert 0 <= seeded <= 64
    if seeded < 64:                                        # thinned only where the cap leaves no room
        assert len(pos) == sw.position_parts(N) * (sw.MAX_SAMPLES // N)
    # a pair that straddles each seam is there as p - 1, p, p + 1: both steps of the seam's sample are aimed at
    if N == 16385:
        assert {16383, 16384} <= have                      # (16385 would be past the end)
    if N == 8193:
        assert {8191, 8192} <= have


def test_position_cases_keep_the_cap_and_cover_every_position():
    sizes = {}
    for N, variant, part in sw.POSITION_CASES:
        p = sw.case_positions(N, part)
        assert 0 < len(p) * N <= sw.MAX_SAMPLES, (N, part, len(p))
        sizes.setdefault((N, variant), []).append(p)
    for (N, variant), parts in sizes.items():
        assert len(parts) == sw.position_parts(N)
        assert np.array_equal(np.concatenate(parts), sw.seam_positions(N))
    assert {k for k in sizes} == {(N, "wave") for N in sw.POW2_SIZES} | {(N, "auto") for N in (100, 1000, 4097, 8193, 16385)}
    assert [N for N in sw.POW2_SIZES if sw.position_parts(N) > 1] == [32768]


def test_outlier_frames():
    base = sw.base_frame(1024)
    assert base.dtype == np.complex64 and base.shape == (1024,)
    pos = sw.seam_positions(1024)
    x = sw.outlier_frames(base, pos)
    assert x.dtype == np.complex64 and x.shape == (len(pos), 1024)
    diff = x != base[None, :]
    assert (diff.sum(axis=1) == 1).all() and np.array_equal(diff.argmax(axis=1), pos)
    r = x[np.arange(len(pos)), pos].astype(np.complex128) / base[pos].astype(np.complex128)
    assert np.allclose(r, 3.0 * np.exp(2.0j), rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: the comparisons can fail
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [63, 256])
def test_bin_comparison_fails_for_the_scaled_bin_alone(N):
    """A transform whose output bin j is 1 + 1e-4 too large in power, every other bin right: the sweep's comparison
    fails for frame j and passes every other frame."""
    bins = sw.all_bins(N)
    x = sw.tone_frames(N, bins, sw.BIN_SEED)
    P = sw.power_spectrum(x)
    ref = sw.peak_reference(x)
    assert sw.bins_beyond(P.max(axis=1).astype(np.float32), ref, bins) == []
    for j in range(N):
        Q = P.copy()
        Q[:, j] *= 1.0 + 1e-4
        miss = sw.bins_beyond(Q.max(axis=1).astype(np.float32), ref, bins)
        assert [b for b, _ in miss] == [j], (j, miss)
        with pytest.raises(AssertionError, match=rf"bins \[{j}\]"):
            sw.assert_bins(Q.max(axis=1).astype(np.float32), ref, bins, "sensitivity")
    # a lost peak: 1000-fold and more
    Q = P.copy()
    Q[5, 5] = 0.0
    miss = sw.bins_beyond(Q.max(axis=1).astype(np.float32), ref, bins)
    assert [b for b, _ in miss] == [5] and miss[0][1] > 0.999
    nan = ref.copy()
    nan[7] = np.nan
    assert [b for b, _ in sw.bins_beyond(nan, ref, bins)] == [7]


@pytest.mark.parametrize("N", [128, 4096, 32768])
def test_position_comparison_fails_when_the_sample_is_dropped(N):
    """Features computed with sample p left out of frame p (what a kernel that drops it would see): the position
    comparison fails for that frame -- for each frame alone, and naming the positions for the batch."""
    pos = sw.seam_positions(N)
    if N > 512:                                            # a spread of 24 of them, both ends included
        pos = pos[np.unique(np.linspace(0, len(pos) - 1, 24).astype(int))]
    base = sw.base_frame(N)
    x = sw.outlier_frames(base, pos)
    gold = orc.features18_batch(x)
    sw.assert_position_parity(gold.astype(np.float32), gold, x, pos, "the oracle against itself")
    keep = np.ones(x.shape, bool)
    keep[np.arange(len(pos)), pos] = False
    dropped = orc.features18_batch(x[keep].reshape(len(pos), N - 1)).astype(np.float32)
    for i, p in enumerate(pos):
        with pytest.raises(AssertionError):
            sw.assert_position_parity(dropped[i:i + 1], gold[i:i + 1], x[i:i + 1], pos[i:i + 1], f"dropped {p}")
    mixed = gold.astype(np.float32)
    mixed[3] = dropped[3]
    with pytest.raises(AssertionError, match=rf"positions \[{int(pos[3])}\]"):
        sw.assert_position_parity(mixed, gold, x, pos, "one frame dropped its sample")
