"""Index coverage of the kernels (needs an MI355X: -m gpu): feature 1 with the spectral peak in a PRESCRIBED output bin of
every FFT path, and all 18 features with one outlying sample at a PRESCRIBED position around every seam of every
kernel's data layout.  The frames, the index sets and the two comparisons are tests/index_sweeps.py (checked on the CPU
by tests/test_index_sweeps_host.py); the bounds are the project's contract and nothing else: plain relative 1e-5 on
feature 1, tests/test_gpu_parity.py::_assert_parity on the 18.  A failure names bins or sample positions: indices that
share a residue, a lane, a register row or a chirp range point at the stage that is wrong."""
import numpy as np
import pytest

from amcpy_amd import _lib
from oracle import iq_features_oracle as orc
from tests import index_sweeps as sw
from tests.test_gpu_parity import _run, _run_ws

pytestmark = pytest.mark.gpu

# a case of more than five chunks of 8 M samples is cut into equal parametrised parts, so that host generation and np.fft
# stay at a few seconds a case: 8192 (every bin: 64 M samples) and 32768 (2050 bins: 64 M samples) go in two parts each
_PARTS = {c: -(-len(sw.chunks(sw.case_bins(c[0], c[3]), c[0])) // 5) for c in sw.BIN_CASES}
_BIN_PARAMS = [pytest.param(c, part, id=f"{c[0]}-{c[1]}-{c[3]}-part{part}") for c in sw.BIN_CASES for part in range(_PARTS[c])]


def _feature1(x, how, N):
    if how == "ws0":
        return _run_ws(x, N, 0)[:, 0]
    return _run(x, how)[:, 0]


def _assert_kernel(N, how, kernel):
    assert _lib.kernel_name(N, _lib.VARIANTS["auto" if how == "ws0" else how]) == kernel, (N, how)


@pytest.mark.parametrize("case,part", _BIN_PARAMS)
def test_bin_sweep(case, part):
    """One frame per bin (tests/index_sweeps.py: tone_frames), feature 1 against golden64's definition, plain relative
    <= 1e-5 on every frame; a failure lists the bins.

    every bin: the short kernels (128, 256, 512), the wave kernels (1024, 2048, 4096), the quad kernel (8192), the LDS
    radix-2 FFT (2048 "block"), block_kernel<0> (3, 10, 63), <1> (64), <2> (65, 1000, 4095), <3> (4097);
    k_j = W j + (j mod W) and 1, N/2, N/2 + 1, N - 1: the group kernels (16384, 32768) -- every output index of a wave's
    2048-point FFT and every wave residue; the lowest 64, the highest 64 and seeded bins between: 2048 at 8191 (<3>), 1024
    at 8193, 16385 and 32767 (the stream kernel's chirp-z through a workspace), 64 (8 + 8 + 48) at 8193 with no workspace
    (the DFT by its definition)."""
    N, how, kernel, kind = case
    _assert_kernel(N, how, kernel)
    bins = np.array_split(sw.case_bins(N, kind), _PARTS[case])[part]
    runs = sw.chunks(bins, N)
    got, ref = [], []
    for run in runs:
        x = sw.tone_frames(N, run, sw.BIN_SEED)
        assert x.size <= sw.MAX_SAMPLES
        ref.append(sw.peak_reference(x))
        got.append(_feature1(x, how, N))
    got, ref = np.concatenate(got), np.concatenate(ref)
    rel = np.abs(got.astype(np.float64) - ref) / ref
    print(f"\n[bin sweep N={N} {how} {kernel}] {len(bins)} bins, worst plain rel {np.nanmax(rel):.2e} at bin {int(bins[np.nanargmax(rel)])}")
    sw.assert_bins(got, ref, bins, f"bin sweep N={N} {how} ({kernel})")


@pytest.mark.parametrize("N,how,kernel", [(c[0], c[1], c[2]) for c in sw.BIN_CASES if c[0] in sw.POW2_SIZES])
def test_off_bin_tones(N, how, kernel):
    """64 tones at k + 1/2 for seeded k at every power of two: the energy spreads over all bins with known weights
    ((2 / pi)^2 of it in each neighbour), so leakage in the wrong direction anywhere moves the maximum."""
    _assert_kernel(N, how, kernel)
    ks = sw.half_bins(N, sw.BIN_SEED)
    x = sw.tone_frames(N, ks, sw.BIN_SEED, half_bin=True)
    ref = sw.peak_reference(x)
    got = _feature1(x, how, N)
    rel = np.abs(got.astype(np.float64) - ref) / ref
    print(f"\n[off-bin tones N={N} {how}] worst plain rel {np.nanmax(rel):.2e} at k = {int(ks[np.nanargmax(rel)])} + 1/2")
    sw.assert_bins(got, ref, ks, f"off-bin tones (k + 1/2) N={N} {how} ({kernel})")


def _named(check, positions, a, b, cols):
    """run `check`; when it fails, add the sample positions of the rows that differ in `cols`"""
    try:
        check()
    except AssertionError as err:
        same = (a[:, cols] == b[:, cols]) | (np.isnan(a[:, cols]) & np.isnan(b[:, cols]))
        rows = np.flatnonzero(~same.all(axis=1))
        raise AssertionError(f"{err}\nsample positions of the rows that differ: {np.asarray(positions)[rows][:64].tolist()}") from None


@pytest.mark.parametrize("N,variant,part", sw.POSITION_CASES)
def test_position_sweep(N, variant, part):
    """Frame p = the size's base frame (16QAM, 12 dB, seed N) with sample p replaced by 3 base[p] exp(2i), for every p
    of tests/index_sweeps.py: seam_positions(N) (N <= 512: every p), against the oracle with _assert_parity unchanged.
    128 ... 32768 with "wave" (32768 in two parts: its seams alone exceed the 8 M samples a case sends through the
    oracle), 100, 1000, 4097, 8193 and 16385 with "auto".  At 128 ... 4096 the same batch also goes through the two plan
    kernels (no spectral term; f10 ... f18 alone) and, quantised, through the kernels that read int16: the asked-for
    columns bit-identical to the full run / to the widened complex64 twin, as tests/test_gpu_feature_subsets.py and
    tests/test_gpu_sc16.py define those identities."""
    pos = sw.case_positions(N, part)
    x = sw.outlier_frames(sw.base_frame(N), pos)
    assert x.size <= sw.MAX_SAMPLES
    want = _lib.kernel_name(N, _lib.VARIANTS[variant])
    if variant == "wave":
        assert any(stem in want for stem in ("short_kernel", "wave_kernel", "quad_kernel", "group_kernel")), want
    else:
        assert want == {100: "amcx_features18_block_kernel<2>", 1000: "amcx_features18_block_kernel<2>",
                        4097: "amcx_features18_block_kernel<3>"}.get(N, "amcx_features18_stream_kernel")
    gold = orc.features18_batch(x)
    got = _run(x, variant)
    sw.assert_position_parity(got, gold, x, pos, f"position sweep N={N} {variant} part {part} ({want})")
    if N not in sw.PLAN_SIZES or variant != "wave":
        return
    import torch
    from tests import test_gpu_feature_subsets as subsets
    from tests import test_gpu_sc16 as typed
    for name in ("no_spectral", "cumulants"):
        mask = subsets.MASKS[name]
        assert "subset" in _lib.kernel_name_subset(N, _lib.VARIANT_WAVE, mask)
        sub = subsets._run(x, N, "wave", mask)
        cols = [j for j in range(18) if (mask >> j) & 1]
        _named(lambda: subsets._check(sub, got, mask, (N, name)), pos, sub, got, cols)
    x16 = typed._quantise(x)
    scale = 2.0 ** -11
    wide = typed._widen(x16, scale)
    assert np.abs(x16.astype(np.int32)).max() < 32767                                  # nothing clipped: the outlier is still one
    xd, wd = torch.from_numpy(x16).cuda(), torch.from_numpy(wide).cuda()
    for mask in (_lib.FEATURES_ALL, _lib.FEATURES_NO_SPECTRAL, _lib.FEATURES_CUMULANTS):
        assert "sc16" in _lib.kernel_name_sc16(N, _lib.VARIANT_WAVE, mask)
        a = typed._sc16(xd, N, "wave", mask, scale)
        b = typed._ref(wd, N, "wave", mask)

        def same():
            assert typed._same(a, b), ((N, hex(mask)), typed._where(a, b))
        _named(same, pos, a, b, list(range(18)))
