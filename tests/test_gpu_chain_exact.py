"""The down-converter, the filter bank and the resampler at their LARGEST tap counts, on data where float32 arithmetic in any
order is exact (tests/chain_exact.py): every output of every case is compared with == against int64 arithmetic.

At these shapes the derived rounding bounds of the three parity suites are as large as one whole term of an output (2^24 /
(2 T (T + 8)) is 2 at T = 2048 and 0.5 at P = 4096), and these shapes are where the kernels differ from the small ones: several
rounds per thread, the remainders of the unrolled loops, the LDS images at their limits, the phase-major tap table at its
largest pitch.  One term lost or doubled anywhere fails here.  Every case runs M = 2 tile + 3 outputs -- two tile seams and a
ragged last tile -- in all four formats at all four quarter-turn settings of the pre-mixer.

For C >= 8 the bank's twiddles are irrational; the branch sums are still exact on this data, so the outputs are held to the
TRANSFORM's share of tests/bank_ref.py's bound alone, 7 log2 C 2^-24 S, against the exact branch sums transformed in float64."""
import functools

import numpy as np
import pytest

from amcpy_amd import _formats, _lib, bank, ddc, resample as rs
from tests import bank_ref, chain_exact as ce, stream_inputs

pytestmark = pytest.mark.gpu


_torch = stream_inputs.torch


@functools.lru_cache(maxsize=4)
def _ints(S, seed):
    k = ce.make_ints(S, seed)
    k.setflags(write=False)
    return k


def _streams(S, seed):
    """{format: the same values k g in GPU memory}"""
    torch = _torch()
    return {fmt: torch.from_numpy(ce.encode(_ints(S, seed), fmt)).cuda() for fmt in ce.FORMATS}


def _taps_dev(h):
    return _torch().from_numpy(np.asarray(h, dtype=np.float32)).cuda()


def _assert_exact(y, exact, g, what):
    y = y.cpu().numpy()
    bad = ce.mismatches(y, exact, g)
    if bad:
        re, im = ce.as_float32(exact, g)
        at = np.argwhere((y.real != re) | (y.imag != im))[:8]
        first = tuple(at[0])
        raise AssertionError(f"{what}: {bad} of {y.size} outputs differ from the exact result, first at {at.tolist()}: "
                             f"got {y[first]!r}, want {re[first]!r} + {im[first]!r}j (in units of g = {g}: "
                             f"{y[first] / g!r} against {exact[0][first]} + {exact[1][first]}j)")


def test_the_default_scales_are_powers_of_two():
    for fmt in ce.FORMATS:
        assert np.frexp(_formats.get(fmt).scale)[0] == 0.5
        assert ce.UNIT[fmt] == _formats.get(fmt).scale * (256 if fmt == "sc16" else 1)


@pytest.mark.parametrize("T,D", ce.DDC_CASES)
def test_down_converter(T, D):
    """... and amcx_resample with interp = 1 gives the same bytes (T <= 2048)."""
    torch = _torch()
    tile, _ = _lib.tune_decimate_plan(T, D)
    M = 2 * tile + 3
    S = ce.ddc_span(M, T, D)
    assert ddc.out_samples(S, T, D) == M and rs.out_samples(S, T, 1, D) == M
    h = ce.make_taps(T)
    taps, x = _taps_dev(h), _streams(S, T + D)
    for shift, index0 in ce.QUARTER_TURNS:
        exact = ce.ddc_exact(ce.mix(_ints(S, T + D), shift, index0), h, D, M)
        for fmt in ce.FORMATS:
            y = ddc.tune_decimate(x[fmt], taps, D, shift=shift, sample_index0=index0)
            r = rs.resample(x[fmt], taps, 1, D, shift=shift, sample_index0=index0)
            torch.cuda.synchronize()
            assert y.shape == (M,) and y.dtype == torch.complex64
            _assert_exact(y, exact, ce.UNIT[fmt], f"ddc {fmt} T={T} D={D} shift={shift} index0={index0} tile={tile}")
            assert r.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (fmt, T, D, shift)
    print(f"ddc exact T={T} D={D} tile={tile} M={M} S={S}: 4 formats x 4 quarter turns equal int64 arithmetic, interp 1 the same bytes")


@pytest.mark.parametrize("T,L,D", ce.RESAMPLE_CASES)
def test_resampler(T, L, D):
    torch = _torch()
    tile = _lib.resample_plan(T, L, D)[0]
    h = ce.make_taps(T)
    taps = _taps_dev(h)
    for tau0 in sorted({0, L - 1}):
        S, M = ce.resample_span(2 * tile + 3, T, L, D, tau0)
        assert rs.out_samples(S, T, L, D, tau0) == M >= 2 * tile + 3
        x = _streams(S, T + L + tau0)
        for shift, index0 in ce.QUARTER_TURNS:
            exact = ce.resample_exact(ce.mix(_ints(S, T + L + tau0), shift, index0), h, L, D, tau0, M)
            for fmt in ce.FORMATS:
                y = rs.resample(x[fmt], taps, L, D, shift=shift, sample_index0=index0, phase_index0=tau0)
                torch.cuda.synchronize()
                assert y.shape == (M,) and y.dtype == torch.complex64
                _assert_exact(y, exact, ce.UNIT[fmt], f"resample {fmt} T={T} L={L} D={D} tau0={tau0} shift={shift} index0={index0} "
                                                      f"tile={tile}")
        print(f"resample exact T={T} L={L} D={D} tau0={tau0} P={ce.phase_taps(T, L)} tile={tile} M={M} S={S}: "
              f"4 formats x 4 quarter turns equal int64 arithmetic")


@pytest.mark.parametrize("Cn,T,D", ce.BANK_EXACT_CASES)
def test_filter_bank_exact(Cn, T, D):
    """C = 2 and 4: the channel factors are +-1 and +-j, every output is a Gaussian integer times g."""
    torch = _torch()
    tile, _, lds = _lib.filter_bank_plan(T, Cn, D)
    if (Cn, T, D) == ce.BANK_LDS_MAX_CASE:
        assert lds == ce.BANK_LDS_MAX, lds                                 # the largest LDS request of any bank launch
    M = 2 * tile + 3
    S = ce.ddc_span(M, T, D)
    assert bank.out_samples(S, T, Cn, D) == M
    h = ce.make_taps(T)
    taps, x = _taps_dev(h), _streams(S, T + Cn + D)
    for shift, index0 in ce.BANK_QUARTER_TURNS:
        assert index0 % 2 == 1
        u = ce.bank_branch_sums(ce.mix(_ints(S, T + Cn + D), shift, index0), h, Cn, D, M, index0)
        exact = ce.bank_exact(u, Cn)
        for fmt in ce.FORMATS:
            y = bank.filter_bank(x[fmt], taps, Cn, D, shift=shift, sample_index0=index0)
            torch.cuda.synchronize()
            assert y.shape == (Cn, M) and y.dtype == torch.complex64
            _assert_exact(y, exact, ce.UNIT[fmt], f"bank {fmt} C={Cn} T={T} D={D} shift={shift} index0={index0} tile={tile}")
    print(f"bank exact C={Cn} T={T} D={D} tile={tile} lds={lds} M={M} S={S}: 4 formats x 4 quarter turns equal int64 arithmetic")


@pytest.mark.parametrize("Cn,T,D", ce.BANK_TRANSFORM_CASES)
def test_filter_bank_transform_alone(Cn, T, D):
    """C >= 8: the branch sums are exact, so |y - transform of the exact sums| <= 7 log2 C 2^-24 S for EVERY output."""
    torch = _torch()
    tile, _, lds = _lib.filter_bank_plan(T, Cn, D)
    M = 2 * tile + 3
    S = ce.ddc_span(M, T, D)
    assert bank.out_samples(S, T, Cn, D) == M
    h = ce.make_taps(T)
    taps, x = _taps_dev(h), _streams(S, T + Cn + D)
    factor = 7 * bank_ref.log2_exact(Cn)
    sabs = ce.abs_sums(_ints(S, T + Cn + D), h, D, M)
    assert sabs.shape == (M,) and sabs.min() > 0
    worst = 0.0
    for shift, index0 in ce.BANK_QUARTER_TURNS:
        u = ce.bank_branch_sums(ce.mix(_ints(S, T + Cn + D), shift, index0), h, Cn, D, M, index0)
        want = ce.bank_float64(u, Cn)
        for fmt in ce.FORMATS:
            g = ce.UNIT[fmt]
            y = bank.filter_bank(x[fmt], taps, Cn, D, shift=shift, sample_index0=index0)
            torch.cuda.synchronize()
            assert y.shape == (Cn, M) and y.dtype == torch.complex64
            ratio = np.abs(y.cpu().numpy().astype(np.complex128) / g - want) / (factor * ce.U * sabs)[None, :]
            at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            worst = max(worst, float(ratio[at]))
            assert ratio[at] <= 1.0, (fmt, Cn, T, D, shift, index0, at, float(ratio[at]))
            # channel 0's twiddles are all 1: its outputs are sums and differences of exact integers
            total = (u[0].sum(axis=1), u[1].sum(axis=1))
            _assert_exact(y[0], total, g, f"bank channel 0 {fmt} C={Cn} T={T} D={D} shift={shift}")
    print(f"bank transform alone C={Cn} T={T} D={D} tile={tile} lds={lds} M={M} S={S}: worst |err| / (7 log2 C 2^-24 S) = "
          f"{worst:.4f} (factor {factor}); channel 0 exact")


# ---- the bank's tile loop beyond one pass of its grid --------------------------------------------------------------------------
def _bank_three_trips(Cn, T, D):
    """(tile, grid, M, S): M = tile (2 grid + 1) + 3 outputs, so that some workgroup takes three tiles and the last is ragged"""
    tile, grid, _ = _lib.filter_bank_plan(T, Cn, D)
    assert tile == 4096 // Cn
    M = tile * (2 * grid + 1) + 3
    tiles = -(-M // tile)
    print(f"bank C={Cn} T={T} D={D}: {M} outputs = {tiles} tiles of {tile} over {grid} workgroups")
    assert tiles >= 2 * grid + 1
    S = ce.ddc_span(M, T, D)
    assert bank.out_samples(S, T, Cn, D) == M
    return tile, grid, M, S


def _branch_sums_blocked(v, h, Cn, D, M, index0, block=4096):
    """ce.bank_branch_sums over M outputs in blocks of outputs (its gather is sized for a few thousand): output m0 + i of the
    stream is output i of the stream from sample m0 D on, whose first sample has the index index0 + m0 D"""
    parts = [ce.bank_branch_sums((v[0][m0 * D:], v[1][m0 * D:]), h, Cn, D, min(block, M - m0), index0 + m0 * D)
             for m0 in range(0, M, block)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _same_bytes(a, b):
    torch = _torch()
    return a.shape == b.shape and bool(torch.equal(torch.view_as_real(a).view(torch.int32), torch.view_as_real(b).view(torch.int32)))


def _sc16_and_its_widened_samples(S, seed):
    """the sc16 stream of _ints and the complex64 stream of the same values k 2^-7, both in GPU memory"""
    torch = _torch()
    k = _ints(S, seed)
    wide = ((k[:, 0] + 1j * k[:, 1]) * ce.UNIT["sc16"]).astype(np.complex64)
    return torch.from_numpy(ce.encode(k, "sc16")).cuda(), torch.from_numpy(wide).cuda()


def test_filter_bank_transform_alone_over_three_trips_of_the_grid():
    """C = 256: tiles of 16 outputs, 2 grid + 1 of them and 3 outputs more.  The derived factor of
    test_filter_bank_transform_alone on EVERY output, channel 0 exact; sc16 the bytes of complex64 on the widened samples."""
    torch = _torch()
    Cn, T, D = 256, 512, 1
    tile, grid, M, S = _bank_three_trips(Cn, T, D)
    h = ce.make_taps(T)
    taps = _taps_dev(h)
    shift, index0 = ce.BANK_QUARTER_TURNS[1]
    assert index0 % 2 == 1 and shift != 0
    k = _ints(S, T + Cn)
    factor = 7 * bank_ref.log2_exact(Cn)
    sabs = ce.abs_sums(k, h, D, M)
    assert sabs.shape == (M,) and sabs.min() > 0
    u = _branch_sums_blocked(ce.mix(k, shift, index0), h, Cn, D, M, index0)
    want = ce.bank_float64(u, Cn)
    y = bank.filter_bank(torch.from_numpy(ce.encode(k, "cf32")).cuda(), taps, Cn, D, shift=shift, sample_index0=index0)
    torch.cuda.synchronize()
    assert y.shape == (Cn, M) and y.dtype == torch.complex64
    ratio = np.abs(y.cpu().numpy().astype(np.complex128) - want) / (factor * ce.U * sabs)[None, :]
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"bank transform alone C={Cn} T={T} D={D} over three trips: worst |err| / (7 log2 C 2^-24 S) = {float(ratio[at]):.4f} "
          f"at {tuple(int(i) for i in at)}")
    assert ratio[at] <= 1.0, (at, float(ratio[at]))
    _assert_exact(y[0], (u[0].sum(axis=1), u[1].sum(axis=1)), 1.0, f"bank channel 0 cf32 C={Cn} T={T} D={D} over three trips")
    raw, wide = _sc16_and_its_widened_samples(S, T + Cn)
    assert _same_bytes(bank.filter_bank(raw, taps, Cn, D, shift=shift, sample_index0=index0),
                       bank.filter_bank(wide, taps, Cn, D, shift=shift, sample_index0=index0))


def test_filter_bank_exact_over_three_trips_of_the_grid():
    """C = 4: tiles of 1024 outputs, 2 grid + 1 of them and 3 outputs more, every output == int64 arithmetic; sc16 the bytes
    of complex64 on the widened samples."""
    torch = _torch()
    Cn, T, D = 4, 8, 1
    tile, grid, M, S = _bank_three_trips(Cn, T, D)
    h = ce.make_taps(T)
    taps = _taps_dev(h)
    shift, index0 = ce.BANK_QUARTER_TURNS[1]
    k = _ints(S, T + Cn)
    exact = ce.bank_exact(ce.bank_branch_sums(ce.mix(k, shift, index0), h, Cn, D, M, index0), Cn)
    y = bank.filter_bank(torch.from_numpy(ce.encode(k, "cf32")).cuda(), taps, Cn, D, shift=shift, sample_index0=index0)
    torch.cuda.synchronize()
    assert y.shape == (Cn, M) and y.dtype == torch.complex64
    _assert_exact(y, exact, 1.0, f"bank cf32 C={Cn} T={T} D={D} shift={shift} index0={index0} over three trips")
    raw, wide = _sc16_and_its_widened_samples(S, T + Cn)
    got = bank.filter_bank(raw, taps, Cn, D, shift=shift, sample_index0=index0)
    assert _same_bytes(got, bank.filter_bank(wide, taps, Cn, D, shift=shift, sample_index0=index0))
    _assert_exact(got, exact, ce.UNIT["sc16"], f"bank sc16 C={Cn} T={T} D={D} over three trips")
