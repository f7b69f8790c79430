"""tests/chain_exact.py on the CPU: the int64 results are the definitions' (against the float64 references of tests/ddc_ref.py,
bank_ref.py and resample_ref.py on the same data), the numpy models of the three kernels meet them with ==, the 2^24 cap holds
for every GPU case, and the comparison sees ONE term of ONE output, dropped or doubled, at the full tap counts.  Needs no GPU."""
import numpy as np
import pytest

from amcpy_amd import _formats, _lib, ddc
from tests import bank_ref, chain_exact as ce, ddc_ref, resample_ref

TURNS = list(range(4))


def _phases(shift, index0):
    step = ddc.phase_step_of(shift)
    return (int(index0) * step) & ddc_ref.MASK64, step


def _wide(k, fmt):
    return ddc_ref.widen(ce.encode(k, fmt), fmt, _formats.get(fmt).scale)


def _close(exact, g, y64, s):
    """the int64 result against a float64 reference: to 1e-12 S"""
    err = np.abs((exact[0] + 1j * exact[1]) * g - y64)
    return bool(np.all(err <= 1e-12 * np.broadcast_to(s, err.shape)))


def _snap(y, g):
    """The numpy models mix with exp() in float64, whose quarter turns are off by 6e-17 (cos(pi / 2) is not 0 there): a mixed
    component is its integer plus at most 1e-14 of a unit, a sum of 4096 terms its integer plus at most 1e-9.  That rounds to
    the right float32 wherever the integer is not 0, and to 1e-9 g where it is -- which is not == 0.  So the models' outputs
    are rounded to whole units first, after the check that this moves nothing by more than 1e-6 of a unit; a lost term is a
    whole unit or more.  What comes out must EQUAL the int64 result."""
    y = np.asarray(y).astype(np.complex128) / g
    r = np.rint(y.real) + 1j * np.rint(y.imag)
    assert np.abs(y - r).max(initial=0.0) < 1e-6
    return (r * g).astype(np.complex64)


def test_the_formats_carry_the_same_values_and_the_scales_are_powers_of_two():
    assert tuple(ddc.FORMATS) == ce.FORMATS
    for fmt in ce.FORMATS:
        scale = _formats.get(fmt).scale
        assert np.frexp(scale)[0] == 0.5 and np.frexp(ce.UNIT[fmt])[0] == 0.5
        assert ce.UNIT[fmt] == scale * (256 if fmt == "sc16" else 1)
    k = ce.make_ints(1000)
    assert k.min() == -128 and not (k == 0).any() and np.abs(k).max() == ce.K_MAX
    for fmt in ce.FORMATS:
        x = ce.encode(k, fmt)
        assert x.dtype == ce.NUMPY[fmt] and x.dtype == _formats.get(fmt).plain and ddc._format_of(x) == fmt
        w = _wide(k, fmt)
        assert np.array_equal(w.real, k[:, 0] * ce.UNIT[fmt]) and np.array_equal(w.imag, k[:, 1] * ce.UNIT[fmt]), fmt
    assert ce.encode(k, "sc16").min() == -32768 and ce.encode(k, "cu8").min() == 0 and ce.encode(k, "ci8").min() == -128
    h = ce.make_taps(4096)
    assert h.dtype == np.float32 and np.array_equal(h, np.rint(h)) and np.abs(h).min() == 1 and np.abs(h).max() == ce.H_MAX


def test_the_cap_holds_for_every_gpu_case():
    for T, _ in ce.DDC_CASES:
        assert T <= ddc.MAX_TAPS
        ce.check_cap(T)
    for T, _, _ in ce.RESAMPLE_CASES:
        ce.check_cap(T)
    for _, T, _ in ce.BANK_EXACT_CASES + ce.BANK_TRANSFORM_CASES:
        ce.check_cap(T)
    assert 4096 * ce.H_MAX * ce.K_MAX == 1 << 22
    with pytest.raises(AssertionError):
        ce.check_cap(4096, 32, 128)
    with pytest.raises(AssertionError):
        ce.int_taps(np.full(4096, 32.0, np.float32))
    with pytest.raises(AssertionError):
        ce.int_taps(np.array([1.5], np.float32))
    assert ce.BANK_LDS_MAX_CASE in ce.BANK_EXACT_CASES
    assert {c for c, _, _ in ce.BANK_EXACT_CASES} == {2, 4} and min(c for c, _, _ in ce.BANK_TRANSFORM_CASES) == 8


def test_the_mixer_at_quarter_turns():
    """v = x j^((index0 + n) qs) against exp() in float64, and the four settings leave four different q0"""
    k = ce.make_ints(64)
    seen = set()
    for shift, index0 in ce.QUARTER_TURNS + ce.BANK_QUARTER_TURNS:
        p0, step = _phases(shift, index0)
        assert step % (1 << 62) == 0 and p0 % (1 << 62) == 0
        re, im = ce.mix(k, shift, index0)
        want = (k[:, 0] + 1j * k[:, 1]) * np.exp(2j * np.pi * ddc_ref.phases(np.arange(64), p0, step))
        assert np.abs(re + 1j * im - want).max() < 1e-10
        seen.add((step >> 62, p0 >> 62))
    assert {s for s, _ in seen} == {0, 1, 2, 3} and len(seen) >= 6
    for _, index0 in ce.BANK_QUARTER_TURNS:
        assert index0 % 2 == 1


@pytest.mark.parametrize("T,D,M", ce.DDC_SMALL)
@pytest.mark.parametrize("turn", TURNS)
def test_down_converter(T, D, M, turn):
    shift, index0 = ce.QUARTER_TURNS[turn]
    p0, step = _phases(shift, index0)
    S = ce.ddc_span(M, T, D)
    k, h = ce.make_ints(S, T), ce.make_taps(T)
    assert ddc.out_samples(S, T, D) == M
    exact = ce.ddc_exact(ce.mix(k, shift, index0), h, D, M)
    for fmt in ce.FORMATS:
        y64, s = ddc_ref.reference(_wide(k, fmt), h, D, p0, step)
        assert y64.shape == (M,) and _close(exact, ce.UNIT[fmt], y64, s), (fmt, T, D)
        y = ddc_ref.numpy_ddc(ce.encode(k, fmt), h, D, shift=shift, sample_index0=index0)
        assert ce.mismatches(_snap(y, ce.UNIT[fmt]), exact, ce.UNIT[fmt]) == 0, (fmt, T, D)


@pytest.mark.parametrize("T,L,D,M", ce.RESAMPLE_SMALL)
@pytest.mark.parametrize("turn", TURNS)
def test_resampler(T, L, D, M, turn):
    shift, index0 = ce.QUARTER_TURNS[turn]
    p0, step = _phases(shift, index0)
    h = ce.make_taps(T)
    for tau0 in sorted({0, L - 1}):
        S, M1 = ce.resample_span(M, T, L, D, tau0)
        assert resample_ref.out_samples(S, T, L, D, tau0) == M1 == resample_ref.out_samples_brute(S, T, L, D, tau0)
        k = ce.make_ints(S, T + tau0)
        exact = ce.resample_exact(ce.mix(k, shift, index0), h, L, D, tau0, M1)
        for fmt in ce.FORMATS:
            y64, s = resample_ref.reference(_wide(k, fmt), h, L, D, tau0, p0, step)
            assert y64.shape == (M1,) and _close(exact, ce.UNIT[fmt], y64, s), (fmt, T, L, D, tau0)
            y = resample_ref.numpy_resample(ce.encode(k, fmt), h, L, D, shift=shift, sample_index0=index0, phase_index0=tau0)
            assert ce.mismatches(_snap(y, ce.UNIT[fmt]), exact, ce.UNIT[fmt]) == 0, (fmt, T, L, D, tau0)
        if T < L:                                           # phases without a tap: exactly 0
            t = np.arange(M1) * D + tau0
            assert (t % L >= T).any() and not exact[0][t % L >= T].any() and not exact[1][t % L >= T].any()
        if L == 1:                                          # interp 1 is the down-converter
            same = ce.ddc_exact(ce.mix(k, shift, index0), h, D, M1)
            assert np.array_equal(same[0], exact[0]) and np.array_equal(same[1], exact[1])


@pytest.mark.parametrize("C,T,D,M", ce.BANK_SMALL)
@pytest.mark.parametrize("turn", TURNS)
def test_filter_bank(C, T, D, M, turn):
    shift, index0 = ce.BANK_QUARTER_TURNS[turn]
    p0, step = _phases(shift, index0)
    S = ce.ddc_span(M, T, D)
    k, h = ce.make_ints(S, C + T), ce.make_taps(T)
    v = ce.mix(k, shift, index0)
    u = ce.bank_branch_sums(v, h, C, D, M, index0)
    other = ce.bank_branch_sums(v, h, C, D, M, index0, gather=C <= 8)             # the other of the two ways
    assert np.array_equal(u[0], other[0]) and np.array_equal(u[1], other[1])
    total = ce.ddc_exact(v, h, D, M)                                              # channel 0 is the plain sum
    assert np.array_equal(u[0].sum(axis=1), total[0]) and np.array_equal(u[1].sum(axis=1), total[1])
    y_any = ce.bank_float64(u, C)
    fmt = ce.FORMATS[turn]
    g = ce.UNIT[fmt]
    y64, s = bank_ref.reference_by_definition(_wide(k, fmt), h, C, D, p0, step, index0)
    assert y64.shape == (C, M) and bool(np.all(np.abs(y_any * g - y64) <= 1e-12 * s[None, :])), (C, T, D)
    assert np.allclose(ce.abs_sums(k, h, D, M) * g, s, rtol=1e-13, atol=0)
    if C <= 4:
        exact = ce.bank_exact(u, C)
        assert np.array_equal(exact[0] + 1j * exact[1], y_any)                    # the table's quarter turns are exact
        for f in ce.FORMATS:
            y = bank_ref.numpy_bank(ce.encode(k, f), h, C, D, shift=shift, sample_index0=index0)
            assert ce.mismatches(_snap(y, ce.UNIT[f]), exact, ce.UNIT[f]) == 0, (f, C, T, D)


def _seen(exact, g, wrong):
    """the outputs at which an expected array that is wrong differs from the float32 image of the right one"""
    re, im = ce.as_float32(exact, g)
    return ce.mismatches((re + 1j * im).astype(np.complex64), wrong, g)


def test_one_term_is_seen_at_the_full_tap_counts():
    """What the exact tests are for.  At the largest shapes, with M = 2 tile + 3 as on the GPU, the float32 image of the right
    result differs from an expected array with ONE term of ONE output dropped, and from one with it doubled, at exactly that
    output -- for the first tap, the last tap, one tap per phase and the outputs on both sides of a tile seam.  (Against the
    derived bound the same term is a coin flip there: tests/ddc_ref.py.)"""
    shift, index0 = ce.QUARTER_TURNS[1]
    for fmt in ("cf32", "ci8"):
        g = ce.UNIT[fmt]
        # the down-converter at T = 2048
        T, D = 2048, 5
        tile, _ = _lib.tune_decimate_plan(T, D)
        M = 2 * tile + 3
        k, h = ce.make_ints(ce.ddc_span(M, T, D)), ce.make_taps(T)
        v = ce.mix(k, shift, index0)
        exact = ce.ddc_exact(v, h, D, M)
        assert _seen(exact, g, exact) == 0
        for m in (0, tile - 1, tile, 2 * tile, M - 1):
            for tap in (0, 1, T // 2, T - 2, T - 1):
                n = m * D + T - 1 - tap
                term = (int(h[tap]) * v[0][n], int(h[tap]) * v[1][n])
                assert term != (0, 0)
                for factor in (-1, 1):
                    assert _seen(exact, g, ce.without_term(exact, term, m, factor)) == 1, (fmt, m, tap, factor)
        # the resampler at P = 4096 (one phase) and at seven phases of 585 taps, the last of 584
        for T, L, D in ((4096, 1, 1), (4093, 7, 5)):
            tile = _lib.resample_plan(T, L, D)[0]
            tau0 = L - 1
            S, M = ce.resample_span(2 * tile + 3, T, L, D, tau0)
            k, h = ce.make_ints(S, L), ce.make_taps(T)
            v = ce.mix(k, shift, index0)
            exact = ce.resample_exact(v, h, L, D, tau0, M)
            P = ce.phase_taps(T, L)
            t = np.arange(M) * D + tau0
            phase, top = t % L, (P - 1) + t // L
            first_of_phase = [int(np.nonzero(phase == p)[0][0]) for p in range(L)]
            assert len(first_of_phase) == L
            for m in sorted(set(first_of_phase) | {tile - 1, tile, 2 * tile, M - 1}):
                n_q = len(range(int(phase[m]), T, L))
                for q in (0, n_q // 2, n_q - 1):
                    tap, n = int(phase[m]) + q * L, int(top[m]) - q
                    term = (int(h[tap]) * v[0][n], int(h[tap]) * v[1][n])
                    for factor in (-1, 1):
                        assert _seen(exact, g, ce.without_term(exact, term, m, factor)) == 1, (fmt, T, L, m, q, factor)
