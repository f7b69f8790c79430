"""Blind carrier recovery (include/amcx.h, amcx_carrier_c64; ABI 16.2.3) on the GPU.

THE REFERENCE is tests/carrier_ref.py: the contract in numpy float32, operation by operation.  Every field of a record but
phase0, and every output sample restated from the record the device wrote, is compared with ==; phase0 -- the one value that
goes through a library routine, atan2f -- is held to the bound derived there around the float64 atan2 of the restated Z[bin],
and the worst ratio is printed.  The kernel against itself (another place in the call, two calls, a graph replay) as bytes.
The end-to-end caps are the ones tests/test_carrier_host.py holds the float64 estimator to on the same rows."""
import json

import numpy as np
import pytest

from amcpy_amd import _lib, carrier, waveform as wf
from tests import carrier_ref as ref
from tests import test_carrier_host as host
from tests.plain_grids import LINE

pytestmark = pytest.mark.gpu

SENTINEL = np.complex64(-7.0 - 9.0j)
ALL = ref.GAIN | ref.FREQ | ref.PHASE
EXACT_FIELDS = ("phase_step", "bin", "frac", "power", "gain", "quality")


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to("cuda")


def _cpu(t):
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def _records(est) -> np.ndarray:
    _torch().cuda.synchronize()
    return est.numpy()


def _padded(x, pad=3):
    """x (R, N) on the device as the first N columns of a (R, N + pad) buffer filled with a sentinel: odd rows begin on 8 but not 16 bytes"""
    torch = _torch()
    R, N = x.shape
    buf = torch.full((R, N + pad), complex(SENTINEL), dtype=torch.complex64, device="cuda")
    buf[:, :N] = _dev(x)
    return buf, buf[:, :N]


def _same_fields(got, want, fields=EXACT_FIELDS):
    for name in fields:
        g, w = got[name], want[name]
        both_nan = np.isnan(g) & np.isnan(w) if g.dtype.kind == "f" else np.zeros(g.shape, bool)
        assert np.all((g == w) | both_nan), (name, np.flatnonzero(~((g == w) | both_nan))[:4], g[:4], w[:4])


def _phase0_ratio(got, spec, order) -> float:
    """max over the good rows of (distance of the device's phase0 from the restated one) / its tolerance"""
    N, worst = spec["N"], 0.0
    for r in np.flatnonzero(~spec["bad"]):
        k = int(got["bin"][r]) % N
        zre, zim = spec["Zre"][r, k], spec["Zim"][r, k]
        want = ref.phase_word(ref.angle_word64(zre, zim), got["frac"][r], N, order)
        worst = max(worst, ref.phase0_distance(int(got["phase0"][r]), want, order) / ref.phase0_tolerance(zre, zim, order))
    return worst


def _rows(R, N, seed, order=4):
    """test rows: QPSK at 4 samples per symbol with drawn offsets inside N / 16 bins of x^M, phases and noise, at an odd level"""
    return ref.qpsk_rows(R, N, seed, cfo=0.9 * (N // 16) / (order * N), level=0.37)[0]


# ---- the restatement, by == -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ref.ORDERS)
@pytest.mark.parametrize("N", [64, 128, 256, 512, 1024, 2048, 4096])
def test_records_and_rows_equal_the_restatement(N, order):
    """Every size: 3 + 3, 3 + 4, 4 + 4, 3 + 3 + 3, 3 + 3 + 4, 3 + 4 + 4 and 4 + 4 + 4 passes; 64 ... 1 rows per workgroup, 4 ... 256
    threads per row (64: exactly one wave, no LDS level; 128: the pair sums of the tree and of the peak); one row, and three
    workgroups the last with one live slot; four search ranges; rows at a stride of N + 3 in and out, out's padding untouched."""
    torch = _torch()
    G = 4096 // N
    R = 2 * G + 1
    x = _rows(R, N, seed=1000 + N + order, order=order)
    spec = ref.spectrum32(x, order)
    worst = 0.0
    for rows in (1, R):
        _, xin = _padded(x[:rows])
        for sb in (0, 1, N // 16, N // 2 - 1):
            want = ref.estimate32(x[:rows], order, sb, {k: (v[:rows] if isinstance(v, np.ndarray) else v) for k, v in spec.items()})
            obuf = torch.full((rows, N + 3), complex(SENTINEL), dtype=torch.complex64, device="cuda")
            y, est = carrier.recover(xin, order, out=obuf[:, :N], search_bins_=sb)
            got = _records(est)
            _same_fields(got, want["rec"])
            worst = max(worst, _phase0_ratio(got, want, order))
            out = _cpu(obuf)
            assert np.all(out[:, N:] == SENTINEL)
            assert np.array_equal(out[:, :N].view(np.uint32), ref.apply32(x[:rows], got, ALL).view(np.uint32)), (rows, sb)
            only = _records(carrier.estimate(xin, order, search_bins_=sb))              # estimate only: the same records
            assert only.tobytes() == got.tobytes()
    print(f"N={N} M={order}: worst phase0 distance / tolerance = {worst:.3f}")
    assert worst <= 1.0


# ---- exact cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 128, 256, 512, 1024, 2048, 4096])
def test_quarter_rate_tone_is_recovered_exactly(N):
    x = (1j ** (np.arange(N) % 4)).astype(np.complex64)[None, :]
    y, est = carrier.recover(_dev(x), 1, search_bins_=N // 2 - 1)
    rec = _records(est)[0]
    assert (rec["bin"], rec["frac"], rec["phase_step"], rec["phase0"]) == (N // 4, 0.0, 1 << 62, 0)
    assert rec["power"] == 1.0 and rec["gain"] == 1.0 and rec["quality"] == 1.0
    assert np.all(_cpu(y) == np.complex64(1.0 + 0.0j))


def test_impulse_ties_go_to_the_lowest_signed_bin():
    for N, sb in ((64, 31), (512, 32), (4096, 5)):
        x = np.zeros((1, N), np.complex64)
        x[0, 0] = 3.0
        rec = _records(carrier.estimate(_dev(x), 1, search_bins_=sb))[0]
        assert rec["bin"] == -sb and rec["power"] == np.float32(9.0 / N) and rec["frac"] == 0.0      # den = 0: NaN, which is not <= 0.5


def _tones(N, parts):
    n = np.arange(N)
    return sum(a * np.exp(2j * np.pi * k * n / N) for k, a in parts).astype(np.complex64)[None, :]


def test_tones_at_the_edge_of_the_range_are_found_and_one_beyond_it_is_not_chosen():
    N, sb = 512, 20
    for k in (sb, -sb):
        rec = _records(carrier.estimate(_dev(_tones(N, [(k, 1.0)])), 1, search_bins_=sb))[0]
        assert rec["bin"] == k
        out = np.sign(k) * (sb + 1)
        x = _tones(N, [(k // 2, 1.0), (out, 4.0)])
        rec = _records(carrier.estimate(_dev(x), 1, search_bins_=sb))[0]
        assert rec["bin"] == k // 2
        assert _records(carrier.estimate(_dev(x), 1, search_bins_=sb + 1))[0]["bin"] == out


SIZES = (64, 128, 256, 512, 1024, 2048, 4096)


def _exact_tones(N, parts):
    """sum of a exp(2 pi j k n / N) per row: parts is ((k (R,), a), ...), k in bins -- whole or dyadic fractions, so that k n is
    exact in float64 and is reduced mod N before the angle is formed -- -> complex64 (R, N)"""
    n = np.arange(N, dtype=np.float64)[None, :]
    x = np.zeros((len(parts[0][0]), N), np.complex128)
    for k, a in parts:
        index = np.fmod(np.asarray(k, dtype=np.float64)[:, None] * n, float(N))
        if np.all(index == np.rint(index)):                                # whole bins: the N angles there are, looked up
            wave = np.exp(2j * np.pi * (np.arange(N) / N))[index.astype(np.int64) % N]
        else:
            wave = np.exp(2j * np.pi * (index / N))
        x += np.asarray(a).reshape(-1, 1) * wave                             # (a real or complex, float64 / complex128)
    return x.astype(np.complex64)


@pytest.mark.parametrize("N", SIZES)
def test_the_peak_is_found_in_every_bin_and_nowhere_outside_the_range(N):
    """One row per signed bin k = -N / 2 ... N / 2 - 1 and search range sb: a tone of amplitude 4 at k and one of amplitude 1 at
    m = (k mod (2 sb + 1)) - sb, which lies inside the range (m = k: the single tone).  The record's bin is k where |k| <= sb
    and m otherwise -- no tolerance: the second line is 12 dB down and the leakage of whole-bin tones is at rounding level.
    So every lane's signed-bin mapping through the bit reversal, every lane's skip of the bins outside the range and the
    cross-wave reduction with the winner in any wave are asked for, at every size.  Every field but phase0 against the
    restatement too: on all rows for N <= 1024; at 2048 and 4096 on the lowest 64 bins of the transform, the highest 64 (the
    signed bins -64 ... 63) and 128 seeded ones between (a cap on the reference's time; `bin` is checked on every row).  A failure lists the bins: a shared residue points at the bit reversal,
    a shared run of 16 at a lane, a shared wave at the LDS level."""
    k = np.arange(-N // 2, N // 2)
    some = np.arange(N)
    if N > 1024:                                                          # FFT bins: signed bin k stands in row k + N / 2
        between = np.random.default_rng([41, N]).choice(np.arange(64, N - 64), 128, replace=False)
        cut = np.concatenate([np.arange(64), between, np.arange(N - 64, N)])
        some = np.sort((cut + N // 2) % N)
        assert some.size == 256 == np.unique(some).size
    for sb in (0, 1, N // 16, N // 2 - 1):
        m = k % (2 * sb + 1) - sb
        x = _exact_tones(N, ((k, 4.0), (m, np.where(m == k, 0.0, 1.0))))
        want_bin = np.where(np.abs(k) <= sb, k, m)
        got = _records(carrier.estimate(_dev(x), 1, search_bins_=sb))
        wrong = np.flatnonzero(got["bin"] != want_bin)
        assert wrong.size == 0, (f"N={N} sb={sb}: {wrong.size} rows with the wrong bin; k, got, expected: "
                                 f"{[(int(k[r]), int(got['bin'][r]), int(want_bin[r])) for r in wrong[:48]]}")
        want = ref.estimate32(x[some], 1, sb)["rec"]
        assert np.array_equal(want["bin"], want_bin[some])
        _same_fields(got[some], want)
    print(f"N={N}: {4 * N} rows, every bin in four ranges; {some.size} rows per range against the restatement")


@pytest.mark.parametrize("N", [64, 1024, 2048, 4096])
def test_tones_between_bins_equal_the_restatement_at_the_cut(N):
    """Unit tones at k + f, f = 1/4, 1/2 - 2^-10, 1/2, 1/2 + 2^-10 and 3/4, for 32 seeded k of both signs with 0, -1 and N / 2 - 2
    among them, the whole range searched: every field but phase0 by ==, phase0 within its bound, the output rows the bytes of
    the restatement applied to the device's records.

    WHAT IS HELD: the device takes the same side of the `|frac| <= 0.5` cut as the restatement does on the same bits, and
    writes the same words for it.  WHAT IS NOT: the estimator's accuracy at a half bin.  A tone half a bin off has two equal
    lines; whichever wins, the interpolated frac is +-0.5 give or take a rounding, and where it lands beyond the cut the
    contract sets it to 0 -- the record is then half a bin off.  That is the contract's known weakness, not an error of the
    kernel; the count of such rows is printed.

    The lone tones all stay inside the cut: the interpolation is exact for one line.  So 4 x 32 rows more stand AT it.  PUSHED:
    the tone at k + 1/2 - 2^-10 with a line of +-2^-6 at k - 1 in phase with the tone's own leakage there; + widens Z[k - 1]
    and puts frac beyond 0.5, - keeps it inside.  PAIRED: whole-bin lines of 1.5 at k and 1 at k + 1 or k - 1, num / den =
    -+1 / 2 but for the transform's roundings: at every size some of the 32 rows land on |frac| = 0.5 exactly (kept: <=), some
    an ulp beyond (cut to 0) and some an ulp inside -- the test asserts that the restatement has all three on either side.

    IF THAT ASSERTION FAILS (before anything runs on the device), the rows are no longer what they were made for: they are built
    with numpy's float64 exp, and which of the 32 land where depends on its last bits.  Nothing is wrong with the kernel then.
    Draw other k (the seed 17 below) or other amplitudes of the same ratio (3 and 2, 0.75 and 0.5) until the restatement has
    all three cases on either side at every size again; the comparison with the device needs no change."""
    order, sb = 1, N // 2 - 1
    rng = np.random.default_rng([N, 17])
    pool = np.setdiff1d(np.arange(-N // 2 + 1, N // 2 - 1), [0, -1, N // 2 - 2])
    ks = np.concatenate([[0, -1, N // 2 - 2], rng.choice(pool, 29, replace=False)])
    assert (ks < 0).sum() >= 4 and (ks > 0).sum() >= 4
    fs = np.array([0.25, 0.5 - 2.0 ** -10, 0.5, 0.5 + 2.0 ** -10, 0.75])
    at = (ks[:, None] + fs[None, :]).reshape(-1)
    x = _exact_tones(N, ((at, 1.0),))
    # PUSHED (the leakage of a tone at k + 1/2 in bin k - 1 is i / pi N / 1.5: the second line is imaginary) and PAIRED
    near, n_k = ks + fs[1], ks.size
    pushed = [_exact_tones(N, ((near, np.ones(n_k)), (ks - 1, np.full(n_k, s * 2.0 ** -6 * 1j)))) for s in (1.0, -1.0)]
    paired = [_exact_tones(N, ((ks, np.full(n_k, 1.5)), (ks + side, np.ones(n_k)))) for side in (1, -1)]
    x = np.concatenate([x] + pushed + paired)
    want = ref.estimate32(x, order, sb)
    made = want["rec"]["frac"][at.size:].reshape(4, n_k)                       # of the restatement: what the rows were made for
    assert (made[0] == 0).all() and not (made[1] == 0).any()
    for side in (2, 3):
        assert (np.abs(made[side]) == 0.5).any() and (made[side] == 0).any() and ((made[side] != 0) & (np.abs(made[side]) < 0.5)).any()
    assert np.array_equal(want["rec"]["bin"][at.size:].reshape(4, n_k), np.tile(ks, (4, 1)))
    _, xin = _padded(x)
    y, est = carrier.recover(xin, order, search_bins_=sb)
    got = _records(est)
    lone, extra = got["frac"][:at.size].reshape(n_k, fs.size), got["frac"][at.size:].reshape(4, n_k)
    count = lambda rows: rows.sum(axis=-1).tolist()                           # noqa: E731  rows of a block that meet a condition
    print(f"N={N}: {x.shape[0]} rows, {int((got['frac'] == 0).sum())} fell to frac = 0 at the cut "
          f"(restatement: {int((want['rec']['frac'] == 0).sum())})")
    print(f"  lone tones, {n_k} per f = {fs.tolist()}: {count((lone == 0).T)} at 0")
    print(f"  pushed, {n_k} per sign: {count(extra[:2] == 0)} at 0;  paired, {n_k} per side: {count(extra[2:] == 0)} at 0, "
          f"{count(np.abs(extra[2:]) == 0.5)} on |frac| = 0.5 exactly")
    _same_fields(got, want["rec"])
    worst = _phase0_ratio(got, want, order)
    print(f"N={N}: worst phase0 distance / tolerance = {worst:.3f}")
    assert worst <= 1.0
    assert np.array_equal(_cpu(y).view(np.uint32), ref.apply32(x, got, ALL).view(np.uint32))


def test_peak_at_bin_0_reads_its_neighbour_at_n_minus_1():
    """Z[-1] = 0.6 N beside Z[0] = N and Z[1] = 0.05 N, all in phase: num = -0.55 N, den = 1.35 N, frac = +0.55 / 1.35 -- and the
    mirror image gives its negative; a kernel that read Z[1] for Z[-1], or index -1, would give neither."""
    for N in (64, 1024):
        x = _tones(N, [(0, 1.0), (-1, 0.6), (1, 0.05)])
        want = ref.estimate32(x, 1, 3)["rec"]
        got = _records(carrier.estimate(_dev(x), 1, search_bins_=3))
        _same_fields(got, want)
        assert got["bin"][0] == 0 and abs(got["frac"][0] - 0.55 / 1.35) < 1e-4
        mirrored = _records(carrier.estimate(_dev(_tones(N, [(0, 1.0), (1, 0.6), (-1, 0.05)])), 1, search_bins_=3))
        assert mirrored["bin"][0] == 0 and abs(mirrored["frac"][0] + 0.55 / 1.35) < 1e-4


@pytest.mark.parametrize("N", [64, 256, 1024, 2048, 4096])
def test_zero_nan_and_inf_rows_leave_their_neighbours_alone(N):
    good = _rows(4, N, seed=77)
    x = np.stack([good[0], np.zeros(N, np.complex64), good[1], np.full(N, np.nan + 0j, np.complex64), good[2],
                  np.full(N, 1e30 + 1e30j, np.complex64), good[3]])
    x[5, 7] = np.inf                                                          # row 5: |x|^2 overflows, and one sample is inf
    y, est = carrier.recover(_dev(x), 4)
    rec, out = _records(est), _cpu(y)
    y0, est0 = carrier.recover(_dev(good), 4)
    rec0, out0 = _records(est0), _cpu(y0)
    assert rec[[0, 2, 4, 6]].tobytes() == rec0.tobytes() and out[[0, 2, 4, 6]].tobytes() == out0.tobytes()
    for r, power in ((1, 0.0), (3, np.nan), (5, np.inf)):
        assert (np.isnan(rec["power"][r]) if np.isnan(power) else rec["power"][r] == power), (r, rec["power"][r])
        for name in ("phase_step", "phase0", "bin", "frac", "gain", "quality"):
            assert rec[name][r] == 0, (r, name)
        assert np.all(out[r].view(np.uint32) == 0)
    _same_fields(rec, ref.estimate32(x, 4, N // 16)["rec"])


# ---- GIVEN ------------------------------------------------------------------------------------------------------------------------
def test_given_records_are_applied_as_numpy_applies_them():
    N, R = 256, 19
    x = _rows(R, N, seed=5)
    rec = np.zeros(R, ref.RECORD)
    rng = np.random.default_rng(9)
    rec["phase_step"] = rng.integers(-(1 << 63), (1 << 63) - 1, R, dtype=np.int64)      # both signs; n * step wraps 2^64
    rec["phase_step"][:4] = [0, 1 << 62, -(1 << 62), (1 << 63) - 1]
    rec["phase0"] = rng.integers(0, 1 << 32, R, dtype=np.uint64).astype(np.uint32)
    rec["gain"] = rng.uniform(0.1, 9.0, R).astype(np.float32)
    est = carrier.Estimates.from_numpy(rec, N, 4, device="cuda")
    _, xin = _padded(x)
    for flags in (ref.GAIN, ref.FREQ, ref.PHASE, ALL, 0):
        y = _cpu(carrier.apply(xin, est, gain=bool(flags & ref.GAIN), freq=bool(flags & ref.FREQ), phase=bool(flags & ref.PHASE)))
        assert np.array_equal(y.view(np.uint32), ref.apply32(x, rec, flags).view(np.uint32)), flags
        if flags == 0:
            assert np.array_equal(y, x)                                       # the product by 1 + 0j: the finite values come back
    assert _records(est).tobytes() == rec.tobytes()                           # GIVEN: the records are input


def test_combined_estimates_put_one_frequency_on_every_frame_of_an_emitter():
    N = 1024
    x = _rows(12, N, seed=21)
    xd = _dev(x)
    est = carrier.estimate(xd, 4)
    one = carrier.combine(est, 4)
    rec, got = _records(est), _records(one)
    for g in range(3):
        assert np.all(got["phase_step"][4 * g:4 * g + 4] == np.sort(rec["phase_step"][4 * g:4 * g + 4])[1])
    y = _cpu(carrier.apply(xd, one))
    assert np.array_equal(y.view(np.uint32), ref.apply32(x, got, ALL).view(np.uint32))


# ---- position independence, as bytes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,order", [(64, 2), (256, 4), (2048, 8), (4096, 1)])
def test_a_row_is_the_same_bytes_wherever_it_stands(N, order):
    G = 4096 // N
    R = 2 * G + 3
    x = _rows(R, N, seed=N)
    xd = _dev(x)
    y, est = carrier.recover(xd, order)
    rec, out = _records(est), _cpu(y)
    probe = x[5 % R]
    for at in sorted({1, G // 2, G - 1, G, R - 1} - {0}):                       # other slots, the first slot of the next workgroup, the last row
        moved = x.copy()
        moved[at] = probe
        y2, est2 = carrier.recover(_dev(moved), order)
        assert _records(est2)[at].tobytes() == rec[5 % R].tobytes() and _cpu(y2)[at].tobytes() == out[5 % R].tobytes(), at
    alone_y, alone = carrier.recover(_dev(probe[None, :]), order)
    assert _records(alone)[0].tobytes() == rec[5 % R].tobytes() and _cpu(alone_y)[0].tobytes() == out[5 % R].tobytes()
    # the rows cut into two calls, the cut inside a workgroup's group
    cut = G + 1
    ya, ea = carrier.recover(xd[:cut], order)
    yb, eb = carrier.recover(xd[cut:], order)
    assert _records(ea).tobytes() + _records(eb).tobytes() == rec.tobytes()
    assert _cpu(ya).tobytes() + _cpu(yb).tobytes() == out.tobytes()


def _rows_equal_base(big, base, period, points=1 << 24):
    """big[r] == base[r mod period] as bytes for every row r, compared on the device in slabs of `points` 4-byte words"""
    torch = _torch()
    R, width = int(big.shape[0]), int(big.shape[1])
    step = max(1, points // width)
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        index = torch.arange(r0, r1, device=big.device) % period
        if not torch.equal(big[r0:r1], base[index]):
            bad = torch.nonzero((big[r0:r1] != base[index]).any(dim=1))[:4].flatten().tolist()
            return [r0 + r for r in bad]
    return []


@pytest.mark.parametrize("N,order", [(64, 4), (4096, 1)])
def test_rows_over_two_lines_of_the_grid(N, order):
    """LINE + 1 workgroups -- 64 slots each, and one: the launch is folded into two lines, so the `blockIdx.y` term, the
    whole-workgroup return of the 65 535 workgroups behind the last one, and `r * stride` and `est[r]` at rows of 2^22 and more
    (N = 64) are executed.  A carrier workgroup always holds 4096 points, so LINE + 1 groups are 2.1 GB of input whatever N:
    that is why this case stops at two lines, the second with one live workgroup.  A third line would double the memory and add
    only a repeat of the second.

    The rows are a base of B rows repeated on the device (B coprime to the slots per workgroup: a base row lands in every
    slot); nothing of this size crosses the host.  The base alone is a call of at most 16 workgroups, the shape the tests above
    hold to the restatement, and is held to it here again; record r and output row r of the large call are the bytes of the
    base call's r mod B -- from recover, from estimate, and from apply (GIVEN: est[r0 + tid] is read at r0 >= 2^22).  Records
    and rows are written into buffers one row longer, filled with 0xFF: the row beyond keeps them."""
    torch = _torch()
    G = 4096 // N
    R = LINE * G + 1
    groups = -(-R // G)
    print(f"carrier N={N}: {R} rows in {groups} workgroups, LINE = {LINE}")
    assert groups >= LINE + 1
    assert _lib.carrier_plan(N)[0] == G
    B = 997 if N < 4096 else 13
    assert np.gcd(B, G) == 1
    base = _rows(B, N, seed=500 + N, order=order)
    base_dev = _dev(base)
    yb, eb = carrier.recover(base_dev, order)
    rec_b = _records(eb)
    want = ref.estimate32(base, order, N // 16)
    _same_fields(rec_b, want["rec"])
    worst = _phase0_ratio(rec_b, want, order)
    print(f"carrier N={N}: the base's worst phase0 distance / tolerance = {worst:.3f}")
    assert worst <= 1.0
    assert np.array_equal(_cpu(yb).view(np.uint32), ref.apply32(base, rec_b, ALL).view(np.uint32))
    i32 = lambda t: torch.view_as_real(t).view(torch.int32)                   # noqa: E731  (R, N) complex64 -> (R, 2 N) words
    x = out = again = raw = None
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    try:
        x = base_dev.repeat(-(-R // B), 1)[:R]
        assert x.is_contiguous() and x.shape == (R, N)
        out = torch.empty((R + 1, N), dtype=torch.complex64, device="cuda")
        i32(out).fill_(-1)
        y, est = carrier.recover(x, order, out=out[:R])
        assert len(est) == R and _rows_equal_base(est.raw, eb.raw, B) == []
        assert _rows_equal_base(i32(y), i32(yb), B) == []
        assert bool((i32(out)[R] == -1).all())
        # estimate only, into a buffer of R + 1 records
        raw = torch.full((R + 1, carrier.RECORD_BYTES), 255, dtype=torch.uint8, device="cuda")
        _lib.check(_lib.load().amcx_carrier_c64(x.data_ptr(), R, N, N, order, N // 16, 0, raw.data_ptr(), None, 0,
                                                torch.cuda.current_stream().cuda_stream))
        assert torch.equal(raw[:R], est.raw) and bool((raw[R] == 255).all())
        assert torch.equal(carrier.estimate(x, order).raw, est.raw)
        # GIVEN
        again = torch.empty((R + 1, N), dtype=torch.complex64, device="cuda")
        i32(again).fill_(-1)
        assert carrier.apply(x, est, out=again[:R]) is not None
        assert torch.equal(i32(again), i32(out))
        assert torch.equal(raw[:R], est.raw)                                  # GIVEN: the records are input
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        print(f"carrier N={N}: peak device memory {peak / 1e9:.2f} GB")
        assert peak < 10e9
    finally:
        del x, out, again, raw
        y = est = None
        torch.cuda.empty_cache()


def test_graph_replay_equals_the_plain_call():
    torch = _torch()
    N, R, order = 512, 21, 4
    x = _dev(_rows(R, N, seed=3))
    want_y, want = carrier.recover(x, order)
    want_rec, want_out = _records(want), _cpu(want_y)
    out = torch.zeros((R, N), dtype=torch.complex64, device="cuda")
    raw = torch.zeros((R, 32), dtype=torch.uint8, device="cuda")
    lib = _lib.load()

    def launch():
        _lib.check(lib.amcx_carrier_c64(x.data_ptr(), R, N, N, order, N // 16, ALL, raw.data_ptr(), out.data_ptr(), N,
                                        torch.cuda.current_stream().cuda_stream))

    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        launch()                                               # the stream's first call is outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            launch()
    for _ in range(2):
        out.fill_(-1.0)
        raw.fill_(255)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want_out.tobytes() and raw.cpu().numpy().tobytes() == want_rec.tobytes()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _feature12(frames) -> np.ndarray:
    from amcpy_amd.features import features18
    return _cpu(features18(frames))[:, 11].astype(np.float64)


@pytest.mark.parametrize("mod,order,sps,pulse", host.E2E)
def test_generated_rows_are_recovered_within_the_caps(mod, order, sps, pulse):
    """64 rows at 20 dB with a drawn offset of up to 0.004 cycles per sample: EVERY estimate within 0.25 bin of the M-th-power
    grid of the drawn offset; on the rows whose offset is at least 2 cycles of x^4 per frame, feature 12 of the untouched rows
    is below 0.5 of the cfo = 0 rows' (same symbols, same noise) and that of the recovered rows within 5 % of it."""
    x = host.e2e_rows(mod, sps, pulse, host.E2E_CFO, compute=None)
    x0 = host.e2e_rows(mod, sps, pulse, 0.0, compute=None)
    f = host.drawn_offsets(sps)
    y, est = carrier.recover(x, order, search_bins_=host.E2E_N // 16)
    err_bins = np.abs(_cpu(est.cycles) - f) * order * host.E2E_N
    far = np.abs(f) * 4 * host.E2E_N >= 2.0
    f12_0, f12_raw, f12_rec = _feature12(x0), _feature12(x), _feature12(y)
    print(f"{mod} {sps} {pulse}: worst offset error {err_bins.max():.3f} bin; feature 12 untouched / clean at most "
          f"{(f12_raw[far] / f12_0[far]).max():.3f}; recovered within {np.abs(f12_rec[far] / f12_0[far] - 1).max():.2%}; "
          f"lowest quality {float(_cpu(est.quality).min()):.3f}")
    assert far.sum() >= host.E2E_ROWS // 2
    assert err_bins.max() <= 0.25
    assert np.all(f12_raw[far] < 0.5 * f12_0[far])
    assert np.all(np.abs(f12_rec[far] / f12_0[far] - 1.0) <= 0.05)


# ---- wiring -----------------------------------------------------------------------------------------------------------------------
def test_extract_sigmf_recover_brings_feature_12_back_and_none_changes_nothing(tmp_path):
    """One QPSK emitter half a scan bin (nfft = 1024) off the centre it is tuned to: 8 cycles per frame of 2048 after the
    decimation by 8.  Feature 12 against the same recording tuned to the emitter's true centre."""
    from amcpy_amd import sigmf
    S, N, D = 1 << 18, 2048, 8
    centre, off = 0.125, 0.5 / 1024
    x, _ = wf.scene([dict(mod="QPSK", sps=(2, 1), rate=(8, 1), center=centre + off)], S, noise_sigma=0.05, seed=36)
    stem = tmp_path / "one"
    _cpu(x).tofile(str(stem) + ".sigmf-data")
    (tmp_path / "one.sigmf-meta").write_text(json.dumps({
        "global": {"core:datatype": "cf32_le", "core:version": "1.0.0", "core:sample_rate": 1.0e6},
        "captures": [{"core:sample_start": 0, "core:frequency": 0.0}], "annotations": []}))
    tuned = dict(shift_hz=-centre * 1.0e6, decimate=D)
    exact = dict(shift_hz=-(centre + off) * 1.0e6, decimate=D)
    f_true, _ = sigmf.extract_sigmf(stem, N, tune=exact)
    f_raw, starts = sigmf.extract_sigmf(stem, N, tune=tuned)
    f_none, starts_none = sigmf.extract_sigmf(stem, N, tune=dict(tuned, recover=None))
    assert f_none.tobytes() == f_raw.tobytes() and starts_none.tobytes() == starts.tobytes()
    f_rec, starts_rec, found = sigmf.extract_sigmf(stem, N, tune=dict(tuned, recover=dict(order=4, search_hz=2000.0)))
    assert starts_rec.tobytes() == starts.tobytes() and f_rec.shape == f_raw.shape and f_rec.shape[0] >= 8
    keep = slice(None)                                                       # every frame: the filters emit whole windows only
    residual = off * D * (1.0e6 / D)                                         # Hz at the frames' rate
    print(f"carrier found {found['carrier_hz'][keep].min():.1f} ... {found['carrier_hz'][keep].max():.1f} Hz, planted {residual:.1f}; "
          f"feature 12 untouched / true at most {(f_raw[keep, 11] / f_true[keep, 11]).max():.3f}, recovered within "
          f"{np.abs(f_rec[keep, 11] / f_true[keep, 11] - 1).max():.2%}")
    assert np.all(np.abs(found["carrier_hz"][keep] - residual) <= 0.25 * (1.0e6 / D) / (4 * N))
    assert np.all(f_raw[keep, 11] < 0.5 * f_true[keep, 11])
    assert np.all(np.abs(f_rec[keep, 11] / f_true[keep, 11] - 1.0) <= 0.05)
    per_emitter = sigmf.extract_sigmf(stem, N, tune=dict(tuned, recover=dict(order=4, per="emitter")))[2]
    assert np.all(per_emitter["carrier_hz"] == per_emitter["carrier_hz"][0])


def test_dataset_and_occupied_features_take_recover_and_none_changes_nothing():
    torch = _torch()
    from amcpy_amd import occupancy
    from amcpy_amd.features import features18
    kw = dict(sps=(8, 1), cfo=0.003, seed=36)
    plain = wf.dataset_features(["QPSK"], [20.0], 6, 1024, **kw)["QPSK"]
    assert wf.dataset_features(["QPSK"], [20.0], 6, 1024, recover=None, **kw)["QPSK"].tobytes() == plain.tobytes()
    rec = wf.dataset_features(["QPSK"], [20.0], 6, 1024, recover=dict(order=4), **kw)["QPSK"]
    frames = wf.dataset(["QPSK"], [20.0], 6, 1024, **kw)["QPSK"].reshape(6, 1024)
    assert rec.reshape(6, 18).tobytes() == _cpu(features18(carrier.recover(frames, 4)[0])).tobytes()
    with pytest.raises(ValueError):
        wf.dataset_features(["QPSK"], [20.0], 6, 1024, recover=dict(order=4, per="emitter"), **kw)
    # occupied cells: 2 channels x 3 frames, the cells (0, 1), (1, 0), (1, 2) occupied
    cells = frames.reshape(2, 3, 1024).contiguous()
    power = occupancy.row_power(cells.view(6, 1024)).view(2, 3)
    mask = torch.tensor([[False, True, False], [True, False, True]], device="cuda")
    occ = occupancy.Occupancy(mask=mask, floor=torch.zeros(3, device="cuda"), rows=torch.tensor([1, 3, 5], dtype=torch.int32, device="cuda"),
                              snr_db=power)
    base = _cpu(occupancy.occupied_features(cells, occ))
    assert _cpu(occupancy.occupied_features(cells, occ, recover=None)).tobytes() == base.tobytes()
    got = _cpu(occupancy.occupied_features(cells, occ, recover=dict(order=4))).reshape(6, 18)
    want = _cpu(features18(carrier.recover(cells.view(6, 1024)[[1, 3, 5]].contiguous(), 4)[0]))
    assert got[[1, 3, 5]].tobytes() == want.tobytes() and np.isnan(got[[0, 2, 4]]).all()
    one = _cpu(occupancy.occupied_features(cells, occ, recover=dict(order=4, per="emitter"))).reshape(6, 18)
    assert one[1].tobytes() == got[1].tobytes() and np.isfinite(one[[3, 5]]).all()      # channel 0 has one cell: its own estimate
