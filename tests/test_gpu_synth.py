"""The waveform generator (include/amcx.h, amcx_synth_c64; ABI 16.2) on the GPU.

THE REFERENCE is tests/synth_ref.py: every integer of the contract exact, s, v, z and out in float64, and the criterion derived
there -- (P + 8) 2^-24 S + B 2^-24 sigma sqrt(-ln u) + 2^-24 |out64| per output.  What the contract fixes by integers alone is
compared with ==: the symbols against the table, the pulse against the existing resampler run on the numpy-drawn symbols, and
everything the contract calls position independent as bytes.  Each test prints the worst ratio it saw."""
import numpy as np
import pytest

from amcpy_amd import _lib, resample as rs, waveform as wf
from tests import synth_ref as ref
from tests.test_synth_host import N_NOISE, N_SYMBOLS, ORDERS, SEED, histogram_ok, noise_statistics_ok

pytestmark = pytest.mark.gpu

ODD_STEP = 0x9E3779B97F4A7C15
# (seed, row, sample) found once by a numpy search over the noise words of row 0 (tests/synth_ref.words): the first sample
# whose w1 >> 8 is 0xFFFFFF (u = 1) and the first whose w1 >> 8 is 0 (u = 2^-24, the smallest)
U_ONE = (2028, 0, 1594399)
U_MIN = (2028, 0, 8497440)


def _torch():
    import torch
    return torch


def _gen(*a, **kw):
    y = wf.generate(*a, **kw)
    _torch().cuda.synchronize()
    return y.cpu().numpy()


def _taps(T, seed=0):
    """T taps from +-[0.5, 1]: every tap counts"""
    rng = np.random.default_rng(2000 + T + seed)
    return (rng.uniform(0.5, 1.0, T) * rng.choice([-1.0, 1.0], T)).astype(np.float32)


def _table(order):
    rng = np.random.default_rng(order)
    return (rng.uniform(0.5, 1.0, order) * np.exp(2j * np.pi * rng.uniform(0, 1, order))).astype(np.complex64)


@pytest.mark.parametrize("order", [2, 3, 64, 256])
def test_symbols_are_the_table_at_the_drawn_index(order):
    R, S, row0, n0 = 4, 1031, (1 << 32) + 5, 3
    table = _table(order)
    y = _gen(table, R, S, sps=(1, 1), taps=np.ones(1, np.float32), seed=SEED, row_index0=row0, sample_index0=n0,
             random_phase=False, random_timing=False)
    assert y.shape == (R, S) and y.dtype == np.complex64
    for f in range(R):
        idx = ref.symbol_indices(SEED, row0 + f, np.arange(n0, n0 + S), order)
        assert y[f].tobytes() == table[idx].tobytes(), (order, f)
    assert not np.array_equal(y[0], y[1])


# (8, 3, 3) and (8, 1, 5): T < U, phases with no tap (syn_pulse with cnt == 0)
PULSES = [(1, 1, 1), (8, 1, 8), (2, 1, 33), (8, 3, 129), (256, 255, 4096), (3, 4096, 7), (8, 3, 3), (8, 1, 5)]


@pytest.mark.parametrize("random_timing", [False, True])
@pytest.mark.parametrize("U,V,T", PULSES)
def test_pulse_equals_the_resampler_on_the_drawn_symbols(U, V, T, random_timing):
    """sigma = 0, no carrier: a row is amcx_resample with L = U, D = V, tau0 = (n0 V + tau_r) mod U over the symbols from
    floor((n0 V + tau_r) / U) on -- more than one tile of it, from an odd first sample."""
    torch = _torch()
    tile, _, _ = _lib.synth_plan(16, T, U, V)
    R, S, n0, row0 = 2, tile + max(3, min(tile // 2, 37)), 12345, 77
    table, taps = wf.constellation_table("16QAM"), _taps(T)
    y = _gen(table, R, S, sps=(U, V), taps=taps, seed=SEED, row_index0=row0, sample_index0=n0, random_phase=False,
             random_timing=random_timing, timing=U - 1)
    P = -(-T // U)
    taus = set()
    for f in range(R):
        tau = ref.row_params(SEED, row0 + f, U, flags=ref.RANDOM_TIMING if random_timing else 0, tau0=U - 1)[2]
        taus.add(tau)
        s0, tau0 = divmod(n0 * V + tau, U)
        n_sym = (P - 1) + ((S - 1) * V + tau0) // U + 1
        a = ref.symbols(SEED, row0 + f, np.arange(s0, s0 + n_sym), table).astype(np.complex64)
        want = rs.resample(torch.from_numpy(a).cuda(), taps, U, V, phase_index0=tau0)
        torch.cuda.synchronize()
        assert want.shape[0] >= S
        assert y[f].tobytes() == want[:S].cpu().numpy().tobytes(), (U, V, T, f, tau)
    assert random_timing or taus == {U - 1}


def _check(y, seed, row0, n0, table, taps, U, V, sigmas, fpg=1, **kw):
    worst = 0.0
    for f in range(y.shape[0]):
        r = ref.generate(seed, row0 + f, n0, y.shape[1], table, taps, U, V, float(sigmas[f // fpg]), **kw)
        worst = max(worst, ref.worst_ratio(y[f], r))
    return worst


@pytest.mark.parametrize("mod,U,V,T", [("16QAM", 8, 3, 129), ("QPSK", 2, 1, 33), ("WGN", 1, 1, 1), ("8PSK", 5, 7, 23),
                                         ("QPSK", 8, 3, 5)])                # the last: T < U
def test_carrier_and_noise_meet_the_criterion(mod, U, V, T):
    R, S, n0, row0 = 3, 1500, (1 << 39) + 1, (1 << 63) + 11
    table, taps = wf.constellation_table(mod), _taps(T)
    sig = np.array([0.3, 2.0, 0.0], np.float32)
    cfo = 0.01
    y = _gen(mod, R, S, sps=(U, V), taps=taps, sigma=sig, seed=SEED, row_index0=row0, sample_index0=n0, cfo=cfo,
             shift=wf.Fraction(ODD_STEP, 1 << 64))
    worst = _check(y, SEED, row0, n0, table if len(table) else None, taps, U, V, sig, phase_step=ODD_STEP, cfo_max=wf.cfo_max_of(cfo))
    print(f"synth {mod} U={U} V={V} T={T}: worst |err| / bound = {worst:.4f}")
    assert worst <= 1.0
    assert np.isfinite(y.view(np.float32)).all() and np.abs(y[:2]).max() > 0.1


def _resampler_row(seed, r, n0, S, table, taps, U, V, tau):
    """Samples n0 ... n0 + S - 1 of row r without carrier and noise, as the resampler makes them from the numpy-drawn symbols"""
    torch = _torch()
    P = -(-len(taps) // U)
    s0, tau0 = divmod(n0 * V + tau, U)
    n_sym = (P - 1) + ((S - 1) * V + tau0) // U + 1
    a = ref.symbols(seed, r, np.arange(s0, s0 + n_sym), table).astype(np.complex64)
    want = rs.resample(torch.from_numpy(a).cuda(), taps, U, V, phase_index0=tau0)
    torch.cuda.synchronize()
    assert want.shape[0] >= S
    return want[:S].cpu().numpy()


@pytest.mark.parametrize("U,tile", [(1, 1), (2, 2)])
def test_tiles_of_one_and_two_samples(U, tile):
    """(U, 4096, 4096) plans a tile of U samples: at one sample the pair's lone member is A where the absolute index is even
    and B where it is odd.  Rows of 5 samples from an even and an odd first sample: against the resampler by bytes at
    sigma = 0, against the reference by the criterion with carrier and noise."""
    V, T = 4096, 4096
    table, taps = wf.constellation_table("QPSK"), _taps(T)
    assert _lib.synth_plan(len(table), T, U, V)[0] == tile
    R, S, row0 = 2, 5, (1 << 32) - 1
    sig = np.array([0.0, 0.7], np.float32)
    worst = 0.0
    for n0 in (6, 7):
        y = _gen(table, R, S, sps=(U, V), taps=taps, seed=SEED, row_index0=row0, sample_index0=n0, random_phase=False)
        for f in range(R):
            tau = ref.row_params(SEED, row0 + f, U, flags=ref.RANDOM_TIMING)[2]
            assert y[f].tobytes() == _resampler_row(SEED, row0 + f, n0, S, table, taps, U, V, tau).tobytes(), (U, n0, f)
        y = _gen(table, R, S, sps=(U, V), taps=taps, sigma=sig, seed=SEED, row_index0=row0, sample_index0=n0, cfo=0.01,
                 shift=wf.Fraction(ODD_STEP, 1 << 64))
        worst = max(worst, _check(y, SEED, row0, n0, table, taps, U, V, sig, phase_step=ODD_STEP, cfo_max=wf.cfo_max_of(0.01)))
        assert np.abs(y).min() > 0
    print(f"synth tile of {tile}: worst |err| / bound = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mod,U,V,T,per_row", [("16QAM", 3, 4096, 7, 3), ("QPSK", 8, 1, 8, 1)])
def test_every_row_over_three_trips_of_the_grid(mod, U, V, T, per_row):
    """At least 2 grid + 1 (row, tile) items, the grid as the plan reports it: some workgroup goes round its item loop three times,
    re-deriving W, phase0, step, tau and sigma, and drawing the next item's symbols over what the last one's sums read.
    (3, 4096, 7): tiles of 4 samples, rows of 2 tiles + 3, 4 workgroups per CU; the 8 / 1 rectangle: rows of one item, 8 per
    CU.  Rows straddle 2^32, the first sample is odd, sigma is per group of 3 rows and mixes 0 with non-zero values.  EVERY
    row meets the criterion, and the rows equal, as bytes, the same rows made in calls of 15 (one trip each)."""
    torch = _torch()
    table, taps = wf.constellation_table(mod), (_taps(T) if per_row > 1 else wf.design_rect(U))
    tile, _, grid = _lib.synth_plan(len(table), T, U, V)
    S = 2 * tile + 3 if per_row == 3 else 64
    assert -(-S // tile) == per_row
    R = -(-(2 * grid + 1) // per_row) + (2 if per_row > 1 else 4)
    items = R * per_row
    print(f"synth {mod} U={U} V={V} T={T}: {R} rows of {S} = {items} items of {tile} samples over {grid} workgroups")
    assert items >= 2 * grid + 1
    fpg, n0, row0, cfo = 3, 12345, (1 << 32) - R // 2, 0.01
    sig = np.random.default_rng(U).choice(np.array([0.0, 0.0, 0.3, 1.0, 2.0], np.float32), -(-R // fpg))
    assert (sig == 0).any() and (sig != 0).any()
    dev = dict(taps=torch.from_numpy(taps).cuda(), sigma=torch.from_numpy(sig).cuda())
    table_dev = torch.from_numpy(table).cuda()
    kw = dict(sps=(U, V), seed=SEED, sample_index0=n0, cfo=cfo, shift=wf.Fraction(ODD_STEP, 1 << 64), frames_per_group=fpg)
    y = _gen(table_dev, R, S, row_index0=row0, **dev, **kw)
    assert y.shape == (R, S)
    worst = 0.0
    for f in range(R):
        r = ref.generate(SEED, row0 + f, n0, S, table, taps, U, V, float(sig[f // fpg]), phase_step=ODD_STEP,
                         cfo_max=wf.cfo_max_of(cfo))
        ratio = ref.worst_ratio(y[f], r)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (f, ratio)
    print(f"synth {mod} U={U} V={V} T={T} over three trips: worst |err| / bound = {worst:.4f}")
    parts = [wf.generate(table_dev, min(15, R - a), S, row_index0=row0 + a, taps=dev["taps"],
                         sigma=dev["sigma"][a // fpg:(a + 14) // fpg + 1], **kw) for a in range(0, R, 15)]
    torch.cuda.synchronize()
    assert y.tobytes() == torch.cat(parts).cpu().numpy().tobytes()


def test_integer_determined_special_cases_are_exact():
    taps, table = wf.design_rrc(2, 4), wf.constellation_table("QPSK")
    # phase0 = 0 with step = 0: the mixer's product is skipped, and without noise out IS s -- a second call with a carrier
    # whose phase is a multiple of 2^32 below 2^32 ... i.e. none -- equals it, and a drawn phase does not
    plain = _gen("QPSK", 2, 300, sps=(2, 1), taps=taps, seed=5, random_phase=False)
    again = _gen("QPSK", 2, 300, sps=(2, 1), taps=taps, seed=5, random_phase=False, shift=wf.Fraction(1, 1 << 64))
    assert plain.tobytes() == again.tobytes()                   # phi = n < 2^32: still skipped
    for f in range(2):
        r = ref.generate(5, f, 0, 300, table, taps, 2, 1, 0.0, flags=ref.RANDOM_TIMING)
        assert (r["phi"] == 0).all() and ref.worst_ratio(plain[f], r) <= 1.0
    assert plain.tobytes() != _gen("QPSK", 2, 300, sps=(2, 1), taps=taps, seed=5).tobytes()
    # the noise class without noise is zero (s is +0 + 0j; the mixer may turn a zero's sign)
    zero = _gen("WGN", 2, 100, seed=5, cfo=0.01)
    assert not zero.any()
    # u = 1: z = 0 whatever sigma; the smallest u: |z| = sigma sqrt(24 ln 2), within the criterion
    for (seed, row, n), want_u in ((U_ONE, 1.0), (U_MIN, 2.0 ** -24)):
        y = _gen("WGN", 1, 3, sigma=3.0, seed=seed, row_index0=row, sample_index0=n - 1)
        r = ref.generate(seed, row, n - 1, 3, None, np.ones(1, np.float32), 8, 1, 3.0)
        assert r["u"][1] == want_u and ref.worst_ratio(y[0], r) <= 1.0
        if want_u == 1.0:
            assert y[0, 1] == 0 and y[0, 0] != 0 and y[0, 2] != 0
        else:
            assert abs(abs(complex(y[0, 1])) - 3.0 * np.sqrt(24 * np.log(2.0))) < 1e-4
    # sigma = 0 keeps the signed zeros of v: a table of -0 - 0j through a one-tap pulse of 1
    neg = np.array([complex(-0.0, -0.0)], np.complex64)
    y = _gen(neg, 1, 64, sps=(1, 1), taps=np.ones(1, np.float32), random_phase=False, random_timing=False)
    assert np.signbit(y.view(np.float32)).all()


def test_rows_cut_into_calls_equal_one_call():
    taps, sig = _taps(129), np.array([0.5, 0.0, 1.0, 0.25, 0.125], np.float32)
    kw = dict(sps=(8, 3), taps=taps, seed=11, cfo=0.02, sample_index0=9)
    whole = _gen("64QAM", 5, 700, sigma=sig, row_index0=(1 << 32) - 2, **kw)
    parts = [_gen("64QAM", n, 700, sigma=sig[a:a + n], row_index0=(1 << 32) - 2 + a, **kw) for a, n in ((0, 1), (1, 3), (4, 1))]
    assert whole.tobytes() == np.concatenate(parts).tobytes()


def test_a_stream_cut_into_chunks_equals_one_call():
    """10 007 samples against chunks of 1, 2, 255, 256, 257 and the remainder (odd first samples among them), through
    generate and through Stream.push."""
    taps = _taps(129)
    kw = dict(sps=(8, 3), taps=taps, snr_db=3.0, seed=12, cfo=0.02)
    whole = _gen("16QAM", 1, 10_007, row_index0=6, **kw)[0]
    cuts = [1, 2, 255, 256, 257]
    cuts.append(10_007 - sum(cuts))
    at, parts = 0, []
    for n in cuts:
        parts.append(_gen("16QAM", 1, n, row_index0=6, sample_index0=at, **kw)[0])
        at += n
    assert whole.tobytes() == np.concatenate(parts).tobytes()
    s = wf.Stream("16QAM", row=6, **kw)
    pushed = [s.push(n) for n in (3, 0, 4096, 4097, 1, 10_007 - 8197)]
    _torch().cuda.synchronize()
    assert s.index == 10_007 and whole.tobytes() == np.concatenate([p.cpu().numpy() for p in pushed]).tobytes()
    # ... and more than one tile of a short pulse
    tile, _, _ = _lib.synth_plan(4, 8, 8, 1)
    kw = dict(sps=(8, 1), snr_db=10.0, seed=13)
    whole = _gen("QPSK", 1, 2 * tile + 5, **kw)[0]
    parts = [_gen("QPSK", 1, n, sample_index0=a, **kw)[0] for a, n in ((0, tile - 1), (tile - 1, 7), (tile + 6, tile - 1))]
    assert whole.tobytes() == np.concatenate(parts).tobytes()


def test_a_row_stride_on_8_bytes_shifts_no_bit():
    torch = _torch()
    kw = dict(sps=(2, 1), taps=wf.design_rrc(2, 8), snr_db=6.0, seed=14, cfo=0.01, sample_index0=1)
    want = _gen("QPSK", 4, 600, **kw)
    base = torch.zeros((4, 601), dtype=torch.complex64, device="cuda")          # rows 601 x 8 bytes apart: every other one off 16
    got = wf.generate("QPSK", 4, 600, out=base[:, :600], **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == base.data_ptr() and got.cpu().numpy().tobytes() == want.tobytes()
    assert (base[:, 600] == 0).all()
    shifted = torch.zeros(4 * 600 + 1, dtype=torch.complex64, device="cuda")     # the whole matrix 8 bytes off
    wf.generate("QPSK", 4, 600, out=shifted[1:].view(4, 600), **kw)
    torch.cuda.synchronize()
    assert shifted[1:].cpu().numpy().tobytes() == want.tobytes() and shifted[0] == 0


def test_a_resident_call_is_captured_whole_in_a_graph():
    """With the table, the taps, sigma and out on the device, generate is the launch alone: captured in a graph (where an
    upload from host memory or a synchronisation would end the capture with an error) and replayed, it gives the bits of the
    ordinary call.  Any one of the three left on the host is uploaded by the call: the same bits."""
    torch = _torch()
    taps = _taps(33)
    kw = dict(sps=(2, 1), seed=19, cfo=0.01, frames_per_group=2)
    want = _gen("QPSK", 3, 500, taps=taps, sigma=[0.5, 0.25], **kw)
    out = torch.zeros((3, 500), dtype=torch.complex64, device="cuda")
    table_dev, taps_dev = torch.from_numpy(wf.constellation_table("QPSK")).cuda(), torch.from_numpy(taps).cuda()
    sig_dev = torch.tensor([0.5, 0.25], dtype=torch.float32, device="cuda")

    def launch():
        return wf.generate(table_dev, 3, 500, taps=taps_dev, sigma=sig_dev, out=out, **kw)

    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        assert launch() is out                                 # the stream's first call is outside the capture
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes()
        with torch.cuda.graph(g, stream=s):
            launch()
    out.fill_(-1.0)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    mixed = wf.generate(table_dev, 3, 500, taps=taps, sigma=[0.5, 0.25], **kw)
    torch.cuda.synchronize()
    assert mixed.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(TypeError):
        wf.generate(table_dev, 3, 500, taps=taps_dev.double(), sigma=sig_dev, out=out, **kw)
    with pytest.raises(ValueError):                            # out wider than the row: a view of the columns is what to pass
        wf.generate(table_dev, 3, 499, taps=taps_dev, sigma=sig_dev, out=out, **kw)


def test_graph_replay():
    torch = _torch()
    kw = dict(sps=(8, 3), taps=torch.from_numpy(_taps(129)).cuda(), seed=15, cfo=0.01)
    want = _gen("16QAM", 3, 900, sigma=0.5, **kw)
    out = torch.zeros((3, 900), dtype=torch.complex64, device="cuda")
    table = torch.from_numpy(wf.constellation_table("16QAM")).cuda()
    sig = torch.full((1,), 0.5, dtype=torch.float32, device="cuda")
    lib = _lib.load()

    def launch():
        _lib.check(lib.amcx_synth_c64(15, 0, 0, 3, 900, 900, table.data_ptr(), 16, kw["taps"].data_ptr(), 129, 8, 3, 0, 0,
                                      wf.cfo_max_of(0.01), 3, sig.data_ptr(), 3, out.data_ptr(), torch.cuda.current_stream().cuda_stream))

    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        launch()                                               # the stream's first call is outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            launch()
    for _ in range(2):
        out.fill_(-1.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes()


def test_groups_take_their_own_sigma():
    taps = wf.design_rrc(2, 8)
    kw = dict(sps=(2, 1), taps=taps, seed=16, cfo=0.01)
    R, S = 7, 400
    clean = _gen("8PSK", R, S, **kw)
    table = wf.constellation_table("8PSK")
    for fpg, sig in ((1, [0.5, 0.0, 1.0, 0.25, 0.0, 2.0, 0.125]), (3, [0.5, 0.0, 1.0]), (R, [0.75])):
        sig = np.array(sig, np.float32)
        y = _gen("8PSK", R, S, sigma=sig, frames_per_group=fpg, **kw)
        worst = _check(y, 16, 0, 0, table, taps, 2, 1, sig, fpg, cfo_max=wf.cfo_max_of(0.01))
        print(f"synth groups of {fpg}: worst |err| / bound = {worst:.4f}")
        assert worst <= 1.0
        for f in range(R):
            quiet = sig[f // fpg] == 0
            assert (y[f].tobytes() == clean[f].tobytes()) == bool(quiet), (fpg, f)
    default = _gen("8PSK", R, S, sigma=[0.5, 0.0, 1.0], **kw)                    # groups of ceil(7 / 3) = 3 by default
    assert default.tobytes() == _gen("8PSK", R, S, sigma=[0.5, 0.0, 1.0], frames_per_group=3, **kw).tobytes()


def test_statistics_on_the_device():
    """The sizes and caps of tests/test_synth_host.py::test_reference_statistics, which the reference meets on its own: this
    catches a kernel that departs from it."""
    z = _gen("WGN", 1, N_NOISE, sigma=0.5, seed=SEED, row_index0=0)[0]
    noise_statistics_ok(z, 0.5)
    for order in ORDERS:
        table = np.arange(order).astype(np.complex64)
        y = _gen(table, 1, N_SYMBOLS, sps=(1, 1), taps=np.ones(1, np.float32), seed=SEED, row_index0=order, random_phase=False,
                 random_timing=False)[0]
        idx = y.real.astype(np.int64)
        assert np.array_equal(idx, ref.symbol_indices(SEED, order, np.arange(N_SYMBOLS), order)) and not y.imag.any()
        histogram_ok(idx, order)


def test_dataset_features_and_rows_on_the_device():
    mods, snrs = ["BPSK", "WGN"], [0.0, 10.0]
    kw = dict(sps=(2, 1), taps=wf.design_rrc(2, 8), seed=17, cfo=0.005)
    data = wf.dataset(mods, snrs, 5, 1024, **kw)
    _torch().cuda.synchronize()
    one = _gen("BPSK", 2, 1024, snr_db=10.0, row_index0=wf.dataset_row("BPSK", 10.0, 3), **kw)
    assert data["BPSK"].shape == (2, 5, 1024) and data["BPSK"][1, 3:5].cpu().numpy().tobytes() == one.tobytes()
    from amcpy_amd.features import features18
    feats = wf.dataset_features(mods, snrs, 5, 1024, chunk_frames=2, **kw)
    for m in mods:
        want = features18(data[m].reshape(10, 1024)).cpu().numpy().reshape(2, 5, 18)
        assert feats[m].shape == (2, 5, 18) and feats[m].dtype == np.float32 and feats[m].tobytes() == want.tobytes()
    power = float((data["BPSK"][1].abs() ** 2).mean())
    assert abs(power - 1.1) < 0.1                                # unit signal power and sigma^2 = 0.1


def test_scene_scan_tune_closes_the_loop(tmp_path):
    """Two emitters of known rate and place on a floor: the scan finds exactly those two, each centre within one bin, and
    the first, tuned to twice its bandwidth by its annotation, gives frames with finite features."""
    torch = _torch()
    from amcpy_amd import sigmf
    from amcpy_amd.features import features18
    nfft, S = 1024, 1 << 18
    emitters = [dict(mod="QPSK", sps=(2, 1), rate=(8, 1), center=-0.25), dict(mod="16QAM", sps=(8, 3), rate=(4, 1), center=0.1875)]
    x, anns = wf.scene(emitters, S, noise_sigma=0.1, seed=18)
    torch.cuda.synchronize()
    assert x.shape == (S,) and x.dtype == torch.complex64 and len(anns) == 2
    assert anns[0]["amcx:samples_per_symbol"] == 16.0 and abs(anns[1]["amcx:samples_per_symbol"] - 32 / 3) < 1e-12
    path = tmp_path / "scene.cf32"
    x.cpu().numpy().tofile(path)
    found = sigmf.scan_recording(sigmf.raw_recording(path, "cf32"), nfft=nfft, detect={})["emitters"]
    assert len(found) == 2, found
    centres = sorted(((e["freq_lower_edge"] + e["freq_upper_edge"]) / 2.0 + 0.5) % 1.0 - 0.5 for e in found)
    for got, em in zip(centres, emitters):
        assert abs(got - em["center"]) <= 1.0 / nfft, (got, em["center"])
    meta = {"global": {"core:sample_rate": 1.0}, "captures": [{"core:sample_start": 0, "core:frequency": 0.0}], "annotations": anns}
    shift_hz, (L, D) = sigmf.tune_from_annotation(meta, 0, oversample=2.0, rational=True)
    assert abs(shift_hz - 0.25) < 1e-12
    y = rs.resample(x, rs.design_resample_lowpass(L, D), L, D, shift=shift_hz)
    frames = y[:(y.shape[0] // 1024) * 1024].view(-1, 1024)
    f = features18(frames).cpu().numpy()
    assert frames.shape[0] >= 4 and np.isfinite(f).all()
