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
@pytest.mark.parametrize("N", [64, 128, 512, 4096])
def test_records_and_rows_equal_the_restatement(N, order):
    """3 + 3, 3 + 4, 3 + 3 + 3 and 4 + 4 + 4 passes; 64, 32, 8 and 1 rows per workgroup; one row, and three workgroups the last
    with one live slot; four search ranges; rows at a stride of N + 3 in and out, out's padding untouched."""
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
@pytest.mark.parametrize("N", [64, 128, 512, 4096])
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


@pytest.mark.parametrize("N", [64, 1024, 4096])
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
