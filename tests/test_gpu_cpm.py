"""The continuous-phase generator (include/amcx.h, amcx_synth_cpm_c64; ABI 16.2.2) on the GPU.

THE REFERENCE is tests/cpm_ref.py: every integer of the contract in numpy, the mixer restated operation by operation -- without
noise the kernel is compared with it by ==, and the kernel itself in other cuts, segments and a graph replay as bytes.  The noise
is held per component to 2.5 x 2^-24 + 9 x 2^-24 sigma sqrt(-ln u) + 2^-24 |out| around the float64 evaluation at the exact
integer phase, the envelope to 2.5 sqrt(2) 2^-24 of 1.  Each bounded test prints the worst ratio it saw."""
from fractions import Fraction

import numpy as np
import pytest

from amcpy_amd import _lib, channel as ch, waveform as wf
from tests import cpm_ref as ref
from tests.plain_grids import LINE

pytestmark = pytest.mark.gpu

SEED = 0x5EED5EED1234ABCD
ROW0 = (1 << 33) + 7                       # beyond 2^32: the counter's fourth word counts
SENTINEL = np.complex64(-7.0 - 9.0j)
EPS = 2.0 ** -24


def _torch():
    import torch
    return torch


def _cpu(t):
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def _words(t):
    return _cpu(t).view(np.uint32)


def _odd_pulse():
    """seven taps at three samples per symbol, none of them round, and a phase_full that is not the last tap; two of them are
    the bits of signalling NaNs as floats: the taps reach LDS through the float tap routine, which must move bits and nothing else"""
    rng = np.random.default_rng(7)
    taps = np.concatenate([rng.integers(0, 1 << 32, 5, dtype=np.uint64), [0x7FA00001, 0xFFA00001]])
    return wf.CpmPulse(np.sort(taps).astype(np.uint32), 0xC0FFEE11)


#        order, U, V, the pulse (T = its taps)
SHAPES = {"msk_1": (2, 1, 1, lambda: wf.design_cpfsk(1)), "msk_8": (2, 8, 1, lambda: wf.design_cpfsk(8)),
          "fsk4_8_3": (4, 8, 3, lambda: wf.design_cpfsk(8, 1)), "gmsk_8": (2, 8, 1, lambda: wf.design_gmsk(8)),
          "gfsk8_256_255": (8, 256, 255, lambda: wf.design_gfsk(256, 1, 0.3, 16)), "odd_3_4096": (2, 3, 4096, _odd_pulse)}
TAPS = {"msk_1": 1, "msk_8": 8, "fsk4_8_3": 8, "gmsk_8": 32, "gfsk8_256_255": 4096, "odd_3_4096": 7}


def _acc_in(n0, V, U, order, rows):
    """A(K0) per row: the true prefix where K0 is small enough to draw in numpy, else words of no meaning -- the contract
    defines the output from acc_in whatever it holds"""
    K0 = n0 * V // U
    if n0 == 0:
        return None
    if K0 <= 1 << 16:
        return np.array([ref.prefix(SEED, r, K0, order) for r in rows], np.uint32)
    return np.array([(0x9E3779B9 * (i + 1) + n0) & ref.M32 for i in range(len(rows))], np.uint32)


@pytest.mark.parametrize("where", ["0", "1", "odd", "end"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_equals_the_restatement_bit_for_bit(name, where):
    """Three rows of two tiles and a sample with drawn phase, offset and timing, the stride wider than the rows, out on 8 but not
    16 bytes, rows beyond 2^32, the first sample at 0, 1, an odd one and as late as the entry takes; acc_in from numpy, acc_out
    equal to numpy's; the padding of out keeps its sentinel."""
    torch = _torch()
    order, U, V, make = SHAPES[name]
    pulse = make()
    T = len(pulse.phase_taps)
    assert T == TAPS[name]
    tile, lds, seg = _lib.synth_cpm_plan(T, U, V, 3, 1)
    R, count, pad = 3, 2 * tile + 1, 4
    n0 = {"0": 0, "1": 1, "odd": 12345, "end": (1 << 40) - count - 1}[where]
    rows = [ROW0 + f for f in range(R)]
    acc_in = _acc_in(n0, V, U, order, rows)
    flat = torch.full((R * (count + pad) + 1,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
    out = flat[1:].view(R, count + pad)[:, :count]
    assert out.data_ptr() % 16 == 8 and out.stride(0) == count + pad
    acc_out = torch.full((R,), -1, dtype=torch.int32, device="cuda")
    got = wf.generate(f"{order}FSK", R, count, sps=(U, V), taps=pulse, seed=SEED,
                      row_index0=ROW0, sample_index0=n0, cfo=0.01, shift=Fraction(1, 7), acc_in=acc_in, acc_out=acc_out, out=out)
    assert got is out
    y = _cpu(flat)[1:].reshape(R, count + pad)
    state = _words(acc_out)
    kw = dict(phase_step=wf._stream.phase_step_of(Fraction(1, 7)), cfo_max=wf.cfo_max_of(0.01))
    for f, r in enumerate(rows):
        want, a1 = ref.restate(SEED, r, n0, count, order, pulse.phase_taps, pulse.phase_full, U, V,
                               acc_in=0 if acc_in is None else int(acc_in[f]), **kw)
        assert np.array_equal(y[f, :count], want), (name, where, f, int(np.argmax(y[f, :count] != want)))
        assert int(state[f]) == a1, (name, where, f)
    assert (y[:, count:] == SENTINEL).all() and _cpu(flat)[0] == SENTINEL
    assert np.isfinite(y.view(np.float32)).all() and not np.array_equal(y[0, :count], y[1, :count])


def test_msk_at_one_sample_per_symbol_walks_the_exact_quarter_turns():
    """h = 1/2 moves the phase by exact quarter turns, where the mixer is exact: j to the running sum of the drawn symbols"""
    y = _cpu(wf.generate("MSK", 3, 1000, sps=(1, 1), seed=SEED, row_index0=ROW0, random_phase=False, random_timing=False))
    pulse = wf.cpm_pulse("MSK", 1)
    assert list(pulse.phase_taps) == [1 << 30] and pulse.phase_full == 1 << 30
    turns = np.array([1, 1j, -1, -1j], np.complex64)
    for f in range(3):
        a = ref.alphas(SEED, ROW0 + f, np.arange(1000), 2)
        assert set(np.unique(a)) == {-1, 1}
        want = turns[np.cumsum(a) & 3]
        assert np.array_equal(y[f], want), (f, int(np.argmax(y[f] != want)))


@pytest.mark.parametrize("name", ["fsk4_8_3", "odd_3_4096", "gmsk_8"])
def test_segments_change_no_bit(name):
    """One row of three tiles and a sample in 1, 2, 3 and 64 (clamped to its four tiles) segments, and in the plan's: the same
    bytes, the same acc_out, == the restatement.  odd_3_4096 has V / U beyond the window: symbols between two tiles' spans,
    which a workgroup that walks several tiles sweeps."""
    torch = _torch()
    order, U, V, make = SHAPES[name]
    pulse = make()
    tile = _lib.synth_cpm_plan(len(pulse.phase_taps), U, V, 1, 1)[0]
    count = 3 * tile + 1
    want, a1 = ref.restate(SEED, ROW0, 0, count, order, pulse.phase_taps, pulse.phase_full, U, V, cfo_max=wf.cfo_max_of(0.003))
    for segments in (1, 2, 3, 64, 0):
        acc_out = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        y = _cpu(wf.generate(f"{order}FSK", 1, count, sps=(U, V), taps=pulse, seed=SEED, row_index0=ROW0, cfo=0.003, acc_out=acc_out,
                             segments=segments))[0]
        assert np.array_equal(y, want) and y.tobytes() == want.tobytes(), (name, segments, int(np.argmax(y != want)))
        assert int(_words(acc_out)[0]) == a1, (name, segments)
    assert _lib.synth_cpm_plan(len(pulse.phase_taps), U, V, 1, count)[2] == 4


def test_many_short_rows_and_the_plans_one_segment():
    """4096 rows of 64 samples fill the device on their own (one segment each): == the restatement on rows from both ends and the
    middle, with their acc_out; the same bytes as the call that asks for one segment"""
    torch = _torch()
    pulse = wf.design_gmsk(8)
    R, count = 4096, 64
    assert _lib.synth_cpm_plan(32, 8, 1, R, count)[2] == 1
    acc_out = torch.full((R,), -1, dtype=torch.int32, device="cuda")
    y = _cpu(wf.generate("GMSK", R, count, seed=SEED, row_index0=ROW0, acc_out=acc_out))
    state = _words(acc_out)
    for f in (0, 1, 2047, 4095):
        want, a1 = ref.restate(SEED, ROW0 + f, 0, count, 2, pulse.phase_taps, pulse.phase_full, 8, 1)
        assert np.array_equal(y[f], want) and int(state[f]) == a1, f
    assert _cpu(wf.generate("GMSK", R, count, seed=SEED, row_index0=ROW0, segments=1)).tobytes() == y.tobytes()


def test_rows_over_three_lines_of_the_grid():
    """2 LINE + 1 rows of one segment: the launch is folded into three lines, the last with one live workgroup, so the
    `blockIdx.y` term, the whole-workgroup return and `f * row_stride`, `acc_out[f]` at f >= 2^16 are executed.  The seam rows and
    2048 seeded ones == the restatement, samples and acc_out (a cap on the reference's time, about 0.6 ms a row); EVERY row the
    bytes of three calls of at most LINE rows -- single-line grids -- with row_index0 advanced.

    Then 32 769 rows of four tiles in four segments, 131 076 items: item = 4 f + segment, so the lines change between rows
    16 383 and 16 384 and inside the last row's line alone stand its four segments.  Every row the bytes of the call with one
    segment, samples and acc_out.  The restatement of such a row costs about 5 ms, a quarter of the rows 40 s: so the rows
    beside the two seams, the first, the last, and those with f = 0 mod 4 among 1024 seeded ones go to it (about 260 rows)."""
    torch = _torch()
    pulse = wf.design_cpfsk(1)
    T, U, V, order, count = len(pulse.phase_taps), 1, 1, 2, 2
    R = 2 * LINE + 1
    tile, _, seg = _lib.synth_cpm_plan(T, U, V, R, count)
    assert seg == 1
    items = R * seg
    print(f"cpm: {items} items, LINE = {LINE}")
    assert items >= 2 * LINE + 1
    kw = dict(sps=(U, V), taps=pulse, seed=SEED, cfo=0.01)
    buf = torch.full((R + 2, count + 3), complex(SENTINEL), dtype=torch.complex64, device="cuda")
    acc = torch.full((R + 2,), -1, dtype=torch.int32, device="cuda")
    got = wf.generate("MSK", R, count, row_index0=ROW0, acc_out=acc[:R], out=buf[:R, :count], segments=1, **kw)
    assert got.data_ptr() == buf.data_ptr() and got.stride(0) == count + 3
    y, state = _cpu(buf), _words(acc)
    assert (y[:R, count:] == SENTINEL).all() and (y[R:] == SENTINEL).all() and (state[R:] == 0xFFFFFFFF).all()
    y = np.ascontiguousarray(y[:R, :count])
    seams = [0, 1, LINE - 1, LINE, LINE + 1, 2 * LINE - 1, 2 * LINE]
    for f in np.union1d(seams, np.random.default_rng(37).choice(R, 2048, replace=False)):
        want, a1 = ref.restate(SEED, ROW0 + int(f), 0, count, order, pulse.phase_taps, pulse.phase_full, U, V, cfo_max=wf.cfo_max_of(0.01))
        assert y[f].tobytes() == want.tobytes() and int(state[f]) == a1, int(f)
    parts, states, at = [], [], 0
    for rows in (LINE, LINE, 1):
        a = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        parts.append(_cpu(wf.generate("MSK", rows, count, row_index0=ROW0 + at, acc_out=a, segments=1, **kw)))
        states.append(_words(a))
        at += rows
    assert np.concatenate(parts).tobytes() == y.tobytes() and np.concatenate(states).tobytes() == state[:R].tobytes()
    del buf, acc, got

    # rows of four segments across the seams
    R4, segments = LINE // 2 + 1, 4
    count4 = 3 * tile + 1
    # the launch's own count (cpm_plan of amcx.hip, restated): the asked segments, at most the row's tiles, recounted from their length
    tiles_per_row = -(-count4 // tile)
    tiles_per_seg = -(-tiles_per_row // min(segments, tiles_per_row))
    launched = -(-tiles_per_row // tiles_per_seg)
    assert (tiles_per_row, tiles_per_seg, launched) == (4, 1, segments)
    items = R4 * launched
    print(f"cpm: {items} items in {segments} segments a row, LINE = {LINE}")
    assert items >= 2 * LINE + 1
    a4 = torch.full((R4,), -1, dtype=torch.int32, device="cuda")
    a1 = torch.full((R4,), -1, dtype=torch.int32, device="cuda")
    y4 = y1 = None
    try:
        y4 = wf.generate("MSK", R4, count4, row_index0=ROW0, acc_out=a4, segments=segments, **kw)
        y1 = wf.generate("MSK", R4, count4, row_index0=ROW0, acc_out=a1, segments=1, **kw)
        words = lambda t: torch.view_as_real(t).view(torch.int32)             # noqa: E731
        assert torch.equal(words(y4), words(y1)) and torch.equal(a4, a1)
        seeded = np.random.default_rng(41).choice(R4, 1024, replace=False)
        rows = np.union1d([0, LINE // 4 - 1, LINE // 4, LINE // 4 + 1, R4 - 2, R4 - 1], seeded[seeded % 4 == 0])
        some, state = _cpu(y4[torch.from_numpy(rows).cuda()]), _words(a4)
        for i, f in enumerate(rows):
            want, acc1 = ref.restate(SEED, ROW0 + int(f), 0, count4, order, pulse.phase_taps, pulse.phase_full, U, V,
                                     cfo_max=wf.cfo_max_of(0.01))
            assert some[i].tobytes() == want.tobytes() and int(state[f]) == acc1, int(f)
        print(f"cpm: {rows.size} rows of {count4} samples against the restatement")
    finally:
        del y4, y1
        torch.cuda.empty_cache()


def test_rows_and_samples_cut_into_calls_equal_one_call():
    torch = _torch()
    kw = dict(sps=(8, 3), seed=SEED, cfo=0.01, snr_db=5.0)
    whole = _cpu(wf.generate("4FSK", 5, 3000, row_index0=ROW0, **kw))
    rows = np.concatenate([_cpu(wf.generate("4FSK", 2, 3000, row_index0=ROW0, **kw)), _cpu(wf.generate("4FSK", 3, 3000, row_index0=ROW0 + 2, **kw))])
    assert rows.tobytes() == whole.tobytes()
    for cut in (1, 1501, 2999):
        acc = torch.zeros(5, dtype=torch.int32, device="cuda")
        left = _cpu(wf.generate("4FSK", 5, cut, row_index0=ROW0, acc_out=acc, **kw))
        right = _cpu(wf.generate("4FSK", 5, 3000 - cut, row_index0=ROW0, sample_index0=cut, acc_in=acc, **kw))
        assert np.concatenate([left, right], axis=1).tobytes() == whole.tobytes(), cut
    with pytest.raises(ValueError):
        wf.generate("4FSK", 5, 10, sample_index0=4, **kw)


def test_a_stream_cut_into_chunks_equals_one_call():
    """chunks of 1, 2, 255, 256, 257 samples, in turn, over 10 007 samples: the stream swaps its two words of state per push"""
    n = 10007
    kw = dict(sps=(8, 1), seed=SEED, cfo=0.002, snr_db=10.0)
    whole = _cpu(wf.generate("GMSK", 1, n, row_index0=9, **kw))[0]
    stream = wf.Stream("GMSK", row=9, **kw)
    sizes, parts, at = (1, 2, 255, 256, 257), [], 0
    while at < n:
        take = min(sizes[len(parts) % len(sizes)], n - at)
        parts.append(_cpu(stream.push(take)))
        at += take
    assert stream.index == n and np.concatenate(parts).tobytes() == whole.tobytes()


def test_graph_replay():
    torch = _torch()
    pulse = wf.design_gmsk(8)
    taps = torch.from_numpy(pulse.phase_taps.view(np.int32)).cuda()
    sig = torch.full((1,), 0.5, dtype=torch.float32, device="cuda")
    acc_in = torch.from_numpy(np.array([ref.prefix(SEED, f, 5 * 3 // 8, 2) for f in range(3)], np.uint32).view(np.int32)).cuda()
    want_acc = torch.zeros(3, dtype=torch.int32, device="cuda")
    want = _cpu(wf.generate("GMSK", 3, 9000, sps=(8, 3), taps=wf.CpmPulse(taps, pulse.phase_full), sigma=sig, seed=SEED, sample_index0=5, cfo=0.01,
                            acc_in=acc_in, acc_out=want_acc))
    out = torch.zeros((3, 9000), dtype=torch.complex64, device="cuda")
    acc_out = torch.zeros(3, dtype=torch.int32, device="cuda")
    lib = _lib.load()

    def launch():
        _lib.check(lib.amcx_synth_cpm_c64(SEED, 0, 5, 3, 9000, 9000, 2, taps.data_ptr(), 32, pulse.phase_full, 8, 3, 0, 0, wf.cfo_max_of(0.01), 3,
                                          sig.data_ptr(), 3, acc_in.data_ptr(), acc_out.data_ptr(), 0, out.data_ptr(),
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
        acc_out.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes() and acc_out.cpu().numpy().tobytes() == want_acc.cpu().numpy().tobytes()


@pytest.mark.parametrize("mod,U,V", [("GMSK", 8, 1), ("4FSK", 8, 3)])
def test_noise_meets_the_derived_bound(mod, U, V):
    """per component within 2.5 x 2^-24 + 9 x 2^-24 sigma sqrt(-ln u) + 2^-24 |out| of the float64 evaluation at the exact integer
    phase, at three sigmas, with a carrier; a row without noise is the restatement"""
    sig = np.array([0.0, 0.5, 2.0], np.float32)
    pulse = wf.cpm_pulse(mod, U)
    order = wf.cpm_order(mod)
    y = _cpu(wf.generate(mod, 3, 6000, sps=(U, V), sigma=sig, seed=SEED, row_index0=ROW0, cfo=0.01))
    worst = 0.0
    for f in range(3):
        r64 = ref.generate64(SEED, ROW0 + f, 0, 6000, order, pulse.phase_taps, pulse.phase_full, U, V, float(sig[f]), cfo_max=wf.cfo_max_of(0.01))
        worst = max(worst, ref.worst_component_ratio(y[f], r64))
    want0, _ = ref.restate(SEED, ROW0, 0, 6000, order, pulse.phase_taps, pulse.phase_full, U, V, cfo_max=wf.cfo_max_of(0.01))
    print(f"cpm noise {mod} {U}/{V}: worst |err| / bound per component = {worst:.4f}")
    assert np.array_equal(y[0], want0)
    assert worst <= 1.0


@pytest.mark.parametrize("mod", ["GMSK", "8FSK"])
def test_constant_envelope(mod):
    """without noise ||out| - 1| <= 2.5 sqrt(2) 2^-24 at every sample: the mixer's per-component bound on a unit sample"""
    y = _cpu(wf.generate(mod, 2, 20000, sps=(8, 3), seed=SEED, row_index0=ROW0, cfo=0.01)).astype(np.complex128)
    worst = float(np.abs(np.abs(y) - 1.0).max()) / (2.5 * np.sqrt(2.0) * EPS)
    print(f"cpm envelope {mod}: worst ||out| - 1| / bound = {worst:.4f}")
    assert worst <= 1.0


# ---- through the chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fade", [None, "rayleigh"])
def test_dataset_features_of_continuous_and_linear_names(fade):
    """finite, reproducible, and the GMSK rows are not the BPSK rows; the same through a fading channel, which is a launch of
    its own behind the generator's and takes a continuous-phase row as it takes any other"""
    kw = {} if fade is None else dict(channel=dict(profile=ch.rayleigh(), doppler=1e-3))
    a = wf.dataset_features(["GMSK", "4FSK", "BPSK"], [10], 64, 2048, sps=(8, 1), **kw)
    b = wf.dataset_features(["GMSK", "4FSK", "BPSK"], [10], 64, 2048, sps=(8, 1), **kw)
    for m in ("GMSK", "4FSK", "BPSK"):
        assert a[m].shape == (1, 64, 18) and np.isfinite(a[m]).all() and a[m].tobytes() == b[m].tobytes(), m
    assert not np.array_equal(a["GMSK"], a["BPSK"]) and not np.array_equal(a["GMSK"], a["4FSK"])
    if fade is None:                                             # a constant envelope: the amplitude's spread is the noise's alone
        iq = wf.dataset(["GMSK", "BPSK"], [40], 4, 2048, sps=(8, 1), taps={"GMSK": None, "BPSK": wf.design_rrc(8)})
        env = {m: float(np.abs(_cpu(iq[m])).std()) for m in iq}
        assert env["GMSK"] < 0.02 < env["BPSK"], env


def test_scene_with_a_gmsk_emitter_is_found_by_the_scan(tmp_path):
    """one GMSK emitter of known rate and place on a floor: the scan finds exactly it, its centre within one bin"""
    torch = _torch()
    from amcpy_amd import sigmf
    nfft, S = 1024, 1 << 18
    emitters = [dict(mod="GMSK", sps=(4, 1), rate=(4, 1), center=0.1875)]
    x, anns = wf.scene(emitters, S, noise_sigma=0.1, seed=18)
    torch.cuda.synchronize()
    assert x.shape == (S,) and x.dtype == torch.complex64 and len(anns) == 1
    assert anns[0]["amcx:samples_per_symbol"] == 16.0 and anns[0]["core:label"] == "GMSK"
    path = tmp_path / "scene.cf32"
    x.cpu().numpy().tofile(path)
    found = sigmf.scan_recording(sigmf.raw_recording(path, "cf32"), nfft=nfft, detect={})["emitters"]
    assert len(found) == 1, found
    centre = ((found[0]["freq_lower_edge"] + found[0]["freq_upper_edge"]) / 2.0 + 0.5) % 1.0 - 0.5
    assert abs(centre - 0.1875) <= 1.0 / nfft, centre
