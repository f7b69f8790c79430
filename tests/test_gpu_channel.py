"""The fading multipath channel (include/amcx.h, amcx_channel_c64; ABI 16.2.1) on the GPU.

THE REFERENCE is tests/channel_ref.py: the contract restated in numpy operation by operation -- without noise the kernel is
compared with it by ==.  The generator, the down-converter and the kernel itself in other cuts are compared as bytes of values;
the noise is held to the generator's derived bound and the gains to the float64 closed form within the bound derived there.
Each bounded test prints the worst ratio it saw."""
import numpy as np
import pytest

from amcpy_amd import _lib, channel as ch, ddc, waveform as wf
from tests import channel_ref as ref
from tests.plain_grids import LINE

pytestmark = pytest.mark.gpu

SEED = 0x5EED5EED1234ABCD
ROW0 = (1 << 33) + 7                       # beyond 2^32: the counter's fourth word counts
SENTINEL = np.complex64(-7.0 - 9.0j)


def _torch():
    import torch
    return torch


def _cpu(t):
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def _signal(R, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, n)) + 1j * rng.standard_normal((R, n))).astype(np.complex64)


def _profile(L, H, seed):
    """L paths with every field in use: the delays hold 0 (where there are two) and H, the gains have both signs"""
    rng = np.random.default_rng(100 * L + H + seed)
    delays = np.array([H]) if L == 1 else np.concatenate([[0, H], rng.choice(np.arange(1, max(H, L + 1)), L - 2, replace=False)])
    delays = np.minimum(rng.permutation(delays), H)
    sign = lambda: rng.choice([-1.0, 1.0], L)                              # noqa: E731
    return ch.Profile.of_gains(delays, sign() * rng.uniform(0.3, 1.0, L), sign() * rng.uniform(0.3, 1.0, L), rng.uniform(-1.0, 1.0, L))


def _strided(x, pad, offset=1):
    """x (R, n) on the device in rows `pad` samples wider than n, the whole matrix `offset` samples (8 bytes each) off its
    allocation: with offset 1 and an odd stride the base is on 8 but not 16 bytes and every other row on 16"""
    torch = _torch()
    R, n = x.shape
    flat = torch.full((R * (n + pad) + offset,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
    view = flat[offset:].view(R, n + pad)[:, :n]
    view.copy_(torch.from_numpy(x))
    return flat, view


SHAPES = [(1, 1, 0, 0), (2, 5, 0, 3), (1, 16, 6, 0), (3, 8, 4, 17), (16, 32, 12, 1024)]


@pytest.mark.parametrize("where", ["0", "1", "B-1", "end"])
@pytest.mark.parametrize("L,S,b,H", SHAPES)
def test_equals_the_restatement_bit_for_bit(L, S, b, H, where):
    """Three rows of two tiles and a sample, strides wider than the rows on both sides, the input on 8 but not 16 bytes, rows
    beyond 2^32, the first sample at 0, 1, B - 1 and as late as the entry takes; the padding of out keeps its sentinel."""
    torch = _torch()
    tile, lds = _lib.channel_plan(L, S, b, H)
    R, count = 3, 2 * tile + 1
    n0 = {"0": 0, "1": 1, "B-1": (1 << b) - 1, "end": (1 << 40) - count - 1}[where]
    profile, doppler = _profile(L, H, S), 0.01
    x = _signal(R, count + H, 7 * L + S)
    _, x_dev = _strided(x, pad=3)
    assert x_dev.data_ptr() % 16 == 8 and x_dev.stride(0) == count + H + 3
    out_flat, out_dev = _strided(np.full((R, count), SENTINEL), pad=5, offset=0)
    got = ch.apply(x_dev, profile, doppler=doppler, sinusoids=S, interp_log2=b, seed=SEED, row_index0=ROW0, sample_index0=n0, out=out_dev)
    assert got is out_dev
    y = _cpu(out_flat).reshape(R, count + 5)
    rec, dm = profile.records(S), ch.doppler_max_of(doppler)
    for f in range(R):
        want = ref.restate(x[f], rec, S, b, dm, ref.RANDOM_PHASE, seed=SEED, r=ROW0 + f, n0=n0)
        assert y[f, :count].tobytes() == want.tobytes(), (L, S, b, H, where, f, int(np.argmax(y[f, :count] != want)))
    assert (y[:, count:] == SENTINEL).all()
    assert np.isfinite(y.view(np.float32)).all() and not np.array_equal(y[0, :count], y[1, :count])


def _seam_and_seeded_rows(R, count, seed):
    """the rows on either side of every line seam, the first and the last, and `count` seeded ones"""
    seams = [0, 1, LINE - 1, LINE, LINE + 1, 2 * LINE - 1, 2 * LINE]
    assert R == 2 * LINE + 1
    return np.union1d(seams, np.random.default_rng(seed).choice(R, count, replace=False))


def test_rows_over_three_lines_of_the_grid():
    """2 LINE + 1 rows of one tile: the launch is folded into three lines, the last with one live workgroup, so the
    `blockIdx.y` term, the whole-workgroup return and `f * stride` at f >= 2^16 are executed.  The seam rows and 2048 seeded ones
    == the restatement (a cap on the reference's time, about 1 ms a row); EVERY row the bytes of three calls of at most LINE
    rows -- single-line grids, the shape the tests above hold to the restatement -- with row_index0 advanced.  The same with a
    sigma per group of three rows on the device, a.sigma[f / frames_per_group] at f >= 2^16, cut on group boundaries."""
    torch = _torch()
    L, S, b, H, count, n0 = 2, 2, 1, 1, 2, 5
    R = 2 * LINE + 1
    tile, _ = _lib.channel_plan(L, S, b, H)
    tiles_per_row = -(-count // tile)
    assert tiles_per_row == 1
    items = R * tiles_per_row
    print(f"channel: {items} items, LINE = {LINE}")
    assert items >= 2 * LINE + 1
    profile, doppler = _profile(L, H, S), 0.01
    assert sorted(profile.delays.tolist()) == [0, 1]
    x = _signal(R, count + H, 29)
    _, x_dev = _strided(x, pad=3)
    assert x_dev.stride(0) == count + H + 3
    kw = dict(doppler=doppler, sinusoids=S, interp_log2=b, seed=SEED, sample_index0=n0)

    def whole(**more):
        buf = torch.full((R + 2, count + 5), complex(SENTINEL), dtype=torch.complex64, device="cuda")
        got = ch.apply(x_dev, profile, row_index0=ROW0, out=buf[:R, :count], **kw, **more)
        assert got.data_ptr() == buf.data_ptr() and got.stride(0) == count + 5
        y = _cpu(buf)
        assert (y[:R, count:] == SENTINEL).all() and (y[R:] == SENTINEL).all()
        return np.ascontiguousarray(y[:R, :count])

    def in_cuts(cuts, sigma_of=None, **more):
        parts, at = [], 0
        for rows in cuts:
            assert rows <= LINE
            extra = {} if sigma_of is None else dict(sigma=sigma_of(at, rows))
            parts.append(_cpu(ch.apply(x_dev[at:at + rows], profile, row_index0=ROW0 + at, **kw, **extra, **more)))
            at += rows
        assert at == R
        return np.concatenate(parts)

    y = whole()
    rec, dm = profile.records(S), ch.doppler_max_of(doppler)
    for f in _seam_and_seeded_rows(R, 2048, 31):
        want = ref.restate(x[f], rec, S, b, dm, ref.RANDOM_PHASE, seed=SEED, r=ROW0 + int(f), n0=n0)
        assert y[f].tobytes() == want.tobytes(), (int(f), y[f], want)
    assert y.tobytes() == in_cuts((LINE, LINE, 1)).tobytes()
    # a sigma per group of three rows, on the device
    fpg = 3
    sig = torch.tensor([0.5, 0.0, 2.0], dtype=torch.float32, device="cuda").repeat(-(-R // (3 * fpg)))[:-(-R // fpg)].contiguous()
    noisy = whole(sigma=sig, frames_per_group=fpg)
    cuts = (LINE - 1, LINE - 1, 3)
    assert all(rows % fpg == 0 for rows in cuts)
    parts = in_cuts(cuts, sigma_of=lambda at, rows: sig[at // fpg:(at + rows) // fpg].contiguous(), frames_per_group=fpg)
    assert noisy.tobytes() == parts.tobytes()
    group = np.arange(R) // fpg
    silent = group % 3 == 1
    assert silent[LINE:].sum() >= LINE // 3 and noisy[silent].tobytes() == y[silent].tobytes()
    assert (noisy[~silent] != y[~silent]).any(axis=1).all()


def test_one_unit_line_of_sight_is_the_identity_and_the_noise_is_the_generators():
    """One path (0, 0, 1.0, 0), no flag, no Doppler, on generate(..., sigma=None) with sigma: generate(..., sigma) of the same
    seed, rows and samples."""
    kw = dict(sps=(8, 3), taps=wf.design_rrc(8, 4), seed=21, row_index0=ROW0, sample_index0=5, cfo=0.01)
    sig = np.array([0.5, 0.0, 2.0], np.float32)
    clean = wf.generate("16QAM", 3, 1500, **kw)
    want = _cpu(wf.generate("16QAM", 3, 1500, sigma=sig, **kw))
    profile = ch.static([0], [1.0])
    assert profile.records(16).tolist() == [(0, 0.0, 1.0, 0)]
    got = _cpu(ch.apply(clean, profile, seed=21, row_index0=ROW0, sample_index0=5, sigma=sig, random_phase=False))
    assert np.array_equal(got, want) and not np.array_equal(got[0], _cpu(clean)[0]) and np.array_equal(got[1], _cpu(clean)[1])


def test_static_paths_are_the_down_converters_sparse_filter():
    torch = _torch()
    delays, gains = [0, 3, 17, 40], [0.75, -0.5, 0.25, 0.125]
    h = np.zeros(41, np.float32)
    h[delays] = gains
    x = _signal(2, 3000 + 40, 3)
    x_dev = torch.from_numpy(x).cuda()
    got = _cpu(ch.apply(x_dev, ch.static(delays[::-1], gains[::-1]), random_phase=False, seed=5, interp_log2=0))
    again = _cpu(ch.apply(x_dev, ch.static(delays, gains), random_phase=False, seed=6))
    for f in range(2):
        want = _cpu(ddc.tune_decimate(x_dev[f].contiguous(), h, 1, shift=0.0))
        assert want.shape == (3000,) and np.array_equal(got[f], want) and np.array_equal(again[f], want)


def test_a_stream_cut_into_chunks_equals_one_call():
    """chunks of 1, 2, 255, 256, 257 and B - 1, B + 1 samples, in turn, over 10 007 samples"""
    torch = _torch()
    b, n = 6, 10007
    profile = ch.exponential(3, 5, 3.0)
    kw = dict(doppler=2e-3, sinusoids=8, interp_log2=b, seed=SEED, snr_db=10.0)
    x = _signal(1, n, 11)[0]
    x_dev = torch.from_numpy(x).cuda()
    whole = _cpu(ch.apply(torch.cat([x_dev.new_zeros(profile.history), x_dev])[None, :], profile, row_index0=9, **kw))[0]
    fader = ch.Fader(profile, row=9, **kw)
    sizes, parts, at = (1, 2, 255, 256, 257, (1 << b) - 1, (1 << b) + 1), [], 0
    while at < n:
        size = min(sizes[len(parts) % len(sizes)], n - at)
        parts.append(fader.push(x_dev[at:at + size]))
        assert parts[-1].shape == (size,)
        at += size
    assert fader.index == n and len(parts) > 2 * len(sizes)
    assert np.concatenate([_cpu(p) for p in parts]).tobytes() == whole.tobytes()


def test_rows_cut_into_two_calls_and_a_graph_replay_equal_one_call():
    torch = _torch()
    profile = ch.two_ray(9, -3.0)
    kw = dict(doppler=1e-3, sinusoids=16, seed=31, sample_index0=77)
    x_dev = torch.from_numpy(_signal(5, 3000 + 9, 13)).cuda()
    sig = torch.tensor([0.5, 0.25, 0.125], dtype=torch.float32, device="cuda")
    want = _cpu(ch.apply(x_dev, profile, row_index0=ROW0, sigma=sig, frames_per_group=2, **kw))
    first = _cpu(ch.apply(x_dev[:2], profile, row_index0=ROW0, sigma=sig[:1], **kw))
    rest = _cpu(ch.apply(x_dev[2:], profile, row_index0=ROW0 + 2, sigma=sig[1:], frames_per_group=2, **kw))
    assert np.concatenate([first, rest]).tobytes() == want.tobytes()
    out = torch.zeros((5, 3000), dtype=torch.complex64, device="cuda")

    def launch():
        return ch.apply(x_dev, profile, row_index0=ROW0, sigma=sig, frames_per_group=2, out=out, **kw)

    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        assert launch() is out                                 # the stream's first call is outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            launch()
    out.fill_(-1.0)
    torch.cuda.synchronize()
    g.replay()
    assert _cpu(out).tobytes() == want.tobytes()
    with pytest.raises(ValueError):                            # the kernel reads neighbours of the sample it writes
        ch.apply(x_dev, profile, out=x_dev[:, :3000], **kw)


def test_noise_with_fading_meets_the_generators_bound():
    torch = _torch()
    profile, S, b, doppler = ch.rician(3.0, 0.5), 8, 3, 5e-3
    R, count, n0 = 3, 2500, (1 << 39) + 1
    sig = np.array([0.3, 2.0, 0.0], np.float32)
    x = _signal(R, count, 17)
    y = _cpu(ch.apply(torch.from_numpy(x).cuda(), profile, doppler=doppler, sinusoids=S, interp_log2=b, seed=SEED, row_index0=ROW0,
                      sample_index0=n0, sigma=sig))
    rec, dm, worst = profile.records(S), ch.doppler_max_of(doppler), 0.0
    n = n0 + np.arange(count, dtype=np.int64)
    for f in range(R):
        signal = ref.restate(x[f], rec, S, b, dm, ref.RANDOM_PHASE, seed=SEED, r=ROW0 + f, n0=n0)
        if sig[f] == 0.0:
            assert y[f].tobytes() == signal.tobytes()
            continue
        out64 = signal.astype(np.complex128) + ref.synth_ref.noise64(SEED, ROW0 + f, n, float(sig[f]))[0]
        ratio = np.abs(y[f].astype(np.complex128) - out64) / ref.noise_bound(SEED, ROW0 + f, n, float(sig[f]), out64)
        worst = max(worst, float(ratio.max()))
        assert not np.array_equal(y[f], signal)
    print(f"channel noise: worst |err| / bound = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("b", [0, None])
def test_ones_through_one_path_give_the_closed_form_gain(b):
    """interp_log2 = 0 and the default: within the interpolation chord plus the rounding (tests/channel_ref.physics_bound)"""
    torch = _torch()
    S, doppler, R, count, n0 = 16, 1.0 / 256, 4, 3001, 1000
    b = ch.default_interp_log2(doppler) if b is None else b
    ones = torch.ones((R, count), dtype=torch.complex64, device="cuda")
    y = _cpu(ch.apply(ones, ch.rayleigh(), doppler=doppler, sinusoids=S, interp_log2=b, seed=SEED, row_index0=ROW0, sample_index0=n0))
    rec, dm = ch.rayleigh().records(S), ch.doppler_max_of(doppler)
    g = ref.gain64(SEED, ROW0 + np.arange(R), rec, S, dm, ref.RANDOM_PHASE, n0 + np.arange(count))[:, 0, :]
    worst = float(np.abs(y.astype(np.complex128) - g).max()) / ref.physics_bound(S, doppler, b)
    print(f"channel gain, interp_log2 = {b}: worst |err| / bound = {worst:.4f}")
    assert worst <= 1.0
    assert 0.5 < float((np.abs(g) ** 2).mean()) < 2.0


def test_faded_features_end_to_end():
    kw = dict(seed=3, channel=dict(profile=ch.rician(6), doppler=1e-3))
    faded = wf.dataset_features(["BPSK", "QPSK"], [10], 64, 2048, **kw)
    again = wf.dataset_features(["BPSK", "QPSK"], [10], 64, 2048, chunk_frames=24, **kw)
    plain = wf.dataset_features(["BPSK", "QPSK"], [10], 64, 2048, seed=3)
    for mod in ("BPSK", "QPSK"):
        assert faded[mod].shape == (1, 64, 18) and np.isfinite(faded[mod]).all()
        assert faded[mod].tobytes() == again[mod].tobytes()
        assert not np.array_equal(faded[mod], plain[mod])
