"""The one cut of a container over W workers (sharding.FrameCut), the one normaliser of what a caller hands an engine
(frame_sources.as_frame_rows), and the three places that use them: extract_modulation, DeviceFanOut, the rank loop of
run_extraction.  Stand-in engines throughout; the last test runs the fan-out on a real device."""
from concurrent.futures import Future

import numpy as np
import pytest

from amcpy_amd import feature_extraction as fe
from amcpy_amd.features import SC16
from amcpy_amd.sharding import FrameCut, shard_by_frames


def _marker_features(block):
    """A stand-in engine: 18 columns that depend on every sample of the frame."""
    block = np.asarray(block)
    if block.dtype == SC16:
        block = block["i"].astype(np.float64) + 1j * block["q"]
    base = np.abs(block).sum(axis=1, dtype=np.float64) + np.real(block[:, 0])
    return (base[:, None] * np.arange(1, 19)[None, :]).astype(np.float32)


class _Stub:
    """An engine that records the source it was handed."""

    def __init__(self, device, seen):
        self.device, self.stats, self.seen = device, {}, seen

    def __call__(self, rows):
        self.seen[self.device] = rows
        return _marker_features(rows.to_array())


def _where(src):
    return (type(src), src.k_lo, src.k_hi) if isinstance(src, fe.FrameColumns) else (type(src), src.lo, src.hi)


def _check_cut(cut, n_snr, n_frames, world, by_frames):
    F = n_snr * n_frames
    assert cut.by_frames == by_frames and cut.world == world
    ranges = [cut.range(r) for r in range(world)]
    assert ranges[0][0] == 0 and ranges[-1][1] == (n_frames if by_frames else F)        # tiles the axis exactly once,
    assert all(a <= b for a, b in ranges) and all(ranges[r][1] == ranges[r + 1][0] for r in range(world - 1))   # in order
    assert sum(cut.rows(r) for r in range(world)) == F
    single = np.arange(F * 3, dtype=np.float32).reshape(F, 3)       # the single-worker snr-major result: row g marks frame g
    out = np.full((F, 3), np.nan, dtype=np.float32)
    for r, (a, b) in enumerate(ranges):
        block = single.reshape(n_snr, n_frames, 3)[:, a:b].reshape(-1, 3) if by_frames else single[a:b]
        assert block.shape[0] == cut.rows(r)
        cut.place(out, r, block.copy())
    assert np.array_equal(out, single)


def test_frame_cut_exhaustively_small():
    for world in range(1, 9):
        for n_snr in range(1, 6):
            for n_frames in range(0, 10):
                _check_cut(FrameCut(n_snr, n_frames, world), n_snr, n_frames, world, shard_by_frames(n_snr, n_frames, world))
        for F in range(0, 21):
            _check_cut(FrameCut.flat(F, world), 1, F, world, False)


@pytest.mark.parametrize("n_snr,n_frames,by_frames", [(3, 40, True), (5, 3, False)])
def test_one_cut_in_three_places(n_snr, n_frames, by_frames):
    """extract_modulation's share per rank, DeviceFanOut's per device and the rank loop's per rank are the same source."""
    W, N = 4, 12
    rng = np.random.default_rng(11)
    parsed = np.asfortranarray(rng.standard_normal((n_snr, n_frames, N)) + 1j * rng.standard_normal((n_snr, n_frames, N)))
    rows = fe.FrameRows(parsed, n_snr, n_frames)
    assert shard_by_frames(n_snr, n_frames, W) == by_frames
    # extract_modulation: ranks simulated by calling its share helper per rank
    cut = fe._frame_cut(rows, W)
    per_rank = [_where(fe._share(rows, cut, r)) for r in range(W)]
    assert {t for t, _, _ in per_rank} == {fe.FrameColumns if by_frames else fe.FrameRows}
    # DeviceFanOut
    seen = {}
    fan = fe.DeviceFanOut(N, list(range(W)), threads=1)
    fan.engines = [_Stub(d, seen) for d in range(W)]
    want = _marker_features(rows.to_array())
    assert np.array_equal(fan(rows), want)
    fan.close()
    assert all(b > a for _, a, b in per_rank)                   # (an empty share would not reach its engine)
    assert [_where(seen[d]) for d in range(W)] == per_rank
    # the rank loop: step 2 of every rank, on ranks that decoded for themselves
    out = np.empty_like(want)
    for r in range(W):
        seen = {}
        fut = Future()
        fut.set_result((parsed, n_snr, n_frames))
        run = fe._RankRun(None, None, False, r, W, _Stub(r, seen), False, {}, [])
        rcut, local, failure = fe._compute_share(run, "mod", fut, None)
        assert failure is None and rcut.by_frames == by_frames and local.shape == (rcut.rows(r), 18)
        assert _where(seen[r]) == per_rank[r]
        rcut.place(out, r, local)
    assert np.array_equal(out, want)


def _same_frames():
    """(frames as complex128 with integer parts that int16 and float32 hold exactly, every form of them)."""
    rng = np.random.default_rng(3)
    pairs = rng.integers(-300, 300, size=(7, 10, 2)).astype(np.int16)
    z = pairs[..., 0].astype(np.float64) + 1j * pairs[..., 1]
    return pairs, z


def _complex(a):
    return a["i"].astype(np.float64) + 1j * a["q"] if a.dtype == SC16 else np.asarray(a, dtype=np.complex128)


def test_as_frame_rows_takes_every_form(tmp_path):
    pairs, z = _same_frames()
    mm = np.memmap(tmp_path / "f.bin", dtype=np.complex128, mode="w+", shape=z.shape, order="F")
    mm[:] = z
    assert mm.flags.f_contiguous and not mm.flags.c_contiguous
    forms = [z, mm, fe.FrameRows(z[None], 1, z.shape[0]), pairs, pairs.view(SC16)[..., 0]]
    for t in (np.float32, np.float64):
        forms.append(fe.SplitComplex(z.real.astype(t), z.imag.astype(t)))
    for form in forms:
        rows = fe.as_frame_rows(form)
        assert isinstance(rows, fe.FrameRows) and rows.shape == z.shape
        assert np.array_equal(_complex(rows.to_array()), z)
    ready = forms[2]
    assert fe.as_frame_rows(ready) is ready
    assert fe.as_frame_rows(pairs).dtype == SC16 and np.shares_memory(fe.as_frame_rows(pairs).parsed, pairs)
    for t in (np.float32, np.float64):                          # a real signal: no imaginary part
        rows = fe.as_frame_rows(fe.SplitComplex(z.real.astype(t), None))
        assert np.array_equal(_complex(rows.to_array()), z.real)
    for bad in (np.zeros((2, 3, 4), np.complex64), np.zeros(5, np.complex64)):
        with pytest.raises(ValueError, match=r"expected \(F, L\) frames, got shape"):
            fe.as_frame_rows(bad)


def test_device_fan_out_takes_what_one_engine_takes():
    """A SplitComplex and int16 pairs, which DeviceFanOut used to refuse or mangle: as one stand-in engine, bit for bit."""
    pairs, z = _same_frames()
    N = z.shape[1]
    for frames in (fe.SplitComplex(z.real.copy(), z.imag.copy()), pairs):
        fan = fe.DeviceFanOut(N, [0, 1, 2], threads=1)
        fan.engines = [_Stub(d, {}) for d in range(3)]
        got = fan(frames)
        fan.close()
        want = _Stub(0, {})(fe.as_frame_rows(frames))
        assert got.shape == (z.shape[0], 18) and got.dtype == np.float32 and np.array_equal(got, want)
        assert np.array_equal(want, _marker_features(z))


@pytest.mark.gpu
def test_device_fan_out_equals_one_engine_on_gpu():
    """DeviceFanOut(128, [0, 0]) -- the device listed twice -- against HipEngine(128), bit for bit: a (2, 4, 128)
    SplitComplex container (world 2 cuts its frame axis: 4 * 8 <= 4 * 9), a (2, 5, 128) one (the flattening:
    6 * 8 > 5 * 9) and (10, 128, 2) int16 pairs."""
    N = 128
    rng = np.random.default_rng(17)
    cases = []
    for n_frames, by_frames in ((4, True), (5, False)):
        re, im = (np.asfortranarray(rng.standard_normal((2, n_frames, N)).astype(np.float32)) for _ in range(2))
        assert shard_by_frames(2, n_frames, 2) == by_frames
        cases.append(fe.FrameRows(fe.SplitComplex(re, im), 2, n_frames))
    cases.append(rng.integers(-2000, 2000, size=(10, N, 2)).astype(np.int16))
    one, fan = fe.HipEngine(N), fe.DeviceFanOut(N, [0, 0])
    try:
        for frames in cases:
            want, got = one(frames), fan(frames)
            assert want.shape == (10 if isinstance(frames, np.ndarray) else frames.shape[0], 18)
            assert want.any() and np.array_equal(got, want)
            assert sum(fan.stats["frames_per_device"]) == want.shape[0] and min(fan.stats["frames_per_device"]) > 0
    finally:
        fan.close()
        one.close()


def test_rank_readers_publish_each_modulation_under_its_own_path(tmp_path, monkeypatch):
    """The reader choice of the rank loop, and rank 0's shared-host reader with its three threads publishing AT ONCE (a
    barrier inside the stand-in publisher holds them together): every modulation is announced under the path its own
    publish returned, and `published` holds each path once."""
    import functools
    import threading
    from pathlib import Path
    from amcpy_amd.config import Config, Paths, SignalConfig
    cfg = Config(paths=Paths(root=tmp_path), signals=SignalConfig(snr_values={0: "0", 1: "10"}, num_frames=3, frame_size=8))
    mods = list(cfg.signals.modulations_with_noise)
    assert len(mods) == 6                                        # two rounds of three readers
    key_of = {cfg.signals.mat_info[m]: m for m in mods}
    arrays = {m: np.full((2, 3, 8), i + 1, np.complex64) for i, m in enumerate(mods)}
    together = threading.Barrier(3)

    def load(mat_path, key, pool=None, direct=False):
        return arrays[key_of[key]]

    def publish(parsed, n_snr, n_frames, N, threads):
        try:
            together.wait(timeout=10)
        except threading.BrokenBarrierError:
            pass
        return Path(f"/nowhere/{int(parsed[0, 0, 0].real)}.npy")

    monkeypatch.setattr(fe, "_load_variable", load)
    monkeypatch.setattr(fe, "_publish_container", publish)

    def run_of(rank, shared_host):
        return fe._RankRun(cfg, tmp_path / "x.mat", False, rank, 4, None, shared_host, {}, [])

    assert fe._rank_reader(run_of(0, False)) is fe.decode_locally and fe._rank_reader(run_of(3, False)) is fe.decode_locally
    assert fe._rank_reader(run_of(0, True)) is fe.decode_and_publish and fe._rank_reader(run_of(1, True)) is None
    run = run_of(0, True)
    for mod, fut in fe._prefetched(mods, functools.partial(fe._rank_reader(run), run)):
        assert fut.result() == (f"/nowhere/{mods.index(mod) + 1}.npy", 2, 3)
    assert sorted(run.published) == sorted(Path(f"/nowhere/{i + 1}.npy") for i in range(6)) and not run.mapped
    parsed, n_snr, n_frames = fe.decode_locally(run_of(2, False), mods[4])
    assert parsed is arrays[mods[4]] and (n_snr, n_frames) == (2, 3)
