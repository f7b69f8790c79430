"""The persistent launches that tests/persistent_loops.py lists and no other GPU test takes three times round their loop: the
feature kernels of every frame size (amcx_launch.h), the block and stream kernels, the two widening kernels, the scaler, the
classifier, the range and the Q15 kernels.

Every case gives its launch at least 2 grid + 1 units of work, so that some workgroup makes three trips and the last trip is
ragged, and prints units and grid.  These launches have no plan entry: a case RESTATES its call site -- workgroups per CU and
the unit of work -- beside the number of CUs the device reports; where a call site's count depends on LDS the case takes the
largest it can be, which only makes the case larger than it had to be.

What is asserted: a row's bits do not depend on the call it is made in (every contract here says so), so the rows of the large
call equal, bit for bit, the same rows made in calls of at most ONE trip -- the calls every other test of these kernels holds
to its reference -- and a sample of rows from the third trip is held to the reference directly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _same(a, b):
    """bit for bit, a NaN equal to a NaN; tensors on the device"""
    torch = _torch()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return bool(torch.equal(a, b))
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _three_trips(what, n, unit, per_cu):
    """n items in units of `unit` over per_cu workgroups a CU: printed, and asserted to be 2 grid + 1 units at least"""
    grid, units = per_cu * _cus(), -(-n // unit)
    print(f"{what}: {n} = {units} units of {unit} over {grid} workgroups")
    assert units >= 2 * grid + 1
    return grid


# ---- the feature kernels --------------------------------------------------------------------------------------------------------
# (frame size, variant) -> (workgroups per CU, frames per unit), from the launchers of amcx_launch.h and amcx.hip:
#   ShortSize   one per CU, kWavesPerWG (16 at 128, else 12) waves of kQuad = 4 frames
#   WaveSize    one per CU, kWavesPerWG (8 at 4096, else 16) frames
#   QuadSize    two per CU, kBatch = 4 frames;   GroupSize   one per CU, kBatch = 8 (16384) or 2 (32768) frames
#   the block kernel   min(8, 160 KiB / LDS) * 4 per CU, a frame: 32 where LDS is a few KiB, 4 at the 133 120 bytes of 4097
#   the stream kernel  one per CU (fewer where the workspace holds fewer buffers), a frame
FEATURE_SITES = {
    (128, "wave"): (1, 64), (256, "wave"): (1, 48), (512, "wave"): (1, 48),
    (1024, "wave"): (1, 16), (2048, "wave"): (1, 16), (4096, "wave"): (1, 8),
    (8192, "wave"): (2, 4), (16384, "wave"): (1, 8), (32768, "wave"): (1, 2),
    (33, "block"): (32, 1), (64, "block"): (32, 1), (65, "block"): (32, 1), (4097, "block"): (4, 1),
    (8200, "auto"): (1, 1),
}
KERNEL_OF = {33: "amcx_features18_block_kernel<0>", 64: "amcx_features18_block_kernel<1>", 65: "amcx_features18_block_kernel<2>",
             4097: "amcx_features18_block_kernel<3>", 8200: "amcx_features18_stream_kernel"}


def _base_frames(N):
    """26 frames: the six modulations at four SNRs, a frame of zeros and one with a NaN"""
    from amcpy_amd import synth
    x = np.concatenate([synth.host_block(m, snr, 1, N, seed=3300 + 7 * i + j)
                        for i, m in enumerate(synth.MODS6) for j, snr in enumerate((-6.0, 0.0, 12.0, 30.0))]
                       + [np.zeros((2, N))]).astype(np.complex64)
    x[-1, N // 3] = complex(np.nan, 1.0)
    return x


def _frames_on_device(N, F):
    """(F frames drawn from the base frames, on the device; the base frames; which base frame each is)"""
    torch = _torch()
    base = _base_frames(N)
    pick = np.random.default_rng(N).integers(0, base.shape[0], F)
    pick[[0, F // 2, F - 1]] = [base.shape[0] - 1, base.shape[0] - 2, 3]      # the NaN frame first, the ordinary one last
    return torch.from_numpy(base).cuda()[torch.from_numpy(pick).cuda()].contiguous(), base, pick


def _in_one_trip_calls(fn, x, per_call):
    torch = _torch()
    return torch.cat([fn(x[lo:lo + per_call]) for lo in range(0, x.shape[0], per_call)])


@pytest.mark.parametrize("N,variant", list(FEATURE_SITES))
def test_feature_rows_over_three_trips_of_the_grid(N, variant):
    torch = _torch()
    from amcpy_amd import _lib
    from amcpy_amd.features import features18
    from oracle import iq_features_oracle as orc
    from tests.test_gpu_parity import _assert_parity
    per_cu, unit = FEATURE_SITES[(N, variant)]
    F = unit * (2 * per_cu * _cus() + 1) + 1
    grid = _three_trips(f"features N={N} {variant}", F, unit, per_cu)
    if N in KERNEL_OF:
        assert _lib.kernel_name(N, _lib.VARIANTS[variant]) == KERNEL_OF[N]
    x, base, pick = _frames_on_device(N, F)
    run = lambda v: features18(v, variant=variant)                          # noqa: E731
    got = run(x)
    assert got.shape == (F, 18) and _same(got, _in_one_trip_calls(run, x, unit * grid))
    # the base frames' own rows, from the oracle; then every row of the call is its base frame's row
    ordinary = np.arange(base.shape[0] - 2)
    first = np.array([int(np.flatnonzero(pick == b)[-1]) for b in ordinary])   # the LAST place each stands at: mostly the third trip
    rows = got[torch.from_numpy(first).cuda()].cpu().numpy()
    _assert_parity(rows, orc.features18_batch(base[ordinary].astype(np.complex128)), base[ordinary], f"three trips N={N} {variant}")
    of_base = torch.stack([got[int(np.flatnonzero(pick == b)[-1])] for b in range(base.shape[0])])
    assert _same(got, of_base[torch.from_numpy(pick).cuda()])
    assert bool(torch.isnan(got[0]).all())


def test_stream_kernel_without_a_workspace_over_three_trips_of_the_grid():
    """The DFT form of the stream kernel (no workspace: amcx_features18_stream_kernel<false>), through the C entry."""
    torch = _torch()
    from amcpy_amd import _lib
    lib = _lib.load()
    N, F = 8200, 2 * _cus() + 2
    grid = _three_trips(f"features N={N} stream, no workspace", F, 1, 1)
    x, _, pick = _frames_on_device(N, F)

    def run(v):
        out = torch.full((v.shape[0], 18), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.amcx_features18_c64_ws(v.data_ptr(), v.shape[0], N, v.shape[1], out.data_ptr(), 18,
                                              torch.cuda.current_stream().cuda_stream, _lib.VARIANT_AUTO, None, 0))
        return out

    got = run(x)
    assert _same(got, _in_one_trip_calls(run, x, grid))
    of_base = torch.stack([got[int(np.flatnonzero(pick == b)[-1])] for b in range(int(pick.max()) + 1)])
    assert _same(got, of_base[torch.from_numpy(pick).cuda()])


@pytest.mark.parametrize("N,ids", [(128, (10, 12)), (128, (2, 3)), (2048, (10, 12)), (2048, (2, 3))])
def test_plan_kernels_over_three_trips_of_the_grid(N, ids):
    """The feature-plan kernels (cumulants alone; everything but the spectral term) share their size's launch: the columns
    asked for are the full computation's bits, the others NaN."""
    torch = _torch()
    from amcpy_amd.features import features18
    per_cu, unit = FEATURE_SITES[(N, "wave")]
    F = unit * (2 * per_cu * _cus() + 1) + 1
    _three_trips(f"features N={N} ids={ids}", F, unit, per_cu)
    x, _, _ = _frames_on_device(N, F)
    full, part = features18(x), features18(x, feature_ids=ids)
    cols = [i - 1 for i in ids]
    others = [c for c in range(18) if c not in cols]
    assert _same(part[:, cols], full[:, cols]) and bool(torch.isnan(part[:, others]).all())


def _widened(raw, scale):
    """complex64(float32(I) * scale, float32(Q) * scale) of integer pairs (..., 2), on the device"""
    torch = _torch()
    return torch.view_as_complex((raw.to(torch.float32) * np.float32(scale)).contiguous())


@pytest.mark.parametrize("fmt,N,variant", [("sc16", 128, "wave"), ("sc16", 2048, "wave"), ("sc16", 65, "block"), ("ci8", 4096, "wave"),
                                           ("ci8", 8192, "wave")])
def test_integer_frames_over_three_trips_of_the_grid(fmt, N, variant):
    """sc16 at 128 and 2048: the sizes' own sc16 kernels.  sc16 at 65 (block): amcx_sc16_to_c64_kernel, 8 workgroups per CU,
    256 samples a unit.  ci8: amcx_iq8_to_sc16_kernel (4096) and amcx_iq8_to_c64_kernel (8192), 8 per CU, 256 items of 8
    samples a unit.  The rows are the bits of the complex64 call on the widened frames."""
    torch = _torch()
    from amcpy_amd import _formats
    from amcpy_amd.features import features18, features18_iq8, features18_sc16
    per_cu, unit = FEATURE_SITES[(N, variant)]
    F = unit * (2 * per_cu * _cus() + 1) + 1
    _three_trips(f"features {fmt} N={N} {variant}", F, unit, per_cu)
    if (fmt, N) == ("sc16", 65):
        _three_trips("sc16 widening", F * N, 256, 8)
    if fmt == "ci8":
        _three_trips("ci8 widening", F * (N // 8), 256, 8)
    info = np.iinfo(_formats.get(fmt).plain)
    base = torch.from_numpy(np.random.default_rng(N).integers(info.min, info.max + 1, (24, N, 2)).astype(_formats.get(fmt).plain)).cuda()
    raw = base[torch.from_numpy(np.random.default_rng(N + 1).integers(0, 24, F)).cuda()].contiguous()
    scale = _formats.get(fmt).scale
    got = (features18_sc16 if fmt == "sc16" else features18_iq8)(raw, variant=variant)
    assert got.shape == (F, 18) and _same(got, features18(_widened(raw, scale), variant=variant))


# ---- the scaler, the classifier, the range and the Q15 kernels ------------------------------------------------------------------
USED = (2, 4, 6, 8, 12, 14)
WIDTHS = (6, 9, 4)
TILE_ROWS = 512                                    # kMlpTileRows of amcx_mlp_shape.h


def _rows(n):
    """(n, 18) float32 on the device, a NaN or an infinity in a used column of a few rows of every trip"""
    torch = _torch()
    g = torch.Generator(device="cuda")
    g.manual_seed(33)
    x = torch.randn((n, 18), generator=g, device="cuda") * 3.0 + 0.5
    for r, v in ((0, np.nan), (511, np.inf), (512, -np.inf), (n // 2 + 3, np.nan), (n - 700, np.inf), (n - 1, np.nan)):
        x[r, USED[r % 6]] = v
    return x


GROUP = 4099                                       # rows per group of the counts: a group straddles tiles and trips


def _network_rows():
    """rows for 2 grid + 1 tiles of the classifier and the Q15 kernel (4 workgroups per CU) and a ragged tile more: the next
    whole number of groups (the entries count whole groups alone)"""
    n = -(-(TILE_ROWS * (2 * 4 * _cus() + 1) + 1) // GROUP) * GROUP
    if n % TILE_ROWS == 0:
        n += GROUP
    return n, _rows(n)


def _scaler():
    rng = np.random.default_rng(34)
    return rng.standard_normal(6), 0.5 + 2.0 * rng.random(6)


def test_select_scale_over_three_trips_of_the_grid():
    """amcx_select_scale_f32: 8 workgroups per CU, 256 outputs a unit.  Every output is float(float(x - mean) / scale), the
    subtraction and the division in IEEE double -- computed by torch in float64 on the device."""
    torch = _torch()
    from amcpy_amd import _lib
    n, x = _network_rows()
    _three_trips("select and scale", n * 6, 256, 8)
    mean, scale = (torch.from_numpy(v).cuda() for v in _scaler())
    cols = torch.tensor(USED, dtype=torch.int32, device="cuda")
    out = torch.full((n + 1, 7), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().amcx_select_scale_f32(x.data_ptr(), n, 18, cols.data_ptr(), 6, mean.data_ptr(), scale.data_ptr(),
                                                 out.data_ptr(), 7, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    want = ((x[:, list(USED)].double() - mean).float().double() / scale).float()
    assert _same(out[:n, :6], want) and bool((out[:, 6] == -7.0).all()) and bool((out[n] == -7.0).all())


def test_classifier_over_three_trips_of_the_grid():
    """amcx_mlp_classify_kernel: 4 workgroups per CU, a tile of 512 rows a unit.  Labels and probabilities equal the same rows
    in calls of one trip; the counts are the labels' histogram per group."""
    torch = _torch()
    from amcpy_amd.classifier import MlpModel, classify, params_floats
    from tests import post_shapes as ps
    n, x = _network_rows()
    grid = _three_trips("classifier", n, TILE_ROWS, 4)
    mean, scale = _scaler()
    model = MlpModel(WIDTHS, "tanh", np.random.default_rng(35).standard_normal(params_floats(WIDTHS)).astype(np.float32))
    kw = dict(cols=USED, mean=mean, scale=scale)
    labels, probs, counts = classify(x, model, rows_per_group=GROUP, want=("labels", "probs", "counts"), **kw)
    per = TILE_ROWS * grid
    parts = [classify(x[lo:lo + per], model, want=("labels", "probs"), **kw) for lo in range(0, n, per)]
    assert _same(labels, torch.cat([p[0] for p in parts])) and _same(probs, torch.cat([p[1] for p in parts]))
    lab = labels.cpu().numpy()
    assert (lab == -1).sum() == 6 and len(set(lab.tolist())) >= 3
    assert np.array_equal(counts.cpu().numpy(), ps.group_counts(lab, GROUP, 4))


def test_ranges_over_three_trips_of_the_grid():
    """amcx_mlp_range_kernel: 2 workgroups per CU, a tile of 512 rows a unit.  The ranges of all rows are the minimum and the
    maximum of the ranges of the same rows in calls of one trip, the skipped rows their sum."""
    from amcpy_amd import quantize as qz
    from amcpy_amd.classifier import MlpModel, params_floats
    n = TILE_ROWS * (2 * 2 * _cus() + 1) + 1
    x = _rows(n)
    grid = _three_trips("ranges", n, TILE_ROWS, 2)
    mean, scale = _scaler()
    model = MlpModel(WIDTHS, "relu", np.random.default_rng(36).standard_normal(params_floats(WIDTHS)).astype(np.float32))
    for activation in ("relu", "none"):
        kw = dict(cols=USED, mean=mean, scale=scale, activation=activation)
        got, skipped = qz.calibrate(x, model, **kw)
        per = TILE_ROWS * grid
        parts = [qz.calibrate(x[lo:lo + per], model, **kw) for lo in range(0, n, per)]
        lo = np.min([p[0][:, 0] for p in parts], axis=0)
        hi = np.max([p[0][:, 1] for p in parts], axis=0)
        assert np.array_equal(got[:, 0], lo) and np.array_equal(got[:, 1], hi) and np.isfinite(got).all()
        assert skipped == sum(p[1] for p in parts) == 6


def test_q15_over_three_trips_of_the_grid():
    """amcx_mlp_q15_kernel: 4 workgroups per CU, a tile of 512 rows a unit.  Labels and logits equal the same rows in calls of
    one trip and, on the last 4096 rows, the int64 restatement; the saturation counts add up over the calls."""
    torch = _torch()
    from amcpy_amd import quantize as qz
    from tests import post_shapes as ps, quantize_ref as qr
    n, x = _network_rows()
    grid = _three_trips("Q15 classifier", n, TILE_ROWS, 4)
    mean, scale = _scaler()
    rng = np.random.default_rng(37)
    block = rng.integers(-1024, 1024, sum(WIDTHS[l + 1] * (WIDTHS[l] + 1) for l in range(2))).astype(np.int16)
    q = qz.QuantizedMlp(WIDTHS, block, 11, [12, 12], [12, 12], [10, 10])
    kw = dict(cols=USED, mean=mean, scale=scale)
    labels, logits, counts, saturated = qz.classify_q15(x, q, rows_per_group=GROUP, **kw)
    per = TILE_ROWS * grid
    parts = [qz.classify_q15(x[lo:lo + per], q, want=("labels", "logits", "saturated"), **kw) for lo in range(0, n, per)]
    assert _same(labels, torch.cat([p[0] for p in parts])) and _same(logits, torch.cat([p[1] for p in parts]))
    assert _same(saturated, sum(p[2] for p in parts))
    lab = labels.cpu().numpy()
    assert (lab == -1).sum() == 6 and np.array_equal(counts.cpu().numpy(), ps.group_counts(lab, GROUP, 4))
    tail = x[n - 4096:].cpu().numpy()
    want = qr.classify_q15(tail, list(USED), mean, scale, q.widths, q.params, q.frac_input, q.frac_weights, q.frac_biases, q.frac_outputs)
    assert np.array_equal(lab[n - 4096:], want[0]) and np.array_equal(logits[n - 4096:].cpu().numpy(), want[1])
