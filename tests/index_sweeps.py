"""Frames and index sets that aim at ONE index: a spectral peak in a prescribed FFT bin, an outlying sample at a
prescribed position (tests/test_index_sweeps_host.py checks these inputs on the CPU, tests/test_gpu_index_coverage.py
runs them through the kernels).  numpy only; nothing here touches the GPU.

Bin sweep.  Feature 1 is max_k |FFT(x)[k]|^2 / N.  Frame i of ``tone_frames(N, bins, seed)`` is a tone on bin k_i with
1e-3 of noise under it, so its feature 1 is decided by output bin k_i of the kernel's transform alone: a twiddle, a
transpose slot, a lane exchange or a step of the peak reduction that is wrong for that one bin loses the peak, and the
result falls to ~1e-6 of its value.  The reference is golden64's own definition (``peak_reference``), the bound the
project's contract for id 1: plain relative error <= 1e-5 on every frame (``bins_beyond``).

Position sweep.  Frame p of ``outlier_frames(base, positions)`` is one base frame with sample p replaced by
3 base[p] exp(2i): the envelope statistics, both phase-step statistics and the high-order sums are dominated by that
sample and its two steps, so a sample or a neighbouring pair that a kernel drops or counts twice moves the features far
beyond tests/test_gpu_parity.py::_assert_parity (``assert_position_parity`` applies it unchanged and names positions).
"""
import math

import numpy as np

TOL_F1 = 1e-5                     # the contract for feature 1 (tests/test_gpu_parity.py, module docstring)
MAX_SAMPLES = 8 << 20             # samples in one chunk of a bin sweep / through the oracle in one position case
NOISE = 1e-3                      # noise amplitude under a tone, relative to the tone
POW2_SIZES = (128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
PLAN_SIZES = (128, 256, 512, 1024, 2048, 4096)          # sizes with plan kernels and kernels that read int16


# ---------------------------------------------------------------------------------------------------------------------
# tones
# ---------------------------------------------------------------------------------------------------------------------
def tone_frames(N, bins, seed, half_bin=False):
    """complex64 (len(bins), N): frame i = A_i exp(2 pi i (k_i n / N + phi_i)) + 1e-3 A_i w_i[n], in float64, rounded once.

    A_i uniform in [0.5, 2], phi_i uniform in [0, 1) (cycles), w_i unit-power complex white noise (E |w|^2 = 1), all
    drawn from a generator seeded with (seed, N, k_i): a frame depends on its size, bin and seed only, not on which
    other bins are asked for -- the CPU checks and the chunks of a GPU sweep see the very same frames.  The tone's phase
    is 2 pi ((k n) mod N) / N with the product reduced in integers, so no accuracy is lost at large k n.
    ``half_bin``: the tone sits at k_i + 1/2 (its energy leaks into every bin with known weights)."""
    bins = np.asarray(bins, dtype=np.int64)
    assert bins.ndim == 1 and (bins >= 0).all() and (bins < N).all()
    n = np.arange(N, dtype=np.int64)
    den = 2 * N if half_bin else N
    table = np.exp(2j * np.pi * np.arange(den) / den)
    out = np.empty((len(bins), N), np.complex64)
    for i, k in enumerate(bins):
        rng = np.random.default_rng([int(seed), int(N), int(k), int(half_bin)])
        A = rng.uniform(0.5, 2.0)
        phi = rng.uniform(0.0, 1.0)
        w = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * math.sqrt(0.5)
        tone = table[((2 * k + 1) * n if half_bin else k * n) % den]
        out[i] = A * (tone * np.exp(2j * np.pi * phi) + NOISE * w)
    return out


def power_spectrum(frames):
    """|FFT|^2 / N of the complex128 cast of the frames, float64 (F, N)."""
    x = np.asarray(frames).astype(np.complex128)
    return np.abs(np.fft.fft(x, axis=-1)) ** 2 / x.shape[-1]


def peak_reference(frames):
    """golden64's definition of feature 1, stored float32."""
    return power_spectrum(frames).max(axis=-1).astype(np.float32)


def bins_beyond(got, ref, bins, tol=TOL_F1):
    """THE comparison of the bin sweeps: [(bin, plain relative error)] of the frames whose feature 1 is off by more than
    `tol` (or is not a number), in the order of `bins`."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    with np.errstate(all="ignore"):
        rel = np.abs(got - ref) / np.abs(ref)
    bad = ~(rel <= tol)
    return [(int(b), float(r)) for b, r in zip(np.asarray(bins)[bad], rel[bad])]


def assert_bins(got, ref, bins, what):
    miss = bins_beyond(got, ref, bins)
    worst = max((r for _, r in miss), default=0.0)
    assert not miss, (f"{what}: feature 1 beyond {TOL_F1:g} (plain relative) on {len(miss)} of {len(bins)} bins, worst "
                      f"{worst:.3e}; bins {[b for b, _ in miss][:64]}")


def chunks(bins, N):
    """`bins` cut into runs of at most MAX_SAMPLES / N frames."""
    per = max(1, MAX_SAMPLES // N)
    bins = np.asarray(bins)
    return [bins[a:a + per] for a in range(0, len(bins), per)]


# ---------------------------------------------------------------------------------------------------------------------
# bin sets
# ---------------------------------------------------------------------------------------------------------------------
def all_bins(N):
    return np.arange(N, dtype=np.int64)


def group_bins(N, W):
    """The group kernels (W = N / 2048 waves per frame): output bin k comes out of wave k mod W's 2048-point register
    FFT as its output index k // W.  k_j = W j + (j mod W), j = 0 ... 2047, takes every output index j once and every
    wave residue 2048 / W times; plus bins 1, N/2, N/2 + 1 and N - 1 (N/2 is k_1024 and N - 1 is k_2047 already: 2050 bins)."""
    assert N == 2048 * W
    j = np.arange(2048, dtype=np.int64)
    k = np.concatenate([W * j + j % W, [1, N // 2, N // 2 + 1, N - 1]])
    return k[np.sort(np.unique(k, return_index=True)[1])]


def edge_and_seeded_bins(N, count, seed):
    """`count` bins: the lowest 64, the highest 64, the rest drawn without replacement from those in between (a set of
    fewer than 512 bins gives an eighth of itself to either end: 8 + 8 of 64)."""
    edge = min(64, count // 8)
    assert 0 < count <= N - 2 * edge
    rng = np.random.default_rng([int(seed), int(N), int(count)])
    mid = rng.choice(np.arange(edge, N - edge, dtype=np.int64), size=count - 2 * edge, replace=False)
    return np.concatenate([np.arange(edge), np.sort(mid), np.arange(N - edge, N)]).astype(np.int64)


def half_bins(N, seed, count=64):
    """`count` seeded bins k for the off-bin tones at k + 1/2."""
    rng = np.random.default_rng([int(seed), int(N), 5])
    return np.sort(rng.choice(np.arange(N, dtype=np.int64), size=min(count, N), replace=False))


# (N, how it is run, kernel name the size table must give, bins): "wave" / "block" / "auto" are variants of the device
# entry; "ws0" is the any-size path with no workspace, the DFT by its definition
BIN_SEED = 20
BIN_CASES = (
    [(N, "wave", f"amcx_features18_short_kernel<{N}>", "all") for N in (128, 256, 512)]
    + [(N, "wave", f"amcx_features18_wave_kernel<{N}>", "all") for N in (1024, 2048, 4096)]
    + [(8192, "wave", "amcx_features18_quad_kernel", "all"),
       (2048, "block", "amcx_features18_block_kernel<1>", "all"),
       (16384, "wave", "amcx_features18_group_kernel<8>", "group"),
       (32768, "wave", "amcx_features18_group_kernel<16>", "group")]
    + [(N, "auto", "amcx_features18_block_kernel<0>", "all") for N in (3, 10, 63)]
    + [(64, "auto", "amcx_features18_block_kernel<1>", "all")]
    + [(N, "auto", "amcx_features18_block_kernel<2>", "all") for N in (65, 1000, 4095)]
    + [(4097, "auto", "amcx_features18_block_kernel<3>", "all"),
       (8191, "auto", "amcx_features18_block_kernel<3>", 2048)]
    + [(N, "auto", "amcx_features18_stream_kernel", 1024) for N in (8193, 16385, 32767)]
    + [(8193, "ws0", "amcx_features18_stream_kernel", 64)]
)


def case_bins(N, kind):
    if kind == "all":
        return all_bins(N)
    if kind == "group":
        return group_bins(N, N // 2048)
    return edge_and_seeded_bins(N, int(kind), BIN_SEED)


# ---------------------------------------------------------------------------------------------------------------------
# positions
# ---------------------------------------------------------------------------------------------------------------------
def _triples(stride, lo, hi):
    """p in [lo, hi) with p = -1, 0 or 1 (mod stride)"""
    out = set()
    for m in range(lo - lo % stride, hi + stride, stride):
        out.update(p for p in (m - 1, m, m + 1) if lo <= p < hi)
    return out


def extra_strides(N):
    """Strides of a size's kernel that the common rule of ``seam_positions`` does not hit (see there)."""
    if N > 8192 and N & (N - 1):
        return (1024, 8192, 16384)
    return ()


def seams(N):
    """The structured part of ``seam_positions``: a sorted list."""
    if N <= 512:
        return list(range(N))
    s = set(range(66)) | set(range(N - 66, N))
    if N < 8192:
        s |= _triples(64, 0, N)
    else:
        s |= _triples(2048, 0, N) | _triples(64, 0, 2048) | _triples(64, N - 2048, N)
    for stride in extra_strides(N):
        s |= _triples(stride, 0, N)
    return sorted(s)


def position_parts(N):
    """Into how many parametrised cases a size's positions are cut so that each sends at most MAX_SAMPLES samples through
    the oracle.  One everywhere but at 32768, where the seams alone are 357 frames and 256 fit: two."""
    return -(-len(seams(N)) // (MAX_SAMPLES // N))


def seam_positions(N, seed=0):
    """Sample positions p at which the wrapped phase step's pair (p, p + 1), or the sample itself, crosses a boundary of
    a kernel's data layout; sorted, unique.  N <= 512: every position.  Otherwise

      * the first and the last 66 samples;
      * N < 8192: p = 63, 0, 1 (mod 64) throughout;
      * N >= 8192: p = 2047, 0, 1 (mod 2048) throughout, and p = 63, 0, 1 (mod 64) inside the first and the last 2048;
      * ``extra_strides(N)``: N above 8192 and not a power of two: p = -1, 0, 1 modulo 1024, 8192 and 16384;
      * 64 seeded positions among the rest -- fewer where the 8 M-sample cap of a case (``position_parts``) leaves no
        room: the seeded ones are thinned, the seams never.

    The seams, from the kernels' load code (lane l, row i; a "pair" is two consecutive samples in one lane):

      * amcx_short_kernel_body.h:67-74, load_rows: ``src = iq + f * row_stride + 2 * l``, ``load_pair_nt(src + 32 * (FIRST + j))``
        -- N = 128, 256, 512, sixteen lanes a frame: lane seam every 2 samples, register row and 16-lane group seam
        every 32 (lane 15 of row j -> lane 0 of row j + 1), the prefetched head rows / late tail rows split at 32 kHead.
        32 is no multiple of 64: every position is swept at these sizes.
      * amcx_wave_kernel.h:1029-1036, load_frame: ``src = iq + f * row_stride + 2 * lane``, ``load_pair_nt(src + 128 * i)`` -- N =
        1024, 2048, 4096 (complex64, sc16 and both plan kernels): lane seam every 2, register row seam every 128 (lane 63
        -> lane 0: StatsT::row at :450-455, ``is_last(lane) ? rot : rot_prev``); the frame's last sample has no step (LAST).
      * amcx_quad_kernel.h:362-365, :467-470, :501, ``src = iq + f * row_stride + q * kQuarter + 2 * lane`` + ``128 * i`` (and ``128 * (FIRST + i)``),
        ``nx = iq[... + (q + 1) * kQuarter]`` -- N = 8192: lanes 2, rows 128, WAVE seam every 2048 (the next quarter's
        first sample is fetched for the last step of this one).
      * amcx_group_kernel.h:373-376, :542-545, :561, ``src = iq + f * row_stride + q * kBlock + 2 * lane`` + ``128 * i``, ``nx = iq[... + (q + 1) *
        kBlock]`` -- N = 16384, 32768: lanes 2, rows 128, wave seam every 2048.
      * amcx_block_kernel.h:172, :209, :242, :269, ``for (int n = tid; n < N; n += kBlockThreads)`` -- any N <= 8192 (here 100, 1000, 4097):
        thread seam every sample, wave seam every 64, trip seam every 256 = kBlockThreads.
      * amcx_stream_kernel.h:324, :344, :371, :394, ``for (int n = tid; n < N; n += kThreads)`` (passes A, B, C) -- N > 8192 (here 8193, 16385):
        wave seam every 64, trip seam every 1024 = kThreads, which is no multiple of 2048: added.  ``xs[i] = sample(c0 +
        i)`` (:449) with ``c0 = c * kChunk``: the workspace-free form stages 16384 samples at a time: 16385 is the first size
        of two chunks.  8192 is where the block kernel's range ends: p = 8191, 0, 1 (mod 8192) at 8193 is the tail of
        one sample.

    2, 32 (N <= 512), 64, 128, 256, 1024, 2048, 16384: every seam stride of a kernel divides one that is swept."""
    s = seams(N)
    if N <= 512:
        return np.asarray(s, dtype=np.int64)
    room = position_parts(N) * (MAX_SAMPLES // N) - len(s)
    taken = np.zeros(N, bool)
    taken[s] = True
    rng = np.random.default_rng([int(seed), int(N), 7])
    extra = rng.choice(np.flatnonzero(~taken), size=max(0, min(64, room)), replace=False)
    return np.sort(np.concatenate([np.asarray(s, dtype=np.int64), extra.astype(np.int64)]))


def base_frame(N):
    """The one base frame of a size: 16QAM at 12 dB, seed N, complex64 (N,)."""
    from amcpy_amd import synth
    return synth.host_block("16QAM", 12.0, 1, N, seed=N)[0].astype(np.complex64)


def outlier_frames(base, positions):
    """complex64 (len(positions), N): row i is `base` with sample p_i replaced by 3 base[p_i] exp(2i)."""
    positions = np.asarray(positions, dtype=np.int64)
    x = np.repeat(np.asarray(base, np.complex64)[None, :], len(positions), axis=0)
    rows = np.arange(len(positions))
    x[rows, positions] = (3.0 * base[positions].astype(np.complex128) * np.exp(2.0j)).astype(np.complex64)
    return x


# (N, variant, part): every power of two with "wave", five other sizes with "auto"
POSITION_CASES = [(N, "wave", part) for N in POW2_SIZES for part in range(position_parts(N))] + \
                 [(N, "auto", 0) for N in (100, 1000, 4097, 8193, 16385)]


def case_positions(N, part):
    """The positions of one parametrised case: part `part` of seam_positions(N) cut into position_parts(N) runs."""
    return np.array_split(seam_positions(N), position_parts(N))[part]


def assert_position_parity(got, gold, frames, positions, what):
    """tests/test_gpu_parity.py::_assert_parity, unchanged; when it fails, the message also names the positions."""
    from oracle import iq_features_oracle as orc
    from tests.test_gpu_parity import TOL, _assert_parity
    try:
        _assert_parity(got, gold, frames, what)
    except AssertionError as err:
        plain, scaled = orc.parity_errors(got, np.asarray(gold).astype(np.float32), orc.conditioning_scales(frames))
        strict = [i for i in range(18) if i < 9 or i == 10]
        bad = (scaled > TOL).any(axis=1) | (plain[:, strict] > TOL).any(axis=1)
        pos = np.asarray(positions)[bad]
        ids = sorted({int(j) + 1 for j in np.argwhere(scaled > TOL)[:, 1]} | {strict[int(j)] + 1 for j in np.argwhere(plain[:, strict] > TOL)[:, 1]})
        raise AssertionError(f"{err}\n{what}: {pos.size} of {len(positions)} positions fail, features {ids}: "
                             f"positions {pos[:64].tolist()}") from None
