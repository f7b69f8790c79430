"""References for occupancy detection (include/amcx.h, ABI 14; amcpy_amd/csrc/amcx_occupancy_kernels.h): the row power in
float64 and its error bound, the detection in exact numpy float32, a numpy row power, the injected compute
amcpy_amd.sigmf.survey_sigmf takes, and the synthetic raster the end-to-end tests survey.  No GPU, no torch.

THE BOUND.  power[r] is a sum of 2 N non-negative terms re^2, im^2.  The kernel's order (its header): a lane folds its sample
pairs into one accumulator, s = fma(im, im, fma(re, re, s)) -- ONE rounding per term, the square is exact inside the fma --
so a lane that holds P pairs has rounded 4 P times, P <= ceil(ceil(N / 2) / 64) = ceil(N / 128); the 6-level tree over the 64
lanes rounds 6 more times.  The longest path from any term to the result therefore passes B0 = 4 ceil(N / 128) + 6 roundings,
each of relative size u = 2^-24 at the most.  Every partial sum is a sum of non-negative numbers, so each is at most the
exact total p64 times the growth so far, and the first-order error of the result is at most B0 u p64.  The two spare
units, B = B0 + 2 = 4 ceil(N / 128) + 8, take up the second-order terms ((1 + u)^B0 - 1 - B0 u < 2 u for every N the
library takes: B0 <= 1030, B0^2 u / 2 < 0.04) and the rounding of the float64 reference itself (2 N 2^-53, far below u).
"""
import numpy as np

U = 2.0 ** -24


def bound_factor(N: int) -> int:
    """B = 4 ceil(N / 128) + 8 (the module's docstring derives it)."""
    return 4 * (-(-int(N) // 128)) + 8


def power64(frames) -> np.ndarray:
    """sum_n re^2 + im^2 of every row in float64 (pairwise: its own error is negligible beside float32's)."""
    x = np.asarray(frames)
    return (x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2).sum(axis=-1)


def worst_ratio(p, p64, N: int) -> float:
    """max over rows of |p - p64| / (B 2^-24 p64): the criterion holds iff <= 1 (a row of zeros must give exactly 0)."""
    p64 = np.asarray(p64, dtype=np.float64)
    err = np.abs(np.asarray(p).astype(np.float64) - p64)
    bound = bound_factor(N) * U * p64
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


def numpy_row_power(frames) -> np.ndarray:
    """A float32 row power in numpy: the float64 sum, rounded once (within half a unit of the exact value: inside the bound)."""
    return power64(frames).astype(np.float32)


def _nan_last(power):
    """The values with NaN mapped to what sorts last: np.partition orders NaN last already; +inf < NaN is kept by it."""
    return np.asarray(power, dtype=np.float32)


def numpy_detect(power, floor_rank: int, threshold):
    """Exact float32: power (C, K) -> (floor (K,), mask (C, K) bool, rows ascending int32).  The floor is the element of rank
    ``floor_rank`` (ascending, NaN last: numpy's sort order) of every column; the mask is ONE float32 product and one `>`."""
    p = _nan_last(power)
    C, K = p.shape
    if K == 0:
        return np.empty((0,), np.float32), np.zeros((C, 0), bool), np.empty((0,), np.int32)
    floor = np.partition(p, int(floor_rank), axis=0)[int(floor_rank)].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        limit = (np.float32(threshold) * floor).astype(np.float32)
        mask = p > limit[None, :]
    return floor, mask, np.flatnonzero(mask.reshape(-1)).astype(np.int32)


def brute_detect(power, floor_rank: int, threshold):
    """The same by a full sort per frame in Python (NaN last by an explicit key), for tests of numpy_detect itself."""
    p = np.asarray(power, dtype=np.float32)
    C, K = p.shape
    floor = np.empty((K,), np.float32)
    for k in range(K):
        col = sorted(p[:, k].tolist(), key=lambda v: (v != v, v if v == v else 0.0))
        floor[k] = np.float32(col[int(floor_rank)])
    mask = np.zeros((C, K), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            for k in range(K):
                mask[c, k] = bool(p[c, k] > np.float32(np.float32(threshold) * floor[k]))
    rows = np.array([c * K + k for c in range(C) for k in range(K) if mask[c, k]], dtype=np.int32)
    return floor, mask, rows


def numpy_occupancy(frames, C, K, floor_rank, threshold):
    """The ``occupancy_compute`` amcpy_amd.sigmf.survey_sigmf takes: frames (C K, N) -> (power (C, K), floor, mask)."""
    power = numpy_row_power(frames).reshape(C, K)
    floor, mask, _ = numpy_detect(power, floor_rank, threshold)
    return power, floor, mask


# ---- the synthetic raster ---------------------------------------------------------------------------------------------------
def raster(C: int, N: int, n_frames: int, oversample: int, seed: int, burst=(6, 15), emitters=(2, 5), snr_db: float = 20.0,
           taps_per_channel: int = 16):
    """A wideband stream for the end-to-end tests -> (x complex64 (S,), burst frames (first, last)).

    Unit-power complex white noise plus two band-limited emitters: QPSK at fs / (2 C) symbols per sample through
    windowed_sinc(32 C + 1, 0.3 / C), each ``snr_db`` above the noise that falls into one channel (1 / C of the noise power),
    centred on the channels ``emitters``.  The first is on throughout; the second is switched on for the input samples of
    the frames burst[0] ... burst[1] only (whole frames of the bank's output: frame k covers input samples k N D ...)."""
    from amcpy_amd._stream import windowed_sinc
    rng = np.random.default_rng(seed)
    D = C // oversample
    T = C * taps_per_channel
    S = n_frames * N * D + T + 4 * C
    x = (rng.standard_normal(S) + 1j * rng.standard_normal(S)) / np.sqrt(2.0)
    sps = 2 * C
    h = windowed_sinc(32 * C + 1, 0.3 / C).astype(np.float64)
    n = np.arange(S)
    for j, ch in enumerate(emitters):
        sym = (rng.integers(0, 2, S // sps + 2) * 2 - 1 + 1j * (rng.integers(0, 2, S // sps + 2) * 2 - 1)) / np.sqrt(2.0)
        up = np.zeros(S + len(h), np.complex128)
        up[::sps][:len(sym)] = sym[:len(up[::sps])]
        base = np.convolve(up, h)[len(h) // 2:len(h) // 2 + S]
        base *= np.sqrt((10.0 ** (snr_db / 10.0) / C) / np.mean(np.abs(base) ** 2))
        if j == 1:
            # on for frames burst[0] ... burst[1]: a frame's window of input is [k N D, k N D + N D + T)
            gate = np.zeros(S)
            gate[burst[0] * N * D + T // 2:(burst[1] + 1) * N * D + T // 2] = 1.0
            base = base * gate
        x += base * np.exp(2j * np.pi * ch / C * n)
    return x.astype(np.complex64), burst


def write_sigmf(tmp_path, x, datatype: str, sample_rate: float = 1.0e6, frequency: float = 100.0e6, name: str = "raster"):
    """x complex64 -> a one-capture SigMF recording under tmp_path in cf32_le or ci16_le (scaled to use the int16 range
    without clipping) -> (stem, what the recording holds as complex64 after the reader's default scale)."""
    import json
    from pathlib import Path
    stem = tmp_path / name
    if datatype == "cf32_le":
        blob, held = x.astype(np.complex64).tobytes(), x.astype(np.complex64)
    else:
        peak = float(max(np.abs(x.real).max(), np.abs(x.imag).max()))
        q = np.round(np.stack([x.real, x.imag], axis=-1) * (32000.0 / peak)).astype(np.int16)
        blob = q.tobytes()
        held = ((q[:, 0].astype(np.float32) * np.float32(2.0 ** -15)) + 1j * (q[:, 1].astype(np.float32) * np.float32(2.0 ** -15))).astype(np.complex64)
    Path(str(stem) + ".sigmf-data").write_bytes(blob)
    Path(str(stem) + ".sigmf-meta").write_text(json.dumps({
        "global": {"core:datatype": datatype, "core:version": "1.0.0", "core:sample_rate": sample_rate},
        "captures": [{"core:sample_start": 0, "core:frequency": frequency}], "annotations": []}))
    return stem, held
