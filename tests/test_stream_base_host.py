"""The chunk bookkeeping under every streaming class (amcpy_amd/_stream.py, ``Chunked``) on a toy subclass with no taps and no
FFT, and the SNR label the two detectors share (``occupancy.snr_db``).  No GPU."""
import numpy as np
import pytest

from amcpy_amd import _stream, occupancy

WINDOW, HOP = 3, 5


class _Toy(_stream.Chunked):
    """Output m is the sum of the WINDOW = 3 samples from 5 m on: a window shorter than the HOP = 5 it moves by, so the next
    window begins beyond the data a push completes and the skip path runs.  (A toy whose outputs are ``S // 3`` of
    ``buf[0:3 M:3]`` while each consumes 5 samples is no operation on a stream -- one call spaces its outputs 3 apart, two
    calls 5 apart -- so no bookkeeping could make its pushes equal one call; this is the nearest one that is.)"""
    _NOUN = "toy"

    def __init__(self):
        super().__init__("cf32", None)

    def _outputs(self, S):
        return 0 if S < WINDOW else (S - WINDOW) // HOP + 1

    def _consumed(self, M):
        return HOP * M

    def _run(self, buf, M):
        return sum(buf[k:k + HOP * M:HOP][:M] for k in range(WINDOW))


def test_chunked_pushes_equal_one_call_and_the_state_has_its_closed_form():
    S = 200
    x = np.arange(S).astype(np.complex64)
    whole = _Toy().push(x)
    M = (S - WINDOW) // HOP + 1
    assert whole.dtype == np.complex64 and np.array_equal(whole, WINDOW * HOP * np.arange(M) + 3)      # 0 + 1 + 2, 5 + 6 + 7, ...
    primes = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37]
    for name, sizes in {"ones": [1] * S, "primes": primes * 2, "one piece": [S], "an empty push between": [4, 0, 1, 0, S]}.items():
        toy, got, at = _Toy(), [], 0
        assert toy.index == 0 and toy._skip == 0 and toy._tail is None
        for n in sizes:
            got.append(toy.push(x[at:at + n]))
            at = min(S, at + n)
            done = 0 if at < WINDOW else (at - WINDOW) // HOP + 1
            assert toy.index == HOP * done, (name, at)
            assert toy._skip == max(0, HOP * done - at) and toy._tail.shape[0] == max(0, at - HOP * done), (name, at)
            assert not np.shares_memory(toy._tail, x)                        # a copy: the tail keeps no chunk alive
        assert at == S and np.array_equal(np.concatenate(got), whole), name
    with pytest.raises(TypeError, match="^this toy takes cf32 chunks$"):
        _Toy().push(np.zeros((4, 2), np.int16))


def _grid():
    power = np.array([[4.0, 0.5, 3.0, np.inf], [1.0, 2.0, 0.0, 7.0], [np.nan, 1e-30, 1e30, 2.0]], np.float32)      # (3, 4)
    return power, np.array([1.0, 2.0, 0.0, 2.0], np.float32), np.array([1.0, 0.0, np.nan], np.float32)


def _literal(power, floor):
    with np.errstate(all="ignore"):
        return (10.0 * np.log10(np.maximum(power / floor - np.float32(1.0), np.finfo(np.float32).tiny))).astype(np.float32)


def test_snr_db_is_the_literal_expression_in_numpy():
    power, per_col, per_row = _grid()
    got = occupancy.snr_db(power, per_col, 1)
    assert got.dtype == np.float32 and np.array_equal(got, _literal(power, per_col[None, :]), equal_nan=True)
    # what the grid holds: a cell below its floor (clamped to tiny), a floor of 0 under a power (inf) and under 0 (NaN), inf, NaN
    tiny_db = np.float32(10.0) * np.log10(np.finfo(np.float32).tiny)
    assert got[0, 1] == tiny_db and got[1, 0] == tiny_db and np.isposinf(got[0, 2]) and np.isnan(got[1, 2]) and np.isposinf(got[0, 3])
    assert np.isnan(got[2, 0]) and abs(got[0, 0] - 10.0 * np.log10(3.0)) < 1e-5
    got = occupancy.snr_db(power, per_row, 0)
    assert got.dtype == np.float32 and np.array_equal(got, _literal(power, per_row[:, None]), equal_nan=True)


def test_snr_db_on_a_torch_tensor_agrees_with_numpy_to_one_ulp():
    """torch's and numpy's log10 are different libms: the finite cells agree to 1 ulp of float32, the others exactly."""
    import torch
    power, per_col, per_row = _grid()
    for floor, axis in ((per_col, 1), (per_row, 0)):
        want = occupancy.snr_db(power, floor, axis)
        got = occupancy.snr_db(torch.from_numpy(power), torch.from_numpy(floor), axis)
        assert got.dtype == torch.float32 and tuple(got.shape) == power.shape
        got = got.numpy()
        finite = np.isfinite(want)
        assert np.array_equal(got[~finite], want[~finite], equal_nan=True)
        ulps = np.abs(got[finite].view(np.int32).astype(np.int64) - want[finite].view(np.int32).astype(np.int64))
        print("snr_db, torch against numpy, axis", axis, "worst difference in ulps:", int(ulps.max()))
        assert ulps.max() <= 1
