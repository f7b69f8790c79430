"""The input streams of the down-converter, filter-bank and resampler tests: random samples of every format over its whole
range, made once per (format, length, seed) and never written to.  ``base`` is the constant that keeps the test modules'
streams apart (tests/test_formats_host.py holds digests of what each module has always seen)."""
import ctypes
import functools

import numpy as np

from amcpy_amd import _formats
from tests import ddc_ref


def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    return torch


def aligned(n_floats=256):
    """``(buffer, address)``: host memory for the refusal tests of the C entries, the address aligned to 16 bytes; keep the buffer"""
    buf = (ctypes.c_float * n_floats)()
    p = ctypes.addressof(buf)
    return buf, p + (-p % 16)


def stream(fmt, n, rng):
    """n samples of a format drawn from ``rng``: complex64 (n,) or integers (n, 2) over their whole range"""
    if fmt == "cf32":
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    plain = _formats.get(fmt).plain
    info = np.iinfo(plain)
    return rng.integers(info.min, info.max + 1, (n, 2)).astype(plain)


@functools.lru_cache(maxsize=None)
def host(fmt, n, seed, base):
    """:func:`stream` at the seed of (base, seed, format), read-only"""
    x = stream(fmt, n, np.random.default_rng(base + seed + 7 * _formats.NAMES.index(fmt)))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def dev(fmt, n, seed, base):
    """the same samples in GPU memory, uploaded once"""
    return torch().from_numpy(np.array(host(fmt, n, seed, base))).cuda()


@functools.lru_cache(maxsize=None)
def wide(fmt, n, seed, base):
    """the same samples as the complex128 the references take, at the format's default scale"""
    return ddc_ref.widen(host(fmt, n, seed, base), fmt, _formats.get(fmt).scale)


@functools.lru_cache(maxsize=None)
def taps_dev(T, seed=0):
    return torch().from_numpy(ddc_ref.make_taps(T, seed)).cuda()


def bind(base, pool):
    """``(host, dev, wide)`` of one test module: its ``base``, and ``pool`` samples where a test names no length"""
    def of(f):
        return lambda fmt, n=pool, seed=0: f(fmt, n, seed, base)
    return of(host), of(dev), of(wide)
