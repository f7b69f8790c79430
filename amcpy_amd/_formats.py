"""The sample formats the library reads, each fact once: what a stored sample is, which ``AMCX_SRC_*`` kind and ``AMCX_IQ8_*``
argument the C entries take for it, its default scale and zero level, and what SigMF calls it.  Private, and free of torch:
:mod:`features`, :mod:`_stream`, :mod:`sigmf`, :mod:`frame_sources` and :mod:`feature_extraction` look everything up here."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _lib

# one stored integer sample as numpy sees it: I then Q (include/amcx.h, amcx_features_sc16 / amcx_features_iq8)
SC16 = np.dtype([("i", "<i2"), ("q", "<i2")])
CI8 = np.dtype([("i", "i1"), ("q", "i1")])
CU8 = np.dtype([("i", "u1"), ("q", "u1")])


class Format(NamedTuple):
    name: str
    kind: int                   # _lib.SRC_*
    iq8: Optional[int]          # _lib.IQ8_*: the format argument of the 8-bit entries
    plain: np.dtype             # one component (cf32: the whole sample) ...
    tail: tuple                 # ... and the trailing shape of one sample in an array of them: () or (2,)
    store: np.dtype             # one stored sample; its itemsize is the bytes per sample
    scale: float                # what an integer component is multiplied by unless the caller says otherwise
    zero: int                   # the integer that stands for 0.0
    sigmf: str                  # core:datatype

    @property
    def family(self) -> Optional[str]:
        """Which of the library's integer entries and context scales serve it -- "sc16" (amcx_features_sc16,
        amcx_ctx_set_sc16_scale, ...) or "iq8" -- or None: complex64 has no scale."""
        return None if self.name == "cf32" else "sc16" if self.iq8 is None else "iq8"


TABLE = (
    Format("cf32", _lib.SRC_C64, None, np.dtype("<c8"), (), np.dtype(np.complex64), 1.0, 0, "cf32_le"),
    Format("sc16", _lib.SRC_SC16, None, np.dtype("<i2"), (2,), SC16, _lib.SC16_SCALE, 0, "ci16_le"),
    Format("ci8", _lib.SRC_CI8, _lib.IQ8_CI8, np.dtype("i1"), (2,), CI8, _lib.IQ8_SCALE, 0, "ci8"),
    Format("cu8", _lib.SRC_CU8, _lib.IQ8_CU8, np.dtype("u1"), (2,), CU8, _lib.IQ8_SCALE, 128, "cu8"),
)
NAMES = tuple(f.name for f in TABLE)
_BY_NAME = {f.name: f for f in TABLE}
_BY_PLAIN = {f.plain.name: f for f in TABLE}
# columns of the table by format name, for callers that index one (``ddc`` re-exports them: the benchmark tools read them there)
_KINDS = {f.name: f.kind for f in TABLE}
_DEFAULT_SCALE = {f.name: f.scale for f in TABLE}
_NUMPY = {f.name: f.plain.type for f in TABLE}


def get(name: str) -> Format:
    return _BY_NAME[name]


def by_store(dtype) -> Optional[Format]:
    """The format whose stored sample is ``dtype`` (complex64, ``SC16``, ``CI8``, ``CU8``), or None."""
    return next((f for f in TABLE if f.store == dtype), None)


def by_plain(dtype) -> Optional[Format]:
    """The format whose component is the numpy or torch ``dtype`` (complex64, int16, int8, uint8), or None."""
    return _BY_PLAIN.get(str(dtype).replace("torch.", ""))


def check_scale(scale) -> float:
    """``scale`` as the float32 the library multiplies an integer component by; ValueError unless it is finite and > 0."""
    s = float(np.float32(scale))
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError(f"scale must be a finite float32 > 0, got {scale!r}")
    return s


def scale_of(fmt: str, scale=None) -> float:
    """:func:`check_scale`, or the format's default for None.  cf32 has no scale: whatever is passed is not read."""
    return get(fmt).scale if scale is None or fmt == "cf32" else check_scale(scale)


def scale_kw(fmt: str, scale, sc16: str = "sc16_scale", iq8: str = "iq8_scale") -> dict:
    """The one keyword that carries ``scale`` for ``fmt`` where an interface has a keyword per family (``HipEngine``; with
    ``sc16="scale", iq8="scale8"``: ``extract_raw_stream``): {} for None or cf32, so the callee's default stands."""
    family = get(fmt).family
    return {} if scale is None or family is None else {sc16 if family == "sc16" else iq8: scale}


def sc16_view(pairs: np.ndarray) -> np.ndarray:
    """(..., L, 2) int16 -> (..., L) view of :data:`SC16` samples (no copy).  TypeError for another dtype or a last
    dimension that is not 2, ValueError for pairs that are not interleaved in memory."""
    if not isinstance(pairs, np.ndarray) or pairs.dtype != np.int16 or pairs.ndim < 2 or pairs.shape[-1] != 2:
        raise TypeError("expected an int16 array whose last dimension is (I, Q)")
    if pairs.strides[-1] != 2 or any(st % 4 for st in pairs.strides[:-1]):
        raise ValueError("(I, Q) int16 pairs must be interleaved in memory")
    return pairs.view(SC16)[..., 0]


def iq8_view(pairs: np.ndarray) -> np.ndarray:
    """(..., L, 2) int8 / uint8 -> (..., L) view of :data:`CI8` / :data:`CU8` samples (no copy).  TypeError for another
    dtype or a last dimension that is not 2, ValueError for pairs that are not interleaved in memory."""
    fmt = by_plain(pairs.dtype) if isinstance(pairs, np.ndarray) else None
    if fmt is None or fmt.family != "iq8" or pairs.ndim < 2 or pairs.shape[-1] != 2:
        raise TypeError("expected an int8 or uint8 array whose last dimension is (I, Q)")
    if pairs.strides[-1] != 1 or any(st % 2 for st in pairs.strides[:-1]) or (pairs.shape[-2] > 1 and pairs.strides[-2] != 2):
        raise ValueError("(I, Q) byte pairs must be interleaved in memory")
    return pairs.view(fmt.store)[..., 0]
