"""The Welch spectrogram of a raw stream in GPU memory and the emitters in it (include/amcx.h, ABI 15): where the signals of an
unknown band are, in time and frequency, with no channel raster.

    P = spectrogram(x, 1024, averages=16)              # (R, 1024) float32: sums of A = 16 windowed periodograms, hop nfft / 2
    det = detect(P)                                    # floor per row, mask of occupied bins, SNR per cell
    emitters(det.mask.cpu().numpy())                   # [(first_row, last_row, lo_bin, hi_bin), ...] in signed bins

Segment s begins at sample ``s * hop``; row r sums the segments ``r A ... r A + A - 1``: it covers the ``(A - 1) hop + nfft``
samples from ``r A hop`` on.  Nothing is normalised: :func:`power_scale` is the factor ``1 / (A sum w^2)`` that turns a row
into a power per bin; the detection is free of scale.

WHAT THE DETECTOR ASSUMES.  The floor of row r is a RANK STATISTIC across that row's bins: the element of rank
``int(floor_quantile * (nfft - 1))`` (ascending, NaN last).  It is the noise floor only where at least that many bins of every
row are free.  A bin is occupied where its power exceeds ``threshold`` times that floor (one float32 product, one comparison).
Nothing is smoothed over time: with few averages a row's noise bins scatter widely (A = 4 gives false bands at 6 dB).

Every call is one C-ABI entry on the current torch stream and synchronises nothing.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _formats, _lib, _stream
from .occupancy import floor_rank_of, snr_db, threshold_of

WINDOWS = ("hann", "rect")
Detection = namedtuple("Detection", "floor mask snr_db")
Detection.__doc__ = """``floor`` (R,) float32, ``mask`` (R, nfft) bool, ``snr_db`` (R, nfft) float32."""


def window(nfft: int, kind: str = "hann") -> np.ndarray:
    """``nfft`` float32 window values: ``"hann"`` is the periodic Hann window ``0.5 - 0.5 cos(2 pi n / nfft)`` (computed in
    float64, rounded once), ``"rect"`` all ones."""
    n = int(nfft)
    if n < 1:
        raise ValueError("nfft must be at least 1")
    if kind == "rect":
        return np.ones((n,), np.float32)
    if kind == "hann":
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)).astype(np.float32)
    raise ValueError(f"window must be one of {WINDOWS}, not {kind!r}")


def out_rows(n_samples: int, nfft: int, hop: int, averages: int = 1) -> int:
    """amcx_spectrogram_out_rows: ``floor(nseg / A)`` with ``nseg = floor((S - nfft) / hop) + 1`` (0 below nfft samples).
    ValueError outside the kernel's limits: nfft a power of two 64 ... 4096, hop and averages 1 ... 65536, S < 2^40."""
    ints = [int(n_samples), int(nfft), int(hop), int(averages)]
    if not (-(1 << 63) <= ints[0] < (1 << 63)) or any(not (-(1 << 31) <= v < (1 << 31)) for v in ints[1:]):
        raise ValueError("argument outside the C interface's integer range")
    R = _lib.load().amcx_spectrogram_out_rows(*ints)
    if R < 0:
        raise ValueError(f"S = {n_samples}, nfft = {nfft}, hop = {hop}, averages = {averages} is outside the kernel's limits: "
                         "nfft a power of two 64 ... 4096, hop and averages 1 ... 65536, 0 <= S < 2^40")
    return int(R)


def row_samples(nfft: int, hop: int, averages: int = 1) -> int:
    """``(A - 1) hop + nfft``: the samples one row covers."""
    return (int(averages) - 1) * int(hop) + int(nfft)


def power_scale(window, averages: int = 1) -> float:
    """``1 / (A sum w^2)`` in float64: a row times it is the mean power per bin of a unit-gain periodogram."""
    w = np.asarray(window, dtype=np.float64)
    return 1.0 / (int(averages) * float(np.sum(w * w)))


def bin_frequencies(nfft: int, sample_rate: float = 1.0, center: float = 0.0) -> np.ndarray:
    """The frequency of every bin, float64 ``(nfft,)`` in FFT order, as ``bank.channel_frequencies``: ``b / nfft`` taken into
    [-0.5, 0.5) cycles per sample (bin nfft / 2 is -0.5), times ``sample_rate``, plus ``center``."""
    n = int(nfft)
    b = np.arange(n, dtype=np.float64)
    return float(center) + float(sample_rate) * (np.where(b < n / 2.0, b, b - n) / n)


def _window_of(win, nfft: int, device=None):
    """The window as float32 numpy ``(nfft,)`` (a name, None for Hann, or values), or a torch tensor as given."""
    if win is None or isinstance(win, str):
        return window(nfft, win or "hann")
    if device is not None:
        import torch
        if isinstance(win, torch.Tensor):
            if win.dtype != torch.float32 or win.dim() != 1 or int(win.shape[0]) != nfft or win.device != device:
                raise TypeError("window must be a one-dimensional float32 tensor of nfft values on x's device")
            return win.contiguous()
    w = np.ascontiguousarray(np.asarray(win, dtype=np.float32))
    if w.shape != (nfft,):
        raise ValueError(f"window must hold nfft = {nfft} values, got shape {w.shape}")
    return w


def spectrogram(x, nfft: int, *, hop=None, averages: int = 1, window=None, scale=None, out=None):
    """The spectrogram of a stream in GPU memory: one launch of amcx_spectrogram on the current torch stream.

    ``x``: complex64 ``(S,)`` or int16 / int8 / uint8 ``(S, 2)`` (sc16 / ci8 / cu8: a component is the integer times ``scale``,
    default the format's), contiguous; a view that begins at any sample is fine.  ``hop``: None for ``nfft // 2``.  ``window``:
    None or a name of :func:`window`, or nfft float32 values (numpy, or a tensor on x's device).  ``out``: float32 ``(>= R,
    >= nfft)`` on x's device with contiguous rows; only the R rows' nfft columns are written.  Returns float32 ``(R, nfft)``
    (a view of ``out`` where given), ``R = out_rows(S, nfft, hop, averages)``, in FFT order (:func:`bin_frequencies`)."""
    import torch

    _, kind, scale, S = _stream.source(x, scale)
    nfft = int(nfft)
    hop = nfft // 2 if hop is None else int(hop)
    A = int(averages)
    R = out_rows(S, nfft, hop, A)
    w = _window_of(window, nfft, x.device)
    if not isinstance(w, torch.Tensor):
        w = torch.from_numpy(w).to(x.device)
    if out is None:
        out, stride = torch.empty((R, nfft), dtype=torch.float32, device=x.device), nfft
    else:
        holds = f"out must hold {R} contiguous rows of {nfft} bins"
        _, _, stride = _stream.rows_of(out, torch.float32, "out", "bins", nfft, used=nfft, min_rows=R, device=x.device,
                                       kind="out must be a two-dimensional float32 tensor on x's device", narrow=holds, layout=holds)
    _stream.launch(x, lambda lib, stream: lib.amcx_spectrogram(
        x.data_ptr() if R else None, kind, S, scale, w.data_ptr(), nfft, hop, A, out.data_ptr() if R else None, stride, R, stream))
    return out[:R, :nfft]


class Spectrogram(_stream.Chunked):
    """The spectrogram of a stream that arrives in chunks: ``push(chunk)`` returns the rows the chunk completes, float32
    ``(r, nfft)``, possibly none.  The rows are those of one :func:`spectrogram` call over the whole stream, bit for bit,
    wherever the chunks are cut: a row's bits depend on its own samples alone, so the class only has to keep the samples no
    row has consumed yet (``held`` of them; with ``A hop`` beyond a row's span, the gap's samples are dropped as they come).

    ``rows_done`` counts the rows returned so far and ``index = rows_done * A * hop`` is the stream's sample index at which
    the next row begins.  ``compute(buf, nfft, hop=, averages=, window=, scale=)``: an injected numpy implementation (host
    tests); chunks are then numpy arrays."""

    _NOUN = "spectrogram"

    def __init__(self, nfft: int, hop=None, averages: int = 1, window=None, fmt: str = "cf32", scale=None, compute=None):
        super().__init__(fmt, compute)
        self.nfft = int(nfft)
        self.hop = self.nfft // 2 if hop is None else int(hop)
        self.averages = int(averages)
        out_rows(0, self.nfft, self.hop, self.averages)                 # ValueError outside the kernel's limits
        self.window = _window_of(window, self.nfft)
        self.scale = _formats.scale_of(fmt, scale)
        self.row_samples = row_samples(self.nfft, self.hop, self.averages)
        self._window_dev = None

    @property
    def rows_done(self) -> int:
        return self.index // (self.averages * self.hop)

    @property
    def held(self) -> int:
        """The samples that have arrived and belong to rows not yet complete."""
        return 0 if self._tail is None else int(self._tail.shape[0])

    def _outputs(self, S: int) -> int:
        return out_rows(S, self.nfft, self.hop, self.averages)

    def _consumed(self, R: int) -> int:
        return R * self.averages * self.hop                          # where the next row begins

    def _run(self, buf, R):
        kw = dict(hop=self.hop, averages=self.averages, scale=self.scale)
        if self._compute is not None:
            return self._compute(buf, self.nfft, window=self.window, **kw)
        import torch
        if self._window_dev is None or self._window_dev.device != buf.device:
            self._window_dev = torch.from_numpy(self.window).to(buf.device)
        return spectrogram(buf, self.nfft, window=self._window_dev, **kw)


def detect(P, *, floor_quantile: float = 0.25, threshold_db: float = 6.0) -> Detection:
    """``P``: float32 ``(R, bins)`` on the GPU, contiguous rows at a row stride >= bins, 2 <= bins <= 4096 ->
    :class:`Detection` (the module's docstring says what the detector assumes): one launch of amcx_psd_detect_f32.  Rank and
    threshold are :func:`amcpy_amd.occupancy.floor_rank_of` / ``threshold_of``'s.  ``snr_db`` is
    :func:`amcpy_amd.occupancy.snr_db` of every cell over its row's floor, computed with torch: a label for the user, no part
    of the detection."""
    import torch

    R, bins, stride = _stream.rows_of(P, torch.float32, "P", "bins", 2, 4096, narrow="rows of 2 ... 4096 bins, got {}")
    rank, thr = floor_rank_of(bins, floor_quantile), threshold_of(threshold_db)
    floor = torch.empty((R,), dtype=torch.float32, device=P.device)
    mask = torch.empty((R, bins), dtype=torch.uint8, device=P.device)
    _stream.launch(P, lambda lib, stream: lib.amcx_psd_detect_f32(
        P.data_ptr() if R else None, R, bins, stride, rank, float(thr), floor.data_ptr() if R else None,
        mask.data_ptr() if R else None, stream))
    return Detection(floor, mask.bool(), snr_db(P, floor, 0))


def bands(mask_row, min_bins: int = 2, merge_bins: int = 2) -> list:
    """The occupied bands of one row: ``mask_row`` (nfft,) bool in FFT order -> ``[(lo_bin, hi_bin), ...]`` in SIGNED bins
    (-nfft / 2 ... nfft / 2 - 1, both ends inclusive), ascending.  Host side.

    The row is looked at in ``fftshift`` order, -1/2 ... 1/2 (a run across DC is one run; a run at +1/2 does NOT wrap to -1/2).
    Runs of occupied bins separated by at most ``merge_bins`` free bins are joined first; runs that are then shorter than
    ``min_bins`` are dropped."""
    m = np.asarray(mask_row).astype(bool)
    if m.ndim != 1:
        raise ValueError("mask_row must be (nfft,)")
    n = int(m.shape[0])
    half = n // 2
    s = np.fft.fftshift(m)                                            # index i is the signed bin i - half
    edge = np.diff(np.concatenate(([0], s.astype(np.int8), [0])))
    first, past = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    runs = []
    for a, b in zip(first.tolist(), past.tolist()):                   # [a, b)
        if runs and a - runs[-1][1] <= int(merge_bins):
            runs[-1][1] = b
        else:
            runs.append([a, b])
    return [(a - half, b - 1 - half) for a, b in runs if b - a >= int(min_bins)]


def emitters(mask, min_bins: int = 2, merge_bins: int = 2, min_rows: int = 1) -> list:
    """The emitters of a mask: ``mask`` (R, nfft) bool in FFT order (numpy, or anything ``numpy.asarray`` takes) ->
    ``[(first_row, last_row, lo_bin, hi_bin), ...]``, rows and signed bins inclusive, sorted by ``(first_row, lo_bin)``.  Host side.

    Every row is cut into :func:`bands`.  Two bands of CONSECUTIVE rows belong together where their bin ranges overlap (share
    at least one bin); an emitter is a connected component of that relation -- a band that splits in the next row, or two
    that join, stay one emitter -- with the first and last row of its bands and the union of their edges (the smallest lo,
    the largest hi).  Emitters of fewer than ``min_rows`` rows are dropped."""
    m = np.asarray(mask).astype(bool)
    if m.ndim != 2:
        raise ValueError("mask must be (R, nfft)")
    parent, box = [], []                                              # union-find over bands; [first_row, last_row, lo, hi] per root

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    prev = []                                                         # (band id, lo, hi) of the row above
    for r in range(m.shape[0]):
        cur = []
        for lo, hi in bands(m[r], min_bins, merge_bins):
            i = len(parent)
            parent.append(i)
            box.append([r, r, lo, hi])
            for j, plo, phi in prev:
                if plo <= hi and lo <= phi:
                    a, b = find(i), find(j)
                    if a != b:
                        parent[a] = b
                        box[b] = [min(box[a][0], box[b][0]), max(box[a][1], box[b][1]), min(box[a][2], box[b][2]),
                                  max(box[a][3], box[b][3])]
            cur.append((i, lo, hi))
        prev = cur
    out = [tuple(box[i]) for i in range(len(parent)) if parent[i] == i and box[i][1] - box[i][0] + 1 >= int(min_rows)]
    return sorted(out, key=lambda e: (e[0], e[2]))
