"""The waveform generator: labelled IQ made where it is used (amcx_synth_c64, include/amcx.h ABI 16.2).

One launch writes rows of linearly modulated signal -- symbols of a constellation drawn by Philox4x32-10, a pulse at
``U / V`` samples per symbol, a carrier with a random phase and a bounded random offset, a random timing offset, white Gaussian
noise -- as complex64 in GPU memory.  Every random integer is fixed by the header's contract: a row is named by its ABSOLUTE
index and a sample by its absolute index in the row, so a data set made in any number of calls, or a stream made in chunks of
any length, equals one call bit for bit, and tests/synth_ref.py restates it in numpy.

    design_rrc / design_rect     pulses with sum g^2 = U: unit signal power with a unit-power table, SNR = 1 / sigma^2
    CpmPulse, design_cpfsk / design_gfsk / design_gmsk   phase pulses of the continuous-phase names "MSK", "GMSK", "2FSK", "4FSK", ...
                                 (amcx_synth_cpm_c64, ABI 16.2.2): exp(j Phi[n]), Phi an exact integer sum over every symbol so far
    constellation_table          :func:`amcpy_amd.synth.constellation`'s points as complex64 (WGN: none -- the noise class)
    generate                     one launch: (n_rows, row_samples) complex64
    dataset / dataset_features   the reference's container layout, mod -> (n_snr, n_frames, frame_size) or (..., 18)
    Stream                       one row, ``push(n)`` the next n samples
    scene                        emitters at known frequencies, rates and times on a noise floor, with the ground truth
    run_synth                    the `synth` command: mat-data/all_modulations.mat, or calculated-features/ directly

:mod:`amcpy_amd.synth` stays what it is: the benchmark's and the fixtures' generator, whose numbers they depend on.
"""
from __future__ import annotations

import json
import math
import re
from fractions import Fraction

import numpy as np

from . import _lib, _stream, synth

MAX_TAPS, MAX_UP, MAX_DOWN, MAX_ORDER = 4096, 256, 4096, 256
_MASK64 = (1 << 64) - 1
FRAME_BITS, SNR_BITS = 32, 16          # dataset's rows: (modulation code << 48) | (SNR code << 32) | frame
_tensor = lambda t: hasattr(t, "data_ptr")                                 # noqa: E731  (a torch tensor, without importing torch)


def design_rect(U: int) -> np.ndarray:
    """The rectangular pulse of one symbol: U ones (sum g^2 = U)."""
    U = int(U)
    if not 1 <= U <= MAX_UP:
        raise ValueError(f"design_rect: U {U} is outside 1 ... {MAX_UP}")
    return np.ones(U, np.float32)


def design_rrc(U: int, span_symbols: int = 16, beta: float = 0.35) -> np.ndarray:
    """A root-raised-cosine pulse at U samples per symbol over ``span_symbols`` symbols: ``span_symbols * U + 1`` float32 taps,
    symmetric, computed in float64 and normalised to sum g^2 = U before the rounding.  ValueError where the taps pass 4096."""
    U, span, beta = int(U), int(span_symbols), float(beta)
    if not 1 <= U <= MAX_UP or span < 1 or not 0.0 < beta <= 1.0:
        raise ValueError(f"design_rrc: U {U} (1 ... {MAX_UP}), span_symbols {span} (>= 1), beta {beta} (0 < beta <= 1)")
    T = span * U + 1
    if T > MAX_TAPS:
        raise ValueError(f"design_rrc: {span} symbols at {U} samples per symbol are {T} taps, more than {MAX_TAPS}")
    t = (np.arange(T, dtype=np.float64) - (T - 1) / 2.0) / U
    g = np.empty(T, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        num = np.sin(np.pi * t * (1 - beta)) + 4 * beta * t * np.cos(np.pi * t * (1 + beta))
        g = num / (np.pi * t * (1 - (4 * beta * t) ** 2))
    g[np.abs(t) < 1e-12] = 1 - beta + 4 * beta / np.pi
    edge = np.abs(np.abs(4 * beta * t) - 1.0) < 1e-9
    g[edge] = beta / math.sqrt(2.0) * ((1 + 2 / np.pi) * math.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * math.cos(np.pi / (4 * beta)))
    g = (g + g[::-1]) / 2.0
    return (g * math.sqrt(U / float(np.sum(g * g)))).astype(np.float32)


# ---- continuous-phase modulations (amcx_synth_cpm_c64, ABI 16.2.2) ------------------------------------------------------------------
_M32 = (1 << 32) - 1
_FSK = re.compile(r"^(\d+)FSK$")


class CpmPulse:
    """A phase pulse at U samples per symbol: ``phase_taps[i]`` = the phase one unit of symbol has contributed i samples after
    its first, ``phase_full`` what it contributes for good, both in units of 2^-32 turn (uint32).  ``phase_taps``: a uint32
    array, or -- what :func:`generate` takes as it is -- an int32 tensor on the device holding those bits."""

    def __init__(self, phase_taps, phase_full: int):
        if not _tensor(phase_taps):
            phase_taps = np.ascontiguousarray(np.asarray(phase_taps, dtype=np.uint32))
        if phase_taps.ndim != 1 or not 1 <= int(phase_taps.shape[0]) <= MAX_TAPS or not 0 <= int(phase_full) <= _M32:
            raise ValueError(f"CpmPulse: 1 ... {MAX_TAPS} taps in one dimension and 0 <= phase_full < 2^32")
        self.phase_taps, self.phase_full = phase_taps, int(phase_full)


class CpmOrder(int):
    """What stands where a linear modulation's table stands: the size of a continuous-phase alphabet, 2 ... 256."""


def design_cpfsk(U: int, h=Fraction(1, 2)) -> CpmPulse:
    """Continuous-phase FSK, a rectangular frequency pulse of one symbol: U taps ``round(h/2 (i + 1)/U 2^32)``, ``phase_full =
    round(h/2 2^32)`` (exact rationals, halves away from zero).  h = 1/2 is MSK: 2^30, a quarter turn per symbol."""
    U, h = int(U), Fraction(h)
    if not 1 <= U <= MAX_UP or not 0 < h < 2:
        raise ValueError(f"design_cpfsk: U {U} (1 ... {MAX_UP}), h {h} (0 < h < 2)")
    unit = lambda x: int(math.floor(x * (1 << 32) + Fraction(1, 2)))       # noqa: E731
    return CpmPulse(np.array([unit(h / 2 * Fraction(i + 1, U)) for i in range(U)], np.uint32), unit(h / 2))


def design_gfsk(U: int, h, bt: float = 0.3, span_symbols: int = 4) -> CpmPulse:
    """Gaussian FSK: the rectangular frequency pulse of one symbol through a Gaussian low-pass of bandwidth ``bt`` symbol rates,
    cut to ``span_symbols`` symbols, accumulated and scaled so that the last of its ``span_symbols * U`` taps equals ``phase_full
    = round(h/2 2^32)``; non-decreasing."""
    U, h, bt, span = int(U), Fraction(h), float(bt), int(span_symbols)
    if not 1 <= U <= MAX_UP or not 0 < h < 2 or not bt > 0.0 or span < 1:
        raise ValueError(f"design_gfsk: U {U} (1 ... {MAX_UP}), h {h} (0 < h < 2), bt {bt} (> 0), span_symbols {span} (>= 1)")
    T = span * U
    if T > MAX_TAPS:
        raise ValueError(f"design_gfsk: {span} symbols at {U} samples per symbol are {T} taps, more than {MAX_TAPS}")
    full = int(math.floor(h / 2 * (1 << 32) + Fraction(1, 2)))
    c = math.pi * bt * math.sqrt(2.0 / math.log(2.0))
    t = [(i + 0.5) / U - span / 2.0 for i in range(T)]                      # sample centres, in symbols about the pulse's middle
    g = np.array([0.5 * (math.erf(c * (x + 0.5)) - math.erf(c * (x - 0.5))) for x in t], np.float64)
    q = np.cumsum(g) / float(np.sum(g))
    taps = np.minimum(np.rint(q * full), full).astype(np.uint64)
    taps[-1] = full
    return CpmPulse(np.maximum.accumulate(taps).astype(np.uint32), full)


def design_gmsk(U: int, bt: float = 0.3, span_symbols: int = 4) -> CpmPulse:
    """GMSK: :func:`design_gfsk` at h = 1/2."""
    return design_gfsk(U, Fraction(1, 2), bt, span_symbols)


def cpm_order(mod):
    """The alphabet of a continuous-phase name -- 2 for "MSK" and "GMSK", M for "MFSK" (2 ... 256) -- or None for any other name."""
    if isinstance(mod, CpmOrder):
        return int(mod)
    if not isinstance(mod, str):
        return None
    m = mod.upper()
    if m in ("MSK", "GMSK"):
        return 2
    fsk = _FSK.match(m)
    if fsk is None:
        return None
    if not 2 <= int(fsk.group(1)) <= MAX_ORDER:
        raise ValueError(f"{mod}: an FSK alphabet of 2 ... {MAX_ORDER}")
    return int(fsk.group(1))


def cpm_pulse(mod: str, U: int, *, h=None, bt: float = 0.3, span_symbols: int = 4) -> CpmPulse:
    """The default pulse of a continuous-phase name: "MSK" :func:`design_cpfsk` at 1/2, "GMSK" :func:`design_gmsk`, "MFSK"
    :func:`design_cpfsk` at h = 1 (tones one symbol rate apart) unless ``h`` says otherwise."""
    m = mod.upper()
    if m == "MSK":
        return design_cpfsk(U, Fraction(1, 2))
    if m == "GMSK":
        return design_gmsk(U, bt, span_symbols)
    return design_cpfsk(U, 1 if h is None else h)


def constellation_table(mod: str) -> np.ndarray:
    """The points of a modulation as complex64, unit average power; "WGN" / "NOISE": no point at all, the noise class."""
    pts = synth.constellation(mod)
    if mod.upper() in ("WGN", "NOISE"):
        return np.zeros(0, np.complex64)
    if len(pts) > MAX_ORDER:
        raise ValueError(f"{mod}: {len(pts)} points, the generator takes {MAX_ORDER}")
    return pts.astype(np.complex64)


def cfo_max_of(cfo) -> int:
    """The largest carrier offset a row draws, cycles per sample -> the entry's units of 2^-33 cycles per sample."""
    c = int(round(Fraction(cfo) * (1 << 33)))
    if not 0 <= c < 1 << 32:
        raise ValueError(f"cfo must lie in [0, 0.5) cycles per sample, got {cfo!r}")
    return c


def sigma_of(snr_db) -> np.ndarray:
    """sigma = 10^(-snr_db / 20) as float32: with a unit-power signal SNR = 1 / sigma^2."""
    return (10.0 ** (-np.atleast_1d(np.asarray(snr_db, dtype=np.float64)) / 20.0)).astype(np.float32)


def _sigmas(mod, snr_db, sigma):
    if snr_db is not None and sigma is not None:
        raise ValueError("either snr_db or sigma")
    if sigma is not None:
        s = np.atleast_1d(np.asarray(sigma, dtype=np.float32))
    elif snr_db is not None:
        s = sigma_of(snr_db)
        if isinstance(mod, str) and mod.upper() in ("WGN", "NOISE"):       # no signal to set the noise against: unit noise power
            s = np.ones_like(s)
    else:
        s = np.zeros(1, np.float32)
    if s.ndim != 1 or not np.all(np.isfinite(s)) or np.any(s < 0):
        raise ValueError("every sigma must be a finite float32 >= 0")
    return s


def _shape(sps):
    U, V = (int(sps), 1) if isinstance(sps, (int, np.integer)) else (int(sps[0]), int(sps[1]))
    if not (1 <= U <= MAX_UP and 1 <= V <= MAX_DOWN):
        raise ValueError(f"sps: U / V = {U} / {V} is outside 1 ... {MAX_UP} / 1 ... {MAX_DOWN}")
    return U, V


def _device(device):
    import torch
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _operands(mod, taps, U, snr_db=None, sigma=None, device=None) -> tuple:
    """``(table, taps, sigmas)`` as the entry reads them.  On the host: a modulation's name becomes its table, no taps the
    rectangular pulse, ``snr_db`` the sigmas, all as contiguous complex64 / float32 arrays; a tensor is left as it is.  With a
    ``device``, on it: what is on the host is uploaded, a tensor is taken as it is (and must be what the kernel reads)."""
    order = cpm_order(mod)
    if order is not None:
        return _cpm_operands(mod, order, taps, U, snr_db, sigma, device)
    if isinstance(taps, CpmPulse):
        raise TypeError("a CpmPulse goes with a continuous-phase name (MSK, GMSK, MFSK), not with a table")
    table = mod
    if not _tensor(mod):
        table = constellation_table(mod) if isinstance(mod, str) else np.ascontiguousarray(np.asarray(mod, dtype=np.complex64)).reshape(-1)
    if not _tensor(taps):
        taps = design_rect(U) if taps is None else np.ascontiguousarray(np.asarray(taps, dtype=np.float32))
    if _tensor(sigma) and snr_db is not None:
        raise ValueError("either snr_db or sigma")
    sig = sigma if _tensor(sigma) else _sigmas(mod, snr_db, sigma)          # on the device its values are the caller's (a NaN propagates)
    if device is None:
        return table, taps, sig
    import torch

    def resident(t, dtype, name):
        if not isinstance(t, torch.Tensor):
            return torch.from_numpy(t).to(device)
        if t.dtype != dtype or t.device != device or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous one-dimensional {str(dtype).replace('torch.', '')} tensor on the output's device")
        return t

    return resident(table, torch.complex64, "the table"), resident(taps, torch.float32, "taps"), resident(sig, torch.float32, "sigma")


def _cpm_operands(mod, order, pulse, U, snr_db, sigma, device) -> tuple:
    """:func:`_operands` of a continuous-phase name: ``(CpmOrder, CpmPulse, sigmas)``, the pulse's taps on ``device`` as int32."""
    if pulse is None:
        pulse = cpm_pulse(mod, U)
    if not isinstance(pulse, CpmPulse):
        raise TypeError(f"{mod}: a continuous-phase name takes a CpmPulse (design_cpfsk, design_gfsk, design_gmsk), not float taps")
    if _tensor(sigma) and snr_db is not None:
        raise ValueError("either snr_db or sigma")
    sig = sigma if _tensor(sigma) else _sigmas(mod, snr_db, sigma)
    if device is not None:
        import torch
        taps = pulse.phase_taps
        if not isinstance(taps, torch.Tensor):
            pulse = CpmPulse(torch.from_numpy(taps.view(np.int32)).to(device), pulse.phase_full)
        elif taps.dtype != torch.int32 or taps.device != device or not taps.is_contiguous():
            raise TypeError("a CpmPulse's taps on the device: a contiguous one-dimensional int32 tensor on the output's device")
        if not isinstance(sig, torch.Tensor):
            sig = torch.from_numpy(sig).to(device)
        elif sig.dtype != torch.float32 or sig.device != device or not sig.is_contiguous():
            raise TypeError("sigma must be a contiguous one-dimensional float32 tensor on the output's device")
    return CpmOrder(order), pulse, sig


def generate(mod, n_rows: int, row_samples: int, *, sps=(8, 1), taps=None, snr_db=None, sigma=None, frames_per_group=None,
             seed: int = 0, row_index0: int = 0, sample_index0: int = 0, cfo=0.0, shift=0.0, random_phase: bool = True,
             random_timing: bool = True, timing: int = 0, out=None, device=None, compute=None, acc_in=None, acc_out=None,
             segments: int = 0):
    """One launch of amcx_synth_c64 on the current torch stream -> complex64 ``(n_rows, row_samples)`` in GPU memory.

    mod     : a modulation's name (:func:`constellation_table`), or the table itself: up to 256 complex points, none for noise.
              The table (complex64), ``taps`` and ``sigma`` (float32) may each be a tensor on the device instead of a host
              array: what is a tensor is not uploaded.  With all three and ``out`` given the call is the launch alone -- no
              upload, no allocation -- and can be captured in a graph.  A ``sigma`` tensor's values are the caller's.
    sps     : ``(U, V)``: U / V samples per symbol, the taps given at U per symbol; an int is ``(U, 1)``.
    taps    : the pulse, float32 (numpy, or a tensor on the device); default :func:`design_rect`.
    snr_db / sigma : the noise, a scalar or one value per group of ``frames_per_group`` rows (default: the rows spread evenly
              over the values; no noise at all where neither is given).  "WGN" with ``snr_db`` is noise of unit power.
    seed, row_index0, sample_index0 : the key and where the call begins; rows ``row_index0 ...`` and samples
              ``sample_index0 ...`` of the same seed are the same numbers in whatever call they are made.
    cfo     : the largest carrier offset, cycles per sample: a row draws its own in ``[-cfo, cfo)``.  ``shift``: an offset every
              row has (cycles per sample, a float or a Fraction).
    random_phase, random_timing : a row's carrier phase and its timing ``tau`` (0 <= tau < U) drawn; else 0 and ``timing``.
    out     : a complex64 tensor ``(n_rows, row_samples)`` to write, possibly a strided view with contiguous rows.
    compute : tests only -- ``f(table, taps, U, V, n_rows, row_samples, sigma, frames_per_group, seed=..., row_index0=...,
              sample_index0=..., phase_step=..., cfo_max=..., flags=..., tau0=...)`` over numpy (tests/synth_ref.numpy_generate).

    A CONTINUOUS-PHASE name ("MSK", "GMSK", "2FSK", "4FSK", ...; amcx_synth_cpm_c64) takes a :class:`CpmPulse` for ``taps``
    (default :func:`cpm_pulse`) and carries one uint32 per row: ``acc_in`` (R words, a uint32 array or an int32 tensor on the
    device; needed where ``sample_index0 > 0``: the ``acc_out`` of the call that made the samples in front) and ``acc_out`` (an
    int32 tensor of R words to receive the state behind the call's last sample).  ``segments``: workgroups a row is cut into, 0
    the plan's choice.  There ``compute`` is ``f(order, phase_taps, phase_full, U, V, n_rows, row_samples, sigma,
    frames_per_group, acc_in=..., acc_out=..., ...)`` (tests/cpm_ref.numpy_generate)."""
    pulse_t = isinstance(taps, CpmPulse) and _tensor(taps.phase_taps)
    if compute is not None and (_tensor(mod) or _tensor(taps) or pulse_t or _tensor(sigma) or out is not None):
        raise TypeError("an injected compute takes host arrays and returns its own output")
    U, V = _shape(sps)
    R, S = int(n_rows), int(row_samples)
    table, taps, sig = _operands(mod, taps, U, snr_db, sigma)
    cpm = isinstance(table, CpmOrder)
    if not cpm and (acc_in is not None or acc_out is not None or segments):
        raise TypeError("acc_in, acc_out and segments belong to the continuous-phase names")
    length = lambda t: int(t.shape[0]) if t.ndim == 1 else -1               # noqa: E731
    order, T, G = int(table) if cpm else length(table), length(taps.phase_taps if cpm else taps), length(sig)
    if R < 0 or S < 1 or not 0 <= int(sample_index0) or int(sample_index0) + S >= 1 << 40 or not 0 <= order <= MAX_ORDER \
            or not 1 <= T <= MAX_TAPS or G < 1:
        raise ValueError(f"outside the generator's limits: n_rows {R}, row_samples {S}, sample_index0 {sample_index0}, order {order}, "
                         f"{T} taps, {G} sigmas (each in one dimension)")
    if not 0 <= int(timing) < U:
        raise ValueError(f"timing must lie in 0 ... U - 1 = {U - 1}")
    fpg = max(1, -(-R // G)) if frames_per_group is None else int(frames_per_group)
    if fpg < 1 or (R > 0 and -(-R // fpg) > G):
        raise ValueError(f"{R} rows in groups of {fpg} need {-(-R // max(fpg, 1))} sigmas, {G} given")
    flags = (_lib.SYNTH_RANDOM_PHASE if random_phase else 0) | (_lib.SYNTH_RANDOM_TIMING if random_timing else 0)
    step, cfo_max = _stream.phase_step_of(shift), cfo_max_of(cfo)
    where = dict(seed=int(seed) & _MASK64, row_index0=int(row_index0) & _MASK64, sample_index0=int(sample_index0),
                 phase_step=step, cfo_max=cfo_max, flags=flags, tau0=int(timing))
    if cpm and int(sample_index0) > 0 and acc_in is None:
        raise ValueError("a continuous-phase row that begins behind sample 0 needs acc_in, the state of the samples in front")
    if compute is not None:
        if cpm:
            return compute(order, taps.phase_taps, taps.phase_full, U, V, R, S, sig, fpg, acc_in=acc_in, acc_out=acc_out, **where)
        return compute(table if order else None, taps, U, V, R, S, sig, fpg, **where)

    import torch
    if out is not None:
        _, _, stride = _stream.rows_of(out, torch.complex64, "out", "row_samples", S, S, narrow="out must have row_samples = {} columns",
                                       min_rows=R)
        if int(out.shape[0]) != R:
            raise ValueError(f"out has {int(out.shape[0])} rows, the call makes {R}")
        dev = out.device
    else:
        dev = _device(device)
        stride = S
    table, taps, sig = _operands(table, taps, U, sigma=sig, device=dev)
    if out is None:
        out = torch.empty((R, S), dtype=torch.complex64, device=dev)
    if cpm:
        def state(t, name, upload):
            """a row-state array as the entry reads it; a host array is uploaded where that makes sense (acc_in)"""
            if t is not None and upload and not isinstance(t, torch.Tensor):
                t = torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.uint32)).view(np.int32)).to(dev)
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != dev
                                  or not t.is_contiguous() or t.numel() != R):
                raise TypeError(f"{name}: a contiguous int32 tensor of n_rows words on the output's device")
            return t
        a_in, a_out = state(acc_in, "acc_in", True), state(acc_out, "acc_out", False)
        _stream.launch(out, lambda lib, stream: lib.amcx_synth_cpm_c64(
            where["seed"], where["row_index0"], where["sample_index0"], R, S, stride, order, taps.phase_taps.data_ptr(), T,
            taps.phase_full, U, V, where["tau0"], step, cfo_max, flags, sig.data_ptr(), fpg,
            a_in.data_ptr() if a_in is not None and R else None, a_out.data_ptr() if a_out is not None and R else None,
            int(segments), out.data_ptr() if R else None, stream))
        return out
    _stream.launch(out, lambda lib, stream: lib.amcx_synth_c64(
        where["seed"], where["row_index0"], where["sample_index0"], R, S, stride, table.data_ptr() if order else None, order,
        taps.data_ptr(), T, U, V, where["tau0"], step, cfo_max, flags, sig.data_ptr(), fpg, out.data_ptr() if R else None, stream))
    return out


# ---- data sets ----------------------------------------------------------------------------------------------------------------
def mod_code(mod: str) -> int:
    """A modulation's number in :func:`dataset`'s rows, from its name alone: (family << 12) | order, the family 0 for a name
    that ends in PSK, 1 for QAM, 2 for the noise class, 3 for MFSK, 4 for MSK, 5 for GMSK.  Two names of one family and order (a variant constellation added
    later under another name) would share their rows: :func:`dataset` refuses them in one call."""
    m = mod.upper()
    if m in ("WGN", "NOISE"):
        return 2 << 12
    if cpm_order(m) is not None:
        return ({"MSK": 4, "GMSK": 5}.get(m, 3) << 12) | cpm_order(m)
    order = len(synth.constellation(m))
    return ((0 if m.endswith("PSK") else 1) << 12) | order


def snr_code(snr_db) -> int:
    """An SNR's number in :func:`dataset`'s rows, from its value alone: eighths of a dB above -1000 dB, the nearest.  Two
    values less than 0.125 dB apart can share a number, and so their rows -- the same symbols and noise words at another
    sigma: :func:`dataset` refuses them in one call."""
    c = int(round((float(snr_db) + 1000.0) * 8.0))
    if not 0 <= c < 1 << SNR_BITS:
        raise ValueError(f"snr_db {snr_db!r} is outside -1000 ... +7191 dB")
    return c


def dataset_row(mod: str, snr_db, frame: int = 0) -> int:
    """The absolute row of (modulation, SNR, frame): the same whatever subset of modulations, SNRs or frames is asked for."""
    if not 0 <= int(frame) < 1 << FRAME_BITS:
        raise ValueError("frame must lie in 0 ... 2^32 - 1")
    return (mod_code(mod) << (SNR_BITS + FRAME_BITS)) | (snr_code(snr_db) << FRAME_BITS) | int(frame)


def _grid(mods, snr_db) -> tuple:
    """The modulations and SNRs of a data set; ValueError where two of either share their rows (mod_code, snr_code)."""
    mods = list(mods)
    snrs = [float(v) for v in np.atleast_1d(np.asarray(snr_db, dtype=np.float64))]
    for what, items, code in (("modulations", mods, mod_code), ("SNR values", snrs, snr_code)):
        seen = {}
        for item in items:
            if seen.setdefault(code(item), item) != item or items.count(item) > 1:
                raise ValueError(f"the {what} {seen[code(item)]!r} and {item!r} name the same rows of a data set: one of them in a call")
    return mods, snrs


def _walk(mods, snrs, F, N, chunk, first_frame, kw, shape, view, each=None) -> dict:
    """The one walk of a data set -> mod -> its buffer of ``shape``.  Per modulation the operands go to the device ONCE; then per SNR
    and chunk of at most ``chunk`` of the F frames (None: all, even none, at once) ONE launch makes the frames ``first_frame + f0 ...``
    into ``view(buf, s, n)`` and ``each(mod, s, f0, frames)`` sees them.  An injected ``compute`` walks the same way over numpy."""
    kw = dict(kw)
    fade = kw.pop("channel", None)
    U, _ = _shape(kw.get("sps", (8, 1)))
    dev = _device(kw.get("device")) if kw.get("compute") is None else None
    H = _channel_history(fade)
    clean = None if fade is None or dev is None else _empty((min(chunk or F, F), N + H), dev)   # the rows before the channel
    data = {}
    for mod in mods:
        taps = kw.get("taps")
        table, taps, sig = _operands(mod, taps.get(mod) if isinstance(taps, dict) else taps, U, snr_db=snrs, device=dev)
        buf = data[mod] = _empty(shape, dev)
        for s, snr in enumerate(snrs):
            for f0 in (range(0, F, chunk) if chunk else (0,)):
                dst = view(buf, s, min(chunk or F, F - f0))
                row0 = dataset_row(mod, snr, first_frame + f0)
                if fade is None:
                    x = generate(table, dst.shape[0], N, sigma=sig[s:s + 1], row_index0=row0,
                                 **dict(kw, taps=taps, device=dev, out=None if dev is None else dst))
                else:
                    x = _faded(fade, table, dst.shape[0], N, H, sig[s:s + 1], row0, dict(kw, taps=taps, device=dev),
                               None if dev is None else clean[:dst.shape[0]], None if dev is None else dst)
                if dev is None:
                    dst[...] = x
                if each is not None:
                    each(mod, s, f0, dst)
    return data


_CHANNEL_KEYS = ("profile", "doppler", "sinusoids", "interp_log2", "random_phase", "compute")


def _channel_history(fade) -> int:
    """H of a ``channel=dict(profile=..., doppler=..., ...)`` keyword (:func:`amcpy_amd.channel.apply`'s keywords); 0 for None."""
    if fade is None:
        return 0
    if "profile" not in fade or set(fade) - set(_CHANNEL_KEYS):
        raise ValueError(f"channel: a dict with profile and any of {_CHANNEL_KEYS[1:]}, got {sorted(fade)}")
    return fade["profile"].history


def _channel_record(fade) -> dict:
    """What a provenance record says of the channel a data set went through: the profile (its name where a command named it),
    the Doppler and the sinusoids."""
    p = fade["profile"]
    return {"profile": getattr(p, "spec", None), "delays": [int(d) for d in p.delays], "diffuse_gain": [float(g) for g in p.diffuse_gain],
            "los_gain": [float(g) for g in p.los_gain], "los_doppler": [float(g) for g in p.los_doppler],
            "doppler": float(fade.get("doppler", 0.0)), "sinusoids": int(fade.get("sinusoids", 16)),
            "interp_log2": fade.get("interp_log2"), "random_phase": bool(fade.get("random_phase", True))}


def _faded(fade, table, n, N, H, sigma, row0, kw, clean, dst):
    """n rows of N samples through a channel: the clean rows ``(n, N + H)`` without noise (into ``clean`` on the device), then
    :func:`amcpy_amd.channel.apply` (into ``dst``) with the same seed, the same absolute rows and the sigma -- so a faded row is
    named by its absolute row exactly as a plain one is."""
    from . import channel
    x = generate(table, n, N + H, row_index0=row0, **dict(kw, out=clean))
    return channel.apply(x, seed=kw.get("seed", 0), row_index0=row0, sigma=sigma, out=dst, **fade)


def _empty(shape, device):
    if device is None:
        return np.empty(shape, np.complex64)
    import torch
    return torch.empty(shape, dtype=torch.complex64, device=device)


def dataset(mods, snr_db, n_frames: int, frame_size: int, *, first_frame: int = 0, **kw) -> dict:
    """mod -> ``(n_snr, n_frames, frame_size)`` complex64, the reference's container layout.  ``channel=dict(profile=...,
    doppler=..., ...)`` (:func:`amcpy_amd.channel.apply`'s keywords) takes every frame through a fading channel: each launch makes
    the clean rows with the channel's history in front, without noise, and the channel's launch adds the noise; the seed and the
    absolute rows are the same, so faded rows are as subset-stable as plain ones.  Frame f of (mod, SNR) is row
    :func:`dataset_row` ``(mod, snr, first_frame + f)``, so any subset names the same rows; the rows of two SNRs are 2^32 apart,
    which makes it one launch per (modulation, SNR), each into its slice of the modulation's array.  The table, the taps and
    the sigmas go to the device once per modulation; the launches upload nothing."""
    mods, snrs = _grid(mods, snr_db)
    F, N = int(n_frames), int(frame_size)
    return _walk(mods, snrs, F, N, None, first_frame, kw, (len(snrs), F, N), lambda buf, s, n: buf[s])   # (taps: one pulse, or mod -> its pulse)


def dataset_features(mods, snr_db, n_frames: int, frame_size: int, *, chunk_frames: int = 1 << 14, features=None, recover=None,
                     recover_compute=None, **kw) -> dict:
    """mod -> ``(n_snr, n_frames, 18)`` float32 (numpy): the frames of :func:`dataset` made ``chunk_frames`` at a time, put
    through :func:`amcpy_amd.features.features18` and dropped, so a training set larger than the device's memory never exists
    as IQ.  ``features``: tests only, ``f(frames (F, N) complex64 numpy) -> (F, 18)`` beside an injected ``compute``.
    ``recover`` (default None: the bits without the keyword): ``dict(order=M, search=cycles per sample)`` -- every frame through
    :func:`amcpy_amd.carrier.recover_frames` in front of the features, as ``extract_sigmf(tune=dict(..., recover=...))`` treats a
    recording's, so that what a classifier is trained on is what it will see.  Every row draws its own carrier, so
    ``per="emitter"`` has no meaning here and is refused; ``search_hz`` too (the generator knows no rate).  ``recover_compute``:
    tests only, ``f(frames numpy, recover) -> frames`` beside the injected ``compute`` and ``features``."""
    mods, snrs = _grid(mods, snr_db)
    F, N, chunk = int(n_frames), int(frame_size), max(1, int(chunk_frames))
    if recover is not None:
        if not isinstance(recover, dict) or recover.get("per", "frame") != "frame" or recover.get("search_hz") is not None:
            raise ValueError("recover: dict(order=M, search=cycles per sample); every row is its own emitter and there is no rate")
        injected = features is not None or kw.get("compute") is not None
        if injected and (features is None or recover_compute is None):
            raise ValueError("recover runs on the device: beside an injected compute it needs features and recover_compute too")
        if injected:
            plain = features
            features = lambda x: plain(recover_compute(np.asarray(x), recover))           # noqa: E731
        else:
            from . import carrier
            from .features import features18
            features = lambda x: features18(carrier.recover_frames(x, recover)[0]).cpu().numpy()           # noqa: E731
    if features is None:
        from .features import features18
        features = lambda x: features18(x).cpu().numpy()           # noqa: E731
    out = {mod: np.empty((len(snrs), F, _lib.NUM_FEATURES), np.float32) for mod in mods}

    def keep(mod, s, f0, x):
        out[mod][s, f0:f0 + x.shape[0]] = np.asarray(features(x), dtype=np.float32)[:, :_lib.NUM_FEATURES]
    _walk(mods, snrs, F, N, chunk, 0, kw, (min(chunk, F), N), lambda buf, s, n: buf[:n], keep)
    return out


class Stream:
    """One row as a stream: ``push(n)`` returns its next n samples (``index`` counts the samples made so far, as
    :class:`amcpy_amd._stream.Chunked` counts them).  Cut anywhere, the chunks equal one call bit for bit.  The keywords are
    :func:`generate`'s; ``row`` is the absolute row.  The table, the taps and sigma go to the device once, with the first samples."""

    def __init__(self, mod, *, row: int = 0, **kw):
        for bad in ("row_index0", "sample_index0", "out", "frames_per_group"):
            if bad in kw:
                raise ValueError(f"Stream: {bad} is the stream's own")
        self.mod, self.row, self.index, self._kw, self._resident = mod, int(row), 0, dict(kw), None
        self._acc, self._cur = None, 0         # a continuous-phase row's two words of state, swapped per push

    def push(self, n: int):
        n = int(n)
        if n < 0:
            raise ValueError("push: n >= 0")
        mod, kw = self.mod, self._kw
        dev = _device(kw.get("device")) if kw.get("compute") is None else None
        if n == 0:
            return _empty(0, dev)
        if dev is not None:
            if self._resident is None:
                self._resident = _operands(mod, kw.get("taps"), _shape(kw.get("sps", (8, 1)))[0], kw.get("snr_db"), kw.get("sigma"), dev)
            mod, taps, sig = self._resident
            kw = dict(kw, taps=taps, sigma=sig, snr_db=None)
        if cpm_order(self.mod) is not None:    # acc_out of one push is acc_in of the next
            if self._acc is None:
                self._acc = _state_words(dev)
            kw = dict(kw, acc_in=self._acc[self._cur] if self.index else None, acc_out=self._acc[1 - self._cur])
            self._cur = 1 - self._cur
        y = generate(mod, 1, n, row_index0=self.row, sample_index0=self.index, **kw)
        self.index += n
        return y[0]


def _state_words(device):
    """two rows of one word: a stream's carried sums, on the device (int32) or for an injected compute (uint32 numpy)"""
    if device is None:
        return np.zeros((2, 1), np.uint32)
    import torch
    return torch.zeros((2, 1), dtype=torch.int32, device=device)


def scene(emitters, n_samples: int, *, noise_sigma: float, seed: int = 0, device=None) -> tuple:
    """A stream of ``n_samples`` with known emitters on a noise floor -> ``(x, annotations)``.

    emitters : dicts with ``mod``, ``sps`` (U, V), ``center`` (cycles per sample of the scene), and optionally ``rate`` (L, D)
               (1, 1), ``start`` (0), ``length`` (to the end), ``amplitude`` (1), ``channel`` (a fading channel the emitter passes
               at the scene's rate: :func:`dataset`'s keyword), ``taps`` (default: :func:`design_rrc` over 16
               symbols where U > V and it fits, else rect; a continuous-phase name: its :func:`cpm_pulse`), ``beta`` (0.35).  Emitter e is row e of the seed; the floor is the
               noise class in row ``len(emitters)``.
    Each emitter is one :class:`Stream` row at its own U / V samples per symbol, brought to the scene's rate by
    :func:`amcpy_amd.resample.resample` (L / D, the default low-pass: U L / (V D) samples per symbol in the scene), moved to its
    centre by the same entry's mixer (one tap of 1, ``shift=center``, the phase counted from the scene's sample 0) and added in.
    annotations : one dict per emitter with the keys :func:`amcpy_amd.sigmf.tune_from_annotation` reads --
               ``core:sample_start``, ``core:sample_count``, ``core:freq_lower_edge`` / ``core:freq_upper_edge`` in cycles per
               sample (the occupied band: (1 + beta) symbol rates wide, one symbol rate for a rectangular pulse) -- and
               ``core:label``, ``amcx:samples_per_symbol``."""
    import torch

    from .resample import design_resample_lowpass, out_samples, resample
    S = int(n_samples)
    dev = _device(device)
    x = generate("WGN", 1, S, sigma=float(noise_sigma), seed=seed, row_index0=len(emitters), device=dev)[0]
    one = torch.ones(1, dtype=torch.float32, device=dev)
    annotations = []
    for e, em in enumerate(emitters):
        U, V = _shape(em["sps"])
        L, D = (int(v) for v in em.get("rate", (1, 1)))
        start = int(em.get("start", 0))
        length = int(em.get("length", S - start))
        if not (0 <= start and length >= 1 and start + length <= S):
            raise ValueError(f"emitter {e}: samples {start} ... {start + length} are outside the scene's {S}")
        beta = float(em.get("beta", 0.35))
        taps = em.get("taps")
        alphabet = cpm_order(em["mod"])                          # a continuous-phase emitter keeps its own pulse
        rrc = taps is None and alphabet is None and 16 * U + 1 <= MAX_TAPS and U > V
        if taps is None and alphabet is None:
            taps = design_rrc(U, 16, beta) if rrc else design_rect(U)
        stream = Stream(em["mod"], row=e, sps=(U, V), taps=taps, seed=seed, device=dev)
        fade = em.get("channel")
        need = length + _channel_history(fade)                   # the channel's history in front of the emitter's first sample
        if (L, D) == (1, 1):
            y = stream.push(need)
        else:
            low = design_resample_lowpass(L, D)
            n_in = -(-need * D // L) + -(-len(low) // L) + 1
            while out_samples(n_in, len(low), L, D) < need:
                n_in += 1
            y = resample(stream.push(n_in), low, L, D)[:need]
        if fade is not None:                                     # at the scene's rate, in front of the move to its centre
            from . import channel
            y = channel.apply(y.contiguous()[None, :], seed=seed, row_index0=e, **fade)[0]
        y = resample(y.contiguous(), one, 1, 1, shift=em["center"], sample_index0=start)
        x[start:start + length] += y * float(em.get("amplitude", 1.0))
        per_symbol = Fraction(U * L, V * D)
        width = (1.0 + beta if rrc else 1.0) / float(per_symbol)
        if alphabet is not None and _FSK.match(str(em["mod"]).upper()):
            width *= alphabet                                    # M tones a symbol rate apart (the default h = 1)
        annotations.append({"core:sample_start": start, "core:sample_count": length, "core:label": str(em["mod"]),
                            "core:freq_lower_edge": float(em["center"]) - width / 2.0,
                            "core:freq_upper_edge": float(em["center"]) + width / 2.0,
                            "amcx:samples_per_symbol": float(per_symbol)})
    return x, annotations


# ---- the `synth` command ----------------------------------------------------------------------------------------------------------
def parse_sps(text: str) -> tuple:
    u, _, v = str(text).partition("/")
    return int(u), int(v) if v else 1


def parse_snr(text: str) -> list:
    """``lo:hi:step`` (hi included) or one value, in dB."""
    parts = [float(p) for p in str(text).split(":")]
    if len(parts) == 1:
        return [parts[0]]
    if len(parts) != 3 or parts[2] <= 0 or parts[1] < parts[0]:
        raise ValueError(f"--snr: lo:hi:step with step > 0 and hi >= lo, got {text!r}")
    n = int(math.floor((parts[1] - parts[0]) / parts[2] + 1e-9)) + 1
    return [parts[0] + i * parts[2] for i in range(n)]


def _label(v: float) -> str:
    return str(int(v)) if float(v).is_integer() else repr(float(v))


V5_LIMIT = (1 << 31) - 1      # bytes of one MATLAB v5 file's variables


def run_synth(cfg, *, mods=None, sps=(8, 1), pulse: str = "rrc", beta: float = 0.35, span: int = 16, snr=None, cfo=0.0,
              seed: int = 0, features_only: bool = False, device=None, compute=None, features=None, verbose: bool = True,
              channel=None, cpm=None, recover=None, recover_compute=None) -> list:
    """The `synth` command: the data set of ``cfg`` (its frame size, frame count and SNR labels, unless ``snr`` names the
    grid) for ``mods`` (default ``cfg.signals.modulations_with_noise``) into ``mat-data/all_modulations.mat`` under the variables
    ``cfg.signals.mat_info`` names -- or, ``features_only``, straight into ``calculated-features/{mod}_features.mat`` with the
    provenance record `extract --resume` trusts.  ``channel``: :func:`dataset`'s keyword, a fading channel every frame passes; the
    provenance record names it.  ``cpm``: ``dict(h=..., bt=..., span=...)``, the pulse of the continuous-phase names among
    ``mods`` (:func:`cpm_pulse`), named in their provenance records too.  ``recover``: with ``features_only``, the order M of the
    blind carrier recovery every frame passes in front of the features (:func:`dataset_features`' ``recover=dict(order=M)``), named in
    the provenance record as ``"recover": {"order": M}``.  Returns the files written.  ``compute`` / ``features``: injected (tests)."""
    import scipy.io

    from .feature_extraction import _provenance, _provenance_path
    sig = cfg.signals
    mods = list(sig.modulations_with_noise if mods is None else mods)
    for m in mods:
        if m not in sig.mat_info:
            raise ValueError(f"{m}: the configuration names no container variable for it ({sorted(sig.mat_info)})")
    snrs = [float(v) for v in sig.snr_values.values()] if snr is None else [float(v) for v in snr]
    if len(snrs) != len(sig.snr_values):
        raise ValueError(f"{len(snrs)} SNR values against the configuration's {len(sig.snr_values)} labels")
    U, V = _shape(sps)
    if pulse not in ("rrc", "rect"):
        raise ValueError("pulse: rrc or rect")
    linear = design_rrc(U, span, beta) if pulse == "rrc" else design_rect(U)
    shape = {"h": None, "bt": 0.3, "span": 4, **(cpm or {})}
    taps = {m: linear if cpm_order(m) is None else cpm_pulse(m, U, h=shape["h"], bt=shape["bt"], span_symbols=shape["span"])
            for m in mods}
    F, N = int(sig.num_frames), int(sig.frame_size)
    kw = dict(sps=(U, V), taps=taps, cfo=cfo, seed=seed, compute=compute)
    if compute is None:
        kw["device"] = device
    if channel is not None:
        kw["channel"] = channel
    cfg.paths.ensure_dirs()
    mat_path = cfg.paths.mat_data / cfg.paths.mat_filename
    if recover is not None and not features_only:
        raise ValueError("recover belongs to features_only: the container holds the rows as they were generated")
    if features_only:
        written = []
        for m in mods:
            feats = dataset_features([m], snrs, F, N, features=features, recover=None if recover is None else dict(order=int(recover)),
                                     recover_compute=recover_compute, **kw)[m]
            out_path = cfg.paths.calculated_features / f"{m}_features.mat"
            scipy.io.savemat(str(out_path), {"Modulation": m, sig.mat_info[m]: feats})
            record = _provenance(cfg, mat_path, sig.mat_info[m])
            if channel is not None:
                record["channel"] = _channel_record(channel)
            if cpm_order(m) is not None:
                record["cpm"] = {"order": cpm_order(m), "taps": int(taps[m].phase_taps.shape[0]), "phase_full": taps[m].phase_full,
                                 "h": None if shape["h"] is None else str(Fraction(shape["h"])), "bt": float(shape["bt"]),
                                 "span": int(shape["span"])}
            if recover is not None:
                record["recover"] = {"order": int(recover)}
            _provenance_path(out_path).write_text(json.dumps(record) + "\n")
            written.append(out_path)
            if verbose:
                print(f"synth: {m}: features {feats.shape} -> {out_path}")
        return written
    per_mod = len(snrs) * F * N * 8
    if per_mod * len(mods) > V5_LIMIT:
        raise ValueError(f"the container would hold {len(mods)} variables of {len(snrs)} x {F} x {N} complex64, {per_mod * len(mods)} bytes: "
                         f"more than a MATLAB v5 file's {V5_LIMIT}; --features-only writes calculated-features/ without it")
    data = dataset(mods, snrs, F, N, **kw)
    scipy.io.savemat(str(mat_path), {sig.mat_info[m]: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for m, v in data.items()})
    if verbose:
        print(f"synth: {len(mods)} modulations x {len(snrs)} SNRs x {F} frames of {N} -> {mat_path}")
    return [mat_path]
