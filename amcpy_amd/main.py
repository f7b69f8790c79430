"""`python -m amcpy_amd extract [--root DIR] [--frame-size N] [--num-frames F] [--snr-values L ...]
                              [--device D | --devices 0,1,...|all] [--resume] [--features all|used|3,5,...]`

The `extract` sub-command of the reference's CLI (src/amcpy/main.py:32,85-87,
160-175); plot and train are outside the hot path.
`python -m amcpy_amd classify --root DIR --model ID|PATH [--mode training|test] [--from-iq] [--device D]` is the
evaluation half of the reference's `eval` (nn_model.evaluate_by_snr) on the GPU: amcpy_amd/classifier.py.  The reference's dispatcher calls ``cmd_extract(cfg, args)``
on a one-argument function (main.py:175 vs :85) and raises TypeError as
written; this entry point takes the same defaults and simply works.
`python -m amcpy_amd quantize --root DIR --model ID|PATH [--mode training|test] [--layout reference|folded] [--no-normalize]
[--evaluate] [--device D]` is the reference's `quantize` stage (nn_quantization.py) with the ranges calibrated and the 16-bit integer
network run on the GPU: amcpy_amd/quantize.py.
`python -m amcpy_amd recording FILE --frame-size N [--format cf32|sc16|ci8|cu8] [--scale S] [--features ...] [--device D]
[--out PATH] [--shift-hz F --decimate D [--taps T] | --shift-hz F --resample L/D [--taps T] | --annotation K [--oversample R]
[--rational] | --channels C [--oversample 1|2]
[--taps-per-channel P] [--shift-hz F]]` takes ONE recording -- a SigMF recording (its meta file says the format: no --format), or a raw sample
stream -- and writes `features` (F, 18) and `frame_start` (F,) into a .mat file: amcpy_amd/sigmf.py, extract_raw_stream.
The tuning flags (SigMF only) put the device's down-converter in front: the emitter moved to 0 Hz, low-passed and decimated
(amcpy_amd/ddc.py; sigmf.extract_sigmf, tune=); --resample L/D and --rational put the rational resampler there instead
(amcpy_amd/resample.py): the rate changes by L / D, and the output file also records `interp` and `decim`.  With the tuning flags,
`--recover M [--recover-search-hz F]` puts blind carrier recovery of order M (amcpy_amd/carrier.py) between the tuned frames and the
features; the output file gains `carrier_hz`, `carrier_phase` and `carrier_quality`.  `synth --features-only --recover M` does the same
to the generated frames and names it in the provenance record.
`python -m amcpy_amd scan FILE [--nfft N] [--hop H] [--averages A] [--window hann|rect] [--threshold-db X] [--floor-quantile Q]
[--min-bins B] [--merge-bins G] [--min-rows R] [--format ...] [--scale S] [--device D] [--out PATH] [--annotate OUT.sigmf-meta]`
finds the emitters of a recording with no raster: the Welch spectrogram on the device, a floor and a mask per row, the occupied
bins joined into emitters (amcpy_amd/psd.py; sigmf.scan_sigmf), written into a .mat file and, with --annotate, into a copy of
the meta file as annotations -- which `recording --annotation K --rational` reads back.
`python -m amcpy_amd synth --root DIR [--mods M ...] [--sps U/V] [--pulse rrc|rect] [--beta B] [--span S] [--frames F] [--frame-size N]
[--snr lo:hi:step] [--cfo X] [--seed S] [--channel PROFILE --doppler F [--sinusoids S]] [--cpm-h H] [--bt B] [--cpm-span S] [--features-only] [--device D]` makes the labelled data set on the GPU (amcpy_amd/waveform.py):
mat-data/all_modulations.mat as the reference expects it, or, --features-only, calculated-features/ directly.  --mods takes the
continuous-phase names as well (MSK, GMSK, 2FSK, 4FSK, ...; the last three flags shape their pulse), separated by blanks or commas;
`train`, `classify` and `quantize` take the same --mods where the classes are not the configuration's six.

Several GPUs, ONE command (the reference's caller runs one command and the parallelism happens inside,
feature_extraction.py:89-97): ``--devices 0,1,2,3`` / ``--devices all`` drives one engine per device from one
host thread each inside this process (feature_extraction.DeviceFanOut) -- no launcher, no process group, no
torch.  Started under ``torch.distributed.run`` instead (RANK / WORLD_SIZE in the environment), every rank takes
the GPU of its LOCAL_RANK, joins the process group and computes its share; rank 0 writes the files.
"""
from __future__ import annotations

import argparse
import json
import os
import time
import sys
from dataclasses import replace
from pathlib import Path

from .config import Config, Paths


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="amcpy_amd", description="MI355X IQ feature extraction")
    sub = ap.add_subparsers(dest="command", required=True)
    ex = sub.add_parser("extract", help="compute the 18 features for every modulation container")
    ex.add_argument("--root", type=Path, default=None, help="project root (default: cwd)")
    ex.add_argument("--frame-size", type=int, default=None)
    ex.add_argument("--num-frames", type=int, default=None)
    ex.add_argument("--snr-values", nargs="+", default=None, metavar="LABEL",
                    help="SNR labels of the container's first axis, in order (default: the 16 of SignalConfig)")
    ex.add_argument("--device", type=int, default=None, help="GPU index (default: current device)")
    ex.add_argument("--resume", action="store_true",
                    help="skip modulations whose {mod}_features.mat is already complete for this configuration")
    ex.add_argument("--devices", default=None, metavar="0,1,...|all",
                    help="several GPUs from this one process, frames cut across them (one engine and host thread each)")
    ex.add_argument("--features", default="all", metavar="all|used|3,5,...",
                    help="features to compute (default all).  'used': the columns the reference's preprocess_data and "
                         "evaluate_by_snr read (FeatureConfig.used + 1); or a comma-separated list of ids 1 ... 18.  The "
                         "files keep their (n_snr, n_frames, 18) float32 layout with NaN in the other columns; `plot` "
                         "needs all 18")
    cl = sub.add_parser("classify", help="classify every (modulation, SNR, frame) on the GPU and write the accuracy table")
    cl.add_argument("--root", type=Path, default=None, help="project root (default: cwd)")
    cl.add_argument("--model", required=True, metavar="ID|PATH",
                    help="the id of ann/model-{ID}.pt under the root (the file the reference's training writes), or a "
                         "path to a .pt checkpoint / .npz model")
    cl.add_argument("--mode", choices=("training", "test"), default="test",
                    help="rows the scaler is fitted on, as the reference's preprocess_data: training_snr or all_snr (default)")
    cl.add_argument("--from-iq", action="store_true",
                    help="run the extraction first (the used features only) instead of reading calculated-features/")
    cl.add_argument("--device", type=int, default=None, help="GPU index (default: current device)")
    qz = sub.add_parser("quantize", help="export the network as 16-bit fixed point; --evaluate runs the integer network on the GPU")
    qz.add_argument("--root", type=Path, default=None, help="project root (default: cwd)")
    qz.add_argument("--model", required=True, metavar="ID|PATH", help="as for classify")
    qz.add_argument("--mode", choices=("training", "test"), default="test", help="rows the scaler is fitted on, as for classify")
    qz.add_argument("--layout", choices=("reference", "folded"), default="folded",
                    help="reference: the Linear layers as stored into arm-data/w_and_b.mat, as the reference writes it; folded "
                         "(default): every BatchNorm folded, into arm-data/{model_id}_q15.mat")
    qz.add_argument("--evaluate", action="store_true",
                    help="run the integer network over every row beside the float classifier: figures/{model_id}_q15_figure_data.mat")
    qz.add_argument("--no-normalize", action="store_true",
                    help="folded layout: export the block as it is; by default a layer whose range passes Q6.9 is scaled by a power "
                         "of two (the labels stay the same), so that nothing clips")
    qz.add_argument("--device", type=int, default=None, help="GPU index (default: current device)")
    qz.add_argument("--frame-size", type=int, default=None)
    qz.add_argument("--num-frames", type=int, default=None)
    qz.add_argument("--snr-values", nargs="+", default=None, metavar="LABEL")
    cl.add_argument("--frame-size", type=int, default=None)
    cl.add_argument("--num-frames", type=int, default=None)
    cl.add_argument("--snr-values", nargs="+", default=None, metavar="LABEL",
                    help="SNR labels of the container's first axis, in order (default: the 16 of SignalConfig)")
    tr = sub.add_parser("train", help="train the classifier on the GPU from calculated-features/: ann/model-{id}.pt, figures/{id}_history.mat")
    tr.add_argument("--root", type=Path, default=None, help="project root (default: cwd)")
    tr.add_argument("--epochs", type=int, default=None)
    tr.add_argument("--batch-size", type=int, default=None, help="2 ... 256")
    tr.add_argument("--lr", type=float, default=None)
    tr.add_argument("--dropout", type=float, default=None)
    tr.add_argument("--optimizer", choices=("rmsprop", "adam"), default=None)
    tr.add_argument("--activation", choices=("relu", "tanh", "sigmoid"), default=None)
    tr.add_argument("--seed", type=int, default=None, help="of the split, the initialisation, the epochs' orders and the dropout masks")
    tr.add_argument("--sweep-lr", default=None, metavar="a,b,...", help="one model per value, all trained side by side (256 at most)")
    tr.add_argument("--sweep-dropout", default=None, metavar="a,b,...", help="as --sweep-lr; with both, two lists of one length")
    tr.add_argument("--device", type=int, default=None, help="GPU index (default: current device)")
    for p in (tr, cl, qz):
        p.add_argument("--mods", nargs="+", default=None, metavar="MOD",
                       help="the classes, in label order, where they are not the configuration's six (as `synth --mods` named them)")
    tr.add_argument("--frame-size", type=int, default=None)
    tr.add_argument("--num-frames", type=int, default=None)
    tr.add_argument("--snr-values", nargs="+", default=None, metavar="LABEL")
    rec = sub.add_parser("recording", help="the features of one recording: a SigMF recording or a raw sample stream")
    rec.add_argument("file", type=Path, metavar="FILE",
                     help="X.sigmf-meta, X.sigmf-data or the stem X of a SigMF recording; or a raw stream (then --format)")
    rec.add_argument("--frame-size", type=int, required=True)
    rec.add_argument("--format", choices=("cf32", "sc16", "ci8", "cu8"), default=None,
                     help="the samples of a raw stream (a SigMF recording names its own)")
    rec.add_argument("--scale", type=float, default=None,
                     help="what an integer component is multiplied by (default 2^-15 for sc16, 2^-7 for ci8 / cu8)")
    rec.add_argument("--features", default="all", metavar="all|used|3,5,...", help="as for extract")
    rec.add_argument("--device", type=int, default=None, help="GPU index (default: device 0)")
    rec.add_argument("--out", type=Path, default=None, help="the .mat file to write (default: FILE's stem + _features.mat)")
    rec.add_argument("--shift-hz", type=float, default=None, metavar="F",
                     help="tune first: add F Hz to every frequency (an emitter at +f wants -f); needs --decimate")
    rec.add_argument("--decimate", type=int, default=None, metavar="D", help="... low-pass and keep every D-th sample")
    rec.add_argument("--taps", type=int, default=None, metavar="T", help="taps of the low-pass (default 16 D + 1)")
    rec.add_argument("--resample", default=None, metavar="L/D",
                     help="instead of --decimate: change the rate by L / D through the rational resampler (L 1 ... 256, D 1 ... "
                          "4096; --taps then defaults to 16 max(L, D) + 1)")
    rec.add_argument("--rational", action="store_true",
                     help="with --annotation: the fraction L / D closest to R times the bandwidth over the sample rate, through "
                          "the rational resampler, instead of the next integer decimation")
    rec.add_argument("--annotation", type=int, default=None, metavar="K",
                     help="tune to the band of the recording's annotation K instead (its frequency edges)")
    rec.add_argument("--oversample", type=float, default=None, metavar="R",
                     help="with --annotation: decimate to R times the annotation's bandwidth (default 2); with --channels: "
                          "1 (critically sampled, the default) or 2")
    rec.add_argument("--recover", type=int, default=None, metavar="M", choices=(1, 2, 4, 8),
                     help="with the tuning flags: blind carrier recovery of every frame in front of the features -- the M-th-power "
                          "estimator (2 BPSK, 4 QPSK, 8 8PSK, 1 a bare carrier) takes gain, residual offset and phase out; the "
                          "output file gains carrier_hz, carrier_phase and carrier_quality; the frame size a power of two, 64 ... 4096")
    rec.add_argument("--recover-search-hz", type=float, default=None, metavar="F",
                     help="with --recover: the largest residual offset looked for, Hz (default: frame size / 16 bins of the M-th power)")
    rec.add_argument("--channels", type=int, default=None, metavar="C",
                     help="every channel of a raster of C (a power of two, 2 ... 256) through the polyphase filter bank; "
                          "--shift-hz then offsets the raster")
    rec.add_argument("--taps-per-channel", type=int, default=None, metavar="P",
                     help="with --channels: the prototype low-pass has C P taps (default 16)")
    rec.add_argument("--detect", action="store_true",
                     help="with --channels: occupancy detection -- the power of every (channel, frame) cell against the frame's "
                          "noise floor; only occupied cells get features (NaN elsewhere) and, with --model, labels")
    rec.add_argument("--threshold-db", type=float, default=None, metavar="X",
                     help="with --detect: a cell is occupied where its power is more than X dB over the floor (default 6)")
    rec.add_argument("--floor-quantile", type=float, default=None, metavar="Q",
                     help="with --detect: the floor of a frame is the channel power of rank int(Q (C - 1)) (default 0.25)")
    rec.add_argument("--model", default=None, metavar="ID|PATH",
                     help="with --channels: classify the cells (the occupied ones with --detect); as for classify; needs --root")
    rec.add_argument("--root", type=Path, default=None,
                     help="with --model: the project root whose calculated-features/ files the scaler is fitted on")
    rec.add_argument("--mode", choices=("training", "test"), default=None, help="with --model: as for classify (default test)")
    rec.add_argument("--annotate", type=Path, default=None, metavar="OUT.sigmf-meta",
                     help="with --channels and --detect: a copy of the meta file with one annotation per occupied segment")
    sc = sub.add_parser("scan", help="where the emitters of a SigMF recording are: Welch spectrogram, detection, annotations")
    sc.add_argument("file", type=Path, metavar="FILE",
                    help="X.sigmf-meta, X.sigmf-data or the stem X of a SigMF recording; or a raw stream (then --format)")
    sc.add_argument("--nfft", type=int, default=1024, metavar="N", help="bins: a power of two, 64 ... 4096 (default 1024)")
    sc.add_argument("--hop", type=int, default=None, metavar="H", help="samples between two segments (default N / 2)")
    sc.add_argument("--averages", type=int, default=16, metavar="A", help="segments summed into one row (default 16)")
    sc.add_argument("--window", choices=("hann", "rect"), default="hann")
    sc.add_argument("--threshold-db", type=float, default=6.0, metavar="X",
                    help="a bin is occupied where its power is more than X dB over the row's floor (default 6)")
    sc.add_argument("--floor-quantile", type=float, default=0.25, metavar="Q",
                    help="the floor of a row is the bin power of rank int(Q (N - 1)) (default 0.25)")
    sc.add_argument("--min-bins", type=int, default=2, metavar="B", help="bands narrower than B bins are dropped (default 2)")
    sc.add_argument("--merge-bins", type=int, default=2, metavar="G", help="bands at most G free bins apart are joined (default 2)")
    sc.add_argument("--min-rows", type=int, default=1, metavar="R", help="emitters shorter than R rows are dropped (default 1)")
    sc.add_argument("--format", choices=("cf32", "sc16", "ci8", "cu8"), default=None,
                    help="the samples of a raw stream (a SigMF recording names its own); edges are then in cycles per sample")
    sc.add_argument("--scale", type=float, default=None,
                    help="what an integer component is multiplied by (default 2^-15 for sc16, 2^-7 for ci8 / cu8)")
    sc.add_argument("--device", type=int, default=None, help="GPU index (default: the current device)")
    sc.add_argument("--out", type=Path, default=None, help="the .mat file to write (default: FILE's stem + _scan.mat)")
    sc.add_argument("--annotate", type=Path, default=None, metavar="OUT.sigmf-meta",
                    help="a copy of the meta file with one annotation per emitter, for `recording --annotation K --rational`")
    sy = sub.add_parser("synth", help="make the labelled data set on the GPU: mat-data/all_modulations.mat, or the feature files directly")
    sy.add_argument("--root", type=Path, default=None, help="project root (default: cwd)")
    sy.add_argument("--mods", nargs="+", default=None, metavar="MOD", help="modulations (default: the configuration's, with WGN)")
    sy.add_argument("--sps", default="8/1", metavar="U/V", help="U / V samples per symbol (default 8/1)")
    sy.add_argument("--pulse", choices=("rrc", "rect"), default="rrc")
    sy.add_argument("--beta", type=float, default=0.35, help="roll-off of the root-raised-cosine pulse (default 0.35)")
    sy.add_argument("--span", type=int, default=16, metavar="S", help="symbols the root-raised-cosine pulse spans (default 16)")
    sy.add_argument("--frames", type=int, default=None, metavar="F", help="frames per (modulation, SNR) (default: the configuration's)")
    sy.add_argument("--frame-size", type=int, default=None, metavar="N")
    sy.add_argument("--snr", default=None, metavar="lo:hi:step", help="the SNR grid in dB, hi included (default: the configuration's 16)")
    sy.add_argument("--cfo", type=float, default=0.0, metavar="X", help="largest carrier offset, cycles per sample: a frame draws its own in [-X, X)")
    sy.add_argument("--seed", type=int, default=0)
    sy.add_argument("--channel", default=None, metavar="PROFILE",
                    help="fading multipath: rayleigh | rician:K_DB | exp:N:SPACING:DECAY_DB | tworay:DELAY:DB (amcpy_amd/channel.py)")
    sy.add_argument("--doppler", type=float, default=0.0, metavar="F", help="maximum Doppler of --channel, cycles per sample")
    sy.add_argument("--sinusoids", type=int, default=16, metavar="S", help="sinusoids per path of --channel (default 16)")
    sy.add_argument("--cpm-h", default=None, metavar="H", help="modulation index of the MFSK names, a fraction such as 1/2 (default 1)")
    sy.add_argument("--bt", type=float, default=0.3, metavar="B", help="GMSK: bandwidth of the Gaussian filter, symbol rates (default 0.3)")
    sy.add_argument("--cpm-span", type=int, default=4, metavar="S", help="GMSK: symbols the phase pulse spans (default 4)")
    sy.add_argument("--features-only", action="store_true",
                    help="write calculated-features/{mod}_features.mat directly; the IQ is made a chunk at a time and never stored")
    sy.add_argument("--recover", type=int, default=None, metavar="M", choices=(1, 2, 4, 8),
                    help="with --features-only: every frame through blind carrier recovery of order M in front of the features, as "
                         "`recording --recover M` treats a recording's; named in the provenance record")
    sy.add_argument("--device", type=int, default=None, help="GPU index (default: current device)")
    return ap


def split_mods(mods):
    """--mods as a list of names: blanks or commas between them; None stays None."""
    return None if mods is None else [m for text in mods for m in str(text).split(",") if m]


def synth_config(args) -> tuple:
    """The configuration and the SNR grid the `synth` command's flags name."""
    from .config import with_modulations
    from .waveform import _label, parse_snr
    cfg = Config() if args.root is None else Config(paths=Paths(root=args.root))
    sig = cfg.signals
    if args.mods is not None:                 # a container variable for every name the configuration does not know
        sig = replace(sig, mat_info=with_modulations(sig, split_mods(args.mods)).mat_info)
    if args.frame_size is not None:
        sig = replace(sig, frame_size=args.frame_size)
    if args.frames is not None:
        sig = replace(sig, num_frames=args.frames)
    snr = None
    if args.snr is not None:
        snr = parse_snr(args.snr)
        sig = replace(sig, snr_values={i: _label(v) for i, v in enumerate(snr)})
    return replace(cfg, signals=sig), snr


def run_synth(args, compute=None, features=None, channel_compute=None, recover_compute=None) -> list:
    """The `synth` command (amcpy_amd/waveform.py, run_synth); ``compute`` / ``features`` / ``channel_compute`` /
    ``recover_compute``: injected over numpy (tests)."""
    from . import waveform
    cfg, snr = synth_config(args)
    try:
        fade = None
        if args.channel is not None:
            from .channel import parse_profile
            fade = dict(profile=parse_profile(args.channel), doppler=args.doppler, sinusoids=args.sinusoids)
            if channel_compute is not None:
                fade["compute"] = channel_compute
        from fractions import Fraction
        shape = dict(h=None if args.cpm_h is None else Fraction(args.cpm_h), bt=args.bt, span=args.cpm_span)
        return waveform.run_synth(cfg, mods=split_mods(args.mods), cpm=shape, sps=waveform.parse_sps(args.sps), pulse=args.pulse, beta=args.beta, span=args.span,
                                  snr=snr, cfo=args.cfo, seed=args.seed, features_only=args.features_only, recover=args.recover,
                                  device=None if args.device is None else f"cuda:{args.device}", compute=compute, features=features,
                                  channel=fade, recover_compute=recover_compute)
    except ValueError as e:
        raise SystemExit(f"synth: {e}")


def recording_survey(args):
    """The `recording` command's occupancy and classification flags -> ``None`` (none given: the features of every cell, as
    before) or ``{"detect": dict | None, "model": spec | None, "root": ..., "mode": ..., "annotate": path | None}``.  Every one
    of them needs --channels, and each the flag it belongs to."""
    given = [name for name, on in (("--detect", args.detect), ("--threshold-db", args.threshold_db is not None),
                                   ("--floor-quantile", args.floor_quantile is not None), ("--model", args.model is not None),
                                   ("--root", args.root is not None), ("--mode", args.mode is not None),
                                   ("--annotate", args.annotate is not None)) if on]
    if not given:
        return None
    if args.channels is None:
        raise SystemExit(f"{given[0]} needs --channels")
    for name in ("--threshold-db", "--floor-quantile", "--annotate"):
        if name in given and not args.detect:
            raise SystemExit(f"{name} needs --detect")
    for name in ("--root", "--mode"):
        if name in given and args.model is None:
            raise SystemExit(f"{name} needs --model")
    if args.model is not None and args.root is None:
        raise SystemExit("--model needs --root (the scaler is fitted on its calculated-features/ files)")
    detect = None
    if args.detect:
        detect = {"threshold_db": 6.0 if args.threshold_db is None else args.threshold_db,
                  "floor_quantile": 0.25 if args.floor_quantile is None else args.floor_quantile}
    return {"detect": detect, "model": args.model, "root": args.root, "mode": args.mode or "test", "annotate": args.annotate}


def annotate_segments(meta: dict, segments, frame_start, frame_size: int, decim: int, channel_freq_hz, labels=None,
                      class_names=None) -> dict:
    """A copy of the parsed meta file with one annotation per ``(channel, first_frame, last_frame)`` segment appended:
    ``core:sample_start`` / ``core:sample_count`` in input samples (a frame covers ``frame_size * decim`` of them),
    ``core:freq_lower_edge`` / ``core:freq_upper_edge`` = the channel's centre -/+ half the channel spacing, and -- with
    ``labels`` (C, K) and ``class_names`` -- ``core:label``, the name of the majority label (>= 0) of the segment's cells."""
    import numpy as np
    rate = (meta.get("global") or {}).get("core:sample_rate")
    if not rate:
        raise SystemExit("--annotate needs the global core:sample_rate (the channels' frequency edges)")
    half = float(rate) / len(channel_freq_hz) / 2.0
    anns = []
    for c, k0, k1 in segments:
        ann = {"core:sample_start": int(frame_start[k0]),
               "core:sample_count": int(frame_start[k1] - frame_start[k0]) + int(frame_size) * int(decim),
               "core:freq_lower_edge": float(channel_freq_hz[c]) - half, "core:freq_upper_edge": float(channel_freq_hz[c]) + half}
        if labels is not None and class_names is not None:
            seen = np.asarray(labels)[c, k0:k1 + 1]
            seen = seen[seen >= 0]
            if seen.size:
                ann["core:label"] = str(class_names[int(np.bincount(seen).argmax())])
        anns.append(ann)
    return with_annotations(meta, anns)


def with_annotations(meta: dict, new) -> dict:
    """A copy of the parsed meta file with the annotations ``new`` appended to its own, all in ``core:sample_start`` order
    (a stable sort: the recording's own annotations keep their order among equals, and come first)."""
    import copy
    out = copy.deepcopy(meta)
    out["annotations"] = sorted(list(out.get("annotations") or []) + list(new), key=lambda a: int(a.get("core:sample_start", 0)))
    return out


def annotate_emitters(meta: dict, emitters) -> dict:
    """A copy of the parsed meta file with one annotation per emitter of ``sigmf.scan_sigmf`` appended: ``core:sample_start``,
    ``core:sample_count``, ``core:freq_lower_edge``, ``core:freq_upper_edge`` and ``core:comment`` with the SNR -- what
    ``sigmf.tune_from_annotation`` reads.  The edges are only frequencies where the recording has a sample rate."""
    if not (meta.get("global") or {}).get("core:sample_rate"):
        raise SystemExit("--annotate needs the global core:sample_rate (the emitters' frequency edges)")
    return with_annotations(meta, [{"core:sample_start": int(e["sample_start"]), "core:sample_count": int(e["sample_count"]),
                                    "core:freq_lower_edge": float(e["freq_lower_edge"]),
                                    "core:freq_upper_edge": float(e["freq_upper_edge"]),
                                    "core:comment": f"amcpy_amd scan: snr_db={float(e['snr_db']):.1f}"} for e in emitters])


def run_scan(args, psd_compute=None, detect_compute=None) -> Path:
    """The `scan` command: sigmf.scan_sigmf of args.file -> args.out, a .mat file with psd, row_start, row_samples, freq_hz
    (where the meta gives a sample rate), floor, occupied, snr_db and the emitters as columns (emitter_sample_start,
    emitter_sample_count, emitter_freq_lower_edge, emitter_freq_upper_edge, emitter_snr_db); --annotate writes the emitters
    into a copy of the meta file.  ``psd_compute``, ``detect_compute``: injected (tests)."""
    import numpy as np
    from scipy.io import savemat
    from . import sigmf
    path = Path(args.file)
    if sigmf.is_sigmf(path):
        if args.format is not None:
            raise SystemExit("--format: a SigMF recording names its own datatype")
        rec = sigmf.read_meta(path)
        stem = Path(sigmf._stem(path))
    else:
        if args.format is None:
            raise SystemExit(f"{path} is no SigMF recording: --format cf32|sc16|ci8|cu8 says what its samples are")
        rec = sigmf.raw_recording(path, args.format)
        stem = path.with_suffix("")
    if args.annotate is not None and not (rec["meta"].get("global") or {}).get("core:sample_rate"):
        raise SystemExit("--annotate needs the global core:sample_rate (the emitters' frequency edges)")
    detect = {"threshold_db": args.threshold_db, "floor_quantile": args.floor_quantile, "min_bins": args.min_bins,
              "merge_bins": args.merge_bins, "min_rows": args.min_rows}
    got = sigmf.scan_recording(rec, nfft=args.nfft, hop=args.hop, averages=args.averages, window=args.window, detect=detect,
                               device=args.device, scale_samples=args.scale, psd_compute=psd_compute, detect_compute=detect_compute)
    found = got.pop("emitters")
    for key, kind in (("sample_start", np.int64), ("sample_count", np.int64), ("freq_lower_edge", np.float64),
                      ("freq_upper_edge", np.float64), ("snr_db", np.float64)):
        got["emitter_" + key] = np.array([e[key] for e in found], dtype=kind)
    out = Path(args.out) if args.out is not None else stem.with_name(stem.name + "_scan.mat")
    aside = out.with_name(out.name + f".{os.getpid()}.tmp")
    try:
        with open(aside, "wb") as fh:
            savemat(fh, got)
        os.replace(aside, out)
    finally:
        if aside.exists():
            aside.unlink()
    if args.annotate is not None:
        Path(args.annotate).write_text(json.dumps(annotate_emitters(rec["meta"], found), indent=1))
    print(f"{out}: {got['psd'].shape[0]} rows of {args.nfft} bins, {len(found)} emitters")
    return out


def recording_tune(args):
    """The `recording` command's tuning flags -> the ``tune`` of sigmf.extract_sigmf, or None.  The two forms exclude each
    other, and each flag needs the one it belongs to.  With --channels (:func:`recording_channelize`) there is no tuning:
    --shift-hz and --oversample then belong to the filter bank."""
    if args.channels is not None:
        if (args.decimate is not None or args.taps is not None or args.annotation is not None or args.resample is not None
                or args.rational):
            raise SystemExit("--channels excludes --decimate / --resample / --rational / --taps / --annotation")
        return None
    if args.taps_per_channel is not None:
        raise SystemExit("--taps-per-channel needs --channels")
    manual = args.shift_hz is not None or args.decimate is not None or args.taps is not None or args.resample is not None
    by_annotation = args.annotation is not None or args.oversample is not None or args.rational
    if manual and by_annotation:
        raise SystemExit("--shift-hz / --decimate / --resample / --taps and --annotation / --oversample / --rational exclude "
                         "each other")
    if args.resample is not None:
        if args.decimate is not None:
            raise SystemExit("--resample and --decimate exclude each other")
        try:
            L, D = (int(v) for v in str(args.resample).split("/"))
        except ValueError:
            raise SystemExit(f"--resample {args.resample!r}: expected L/D, two integers")
        return {"shift_hz": 0.0 if args.shift_hz is None else args.shift_hz, "resample": (L, D), "taps": args.taps}
    if manual:
        if args.decimate is None:
            raise SystemExit("--shift-hz and --taps need --decimate or --resample")
        return {"shift_hz": 0.0 if args.shift_hz is None else args.shift_hz, "decimate": args.decimate, "taps": args.taps}
    if by_annotation:
        if args.annotation is None:
            raise SystemExit("--oversample and --rational need --annotation")
        tune = {"annotation": args.annotation, "oversample": 2.0 if args.oversample is None else args.oversample}
        return {**tune, "rational": True} if args.rational else tune
    return None


def recording_channelize(args):
    """The `recording` command's filter-bank flags -> the ``channelize`` of sigmf.extract_sigmf, or None."""
    if args.channels is None:
        return None
    recording_tune(args)                                   # the flags --channels excludes
    over = 1 if args.oversample is None else args.oversample
    if over not in (1, 2):
        raise SystemExit("--oversample with --channels is 1 or 2")
    return {"channels": args.channels, "oversample": int(over),
            "taps_per_channel": 16 if args.taps_per_channel is None else args.taps_per_channel,
            "shift_hz": 0.0 if args.shift_hz is None else args.shift_hz}


def _survey_model(survey, device):
    """--model / --root / --mode -> (model, cols, mean, scale, class names by label): the scaler fitted as `classify` fits it."""
    import torch
    from .classifier import fit_scaler, load_model
    cfg = Config(paths=Paths(root=survey["root"]))
    model, _ = load_model(cfg, survey["model"])
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    _, mean, scale = fit_scaler(cfg, survey["mode"], dev)
    names = [None] * (max(cfg.signals.labels) + 1)
    for mod, lab in zip(cfg.signals.modulations_with_noise, cfg.signals.labels):
        names[int(lab)] = mod
    return model, [int(c) for c in cfg.features.used], mean, scale, names


def run_recording(args, compute=None, tune_compute=None, bank_compute=None, occupancy_compute=None, model=None,
                  class_names=None) -> Path:
    """The `recording` command: features and frame_start of args.file -> args.out (written aside, then renamed).  With
    --channels: features (C, K, 18), and channel_freq_hz (C,) where the meta file gives a sample rate (offset by the first
    capture's core:frequency where it has one).  With --detect / --model (:func:`recording_survey`) the file additionally holds
    power, floor and, as given, occupied, snr_db, labels and class_names (sigmf.survey_sigmf); --annotate writes the segments
    into a copy of the meta file.  ``occupancy_compute``, ``model`` (a callable) and ``class_names``: injected (tests)."""
    import numpy as np
    from scipy.io import savemat
    from . import _formats, sigmf
    from .feature_extraction import extract_raw_stream
    ids = resolve_features(args.features, Config())
    path = Path(args.file)
    tune = recording_tune(args)
    channelize = recording_channelize(args)
    survey = recording_survey(args)
    extra = {}
    recover = None
    if args.recover is not None:
        if tune is None:
            raise SystemExit("--recover needs the tuning flags (--shift-hz ... or --annotation): the frames of one emitter")
        recover = {"order": args.recover}
        if args.recover_search_hz is not None:
            recover["search_hz"] = args.recover_search_hz
    elif args.recover_search_hz is not None:
        raise SystemExit("--recover-search-hz needs --recover")
    if sigmf.is_sigmf(path):
        if args.format is not None:
            raise SystemExit("--format: a SigMF recording names its own datatype")
        if sigmf.is_rational_tune(tune):                      # resolved once: L and D go into the output file
            tune = sigmf.resolve_resample(sigmf.read_meta(path)["meta"], tune)
            extra["interp"], extra["decim"] = np.int64(tune[1]), np.int64(tune[2])
        got = None
        if survey is not None:
            kw = {}
            if survey["model"] is not None:
                if model is None:
                    model, kw["cols"], kw["mean"], kw["scale"], class_names = _survey_model(survey, args.device)
                extra["class_names"] = np.array([str(n) for n in class_names], dtype=object)
            got = sigmf.survey_sigmf(path, args.frame_size, channelize=channelize, detect=survey["detect"], model=model,
                                     device=args.device, feature_ids=ids, scale_samples=args.scale, bank_compute=bank_compute,
                                     occupancy_compute=occupancy_compute, compute=compute, **kw)
            feats, frame_start = got["features"], got["frame_start"]
            extra.update({k: got[k] for k in ("power", "floor", "occupied", "snr_db", "labels") if k in got})
        elif recover is not None:
            try:
                feats, frame_start, found = sigmf.extract_sigmf(path, args.frame_size, device=args.device, feature_ids=ids, scale=args.scale,
                                                                compute=compute, tune={**recording_tune(args), "recover": recover},
                                                                tune_compute=tune_compute)
            except ValueError as e:
                raise SystemExit(f"--recover: {e}")
            extra.update(found)
        else:
            feats, frame_start = sigmf.extract_sigmf(path, args.frame_size, device=args.device, feature_ids=ids, scale=args.scale,
                                                     compute=compute, tune=tune, tune_compute=tune_compute, channelize=channelize,
                                                     bank_compute=bank_compute)
        stem = Path(sigmf._stem(path))
        if channelize is not None:
            from fractions import Fraction
            from .bank import channel_frequencies
            meta = sigmf.read_meta(path)["meta"]
            rate = meta.get("global", {}).get("core:sample_rate")
            if rate:
                center = float((meta.get("captures") or [{}])[0].get("core:frequency", 0.0))
                shift = Fraction(channelize["shift_hz"]) / Fraction(float(rate))
                extra["channel_freq_hz"] = channel_frequencies(channelize["channels"], float(rate), center, shift)
        if survey is not None and survey["annotate"] is not None:
            decim = channelize["channels"] // channelize["oversample"]
            noted = annotate_segments(sigmf.read_meta(path)["meta"], got["segments"], frame_start, args.frame_size, decim,
                                      extra.get("channel_freq_hz"), got.get("labels"), class_names)
            Path(survey["annotate"]).write_text(json.dumps(noted, indent=1))
    else:
        if tune is not None or channelize is not None or survey is not None:
            raise SystemExit("the tuning flags need a SigMF recording (its meta file holds the sample rate)")
        if args.format is None:
            raise SystemExit(f"{path} is no SigMF recording: --format cf32|sc16|ci8|cu8 says what its samples are")
        feats = extract_raw_stream(path, args.frame_size, device=args.device, feature_ids=ids, sample_format=args.format,
                                   compute=compute, **_formats.scale_kw(args.format, args.scale, "scale", "scale8"))
        frame_start = args.frame_size * np.arange(feats.shape[0], dtype=np.int64)
        stem = path.with_suffix("")
    out = Path(args.out) if args.out is not None else stem.with_name(stem.name + "_features.mat")
    aside = out.with_name(out.name + f".{os.getpid()}.tmp")
    try:
        with open(aside, "wb") as fh:
            savemat(fh, {"features": feats, "frame_start": frame_start, **extra})
        os.replace(aside, out)
    finally:
        if aside.exists():
            aside.unlink()
    if channelize is not None:
        print(f"{out}: {feats.shape[0]} channels, {feats.shape[1]} frames of {args.frame_size} samples each")
    else:
        print(f"{out}: {feats.shape[0]} frames of {args.frame_size} samples")
    return out


def resolve_features(spec: str, cfg: Config):
    """--features: None (all 18) or the tuple of ids.  'used' = the columns the reference's preprocess_data and
    evaluate_by_snr read: FeatureConfig.used is taken there as 0-based column indices, so they are the ids used + 1."""
    spec = str(spec).strip().lower()
    if spec == "all":
        return None
    if spec == "used":
        return tuple(sorted({int(c) + 1 for c in cfg.features.used}))
    try:
        ids = [int(t) for t in spec.split(",") if t.strip() != ""]
    except ValueError:
        raise SystemExit(f"--features {spec!r}: expected all, used or a comma-separated list of ids 1 ... 18")
    bad = [i for i in ids if not 1 <= i <= 18]
    if not ids or bad:
        raise SystemExit(f"--features {spec!r}: expected all, used or a comma-separated list of ids 1 ... 18")
    ids = tuple(sorted(set(ids)))
    return None if ids == tuple(range(1, 19)) else ids


def _parse_devices(spec: str):
    from . import _lib
    if spec.strip().lower() == "all":
        n = _lib.load().amcx_device_count()
        if n < 1:
            raise SystemExit("--devices all: no gfx950 device is visible")
        return list(range(n))
    try:
        devs = [int(t) for t in spec.split(",") if t.strip() != ""]
    except ValueError:
        raise SystemExit(f"--devices {spec!r}: expected a comma-separated list of GPU indices, or 'all'")
    if not devs or min(devs) < 0:
        raise SystemExit(f"--devices {spec!r}: expected a comma-separated list of GPU indices, or 'all'")
    return devs


def _run_as_rank(cfg, args) -> None:
    """One rank of a launcher's job (torch.distributed.run: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set): the GPU of
    this rank's LOCAL_RANK, the process group, this rank's share of every modulation (run_extraction's several-rank
    path; rank 0 gathers and writes).  AMCX_DIST_BACKEND=gloo and AMCX_SHARE_GPU=1 rehearse it on a one-GPU box."""
    import torch
    import torch.distributed as dist
    from .feature_extraction import run_extraction
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", rank))
    n_dev = torch.cuda.device_count()
    if args.device is not None:
        dev = args.device
    elif os.environ.get("AMCX_SHARE_GPU", "0") == "1":
        dev = local % max(1, n_dev)
    else:
        dev = local
    problem = None if dev < n_dev else f"rank {rank}: no GPU {dev} ({n_dev} visible); one rank per GPU, or AMCX_SHARE_GPU=1"
    backend = os.environ.get("AMCX_DIST_BACKEND", "nccl")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    # Every rank says whether it can take part BEFORE the process group exists: a rank that has no device must not leave
    # the others waiting in the rendezvous until the store times out (a launcher that tears the job down on the first
    # failure hides this; one that does not, hangs).  The launcher's store carries one status word per rank.
    # (torch's own env:// rendezvous: it knows whether the launcher's agent already serves the store -- torch.distributed.run
    # does -- or rank 0 has to)
    store, _, _ = next(dist.rendezvous("env://", rank=rank, world_size=world))
    # A rank that dies before it has said anything (import error, bad environment) must not hold the others for the
    # store's default timeout (minutes): the exchange has a minute of its own, and running out of it is an error that
    # names the ranks that stayed silent.
    from datetime import timedelta
    wait_s = float(os.environ.get("AMCX_STATUS_TIMEOUT", "60"))
    store.set_timeout(timedelta(seconds=wait_s))
    store.set(f"amcx/status/{rank}", problem or "ok")
    problems, silent = [], []
    for r in range(world):
        try:
            word = store.get(f"amcx/status/{r}").decode()                            # get() waits for the key
        except Exception:
            silent.append(r)
            continue
        if word != "ok":
            problems.append(word)
    if silent:
        problems.append(f"rank(s) {silent} reported nothing within {wait_s:.0f} s (died before the rendezvous?)")
    # Every rank has now read every status: say so before anyone leaves.  Without a launcher rank 0 SERVES the store, and
    # a rank 0 that exits on a problem while others are still inside store.get() takes the store down under them: they
    # would die of a connection error instead of printing the collected message.
    try:
        store.add("amcx/status/read", 1)
        if problems and rank == 0:
            deadline = time.monotonic() + min(wait_s, 30.0)
            while int(store.add("amcx/status/read", 0)) < world - len(silent) and time.monotonic() < deadline:
                time.sleep(0.02)
    except Exception:
        pass
    if problems:
        raise SystemExit("; ".join(problems))
    store.set_timeout(timedelta(seconds=1800))                                        # the process group's own default
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", store=store, rank=rank, world_size=world, device_id=torch.device("cuda", dev))
    else:
        dist.init_process_group(backend, store=store, rank=rank, world_size=world)
    try:
        run_extraction(cfg, device=dev, verbose=rank == 0, resume=args.resume,
                       feature_ids=resolve_features(args.features, cfg))
    finally:
        dist.destroy_process_group()


def main(argv=None, *, skip_torch: bool = False) -> int:
    """``skip_torch``: load libamcx on the system HIP runtime without importing torch -- what the command line
    (`python -m amcpy_amd`, amcpy_amd/__main__.py) asks for, a second faster.  An in-process caller keeps the
    default: the library then binds to torch's runtime and the tensor entry points stay usable afterwards."""
    args = build_parser().parse_args(argv)
    if args.command == "recording":           # one file in, one file out: no project root, no torch (unless it tunes)
        from . import _lib
        recording_survey(args)                 # (its refusals, before anything is loaded)
        if skip_torch and recording_tune(args) is None and recording_channelize(args) is None:
            _lib.load(skip_torch=True)
        run_recording(args)
        return 0
    if args.command == "scan":                # tensors on torch's runtime: this command never skips the import
        run_scan(args)
        return 0
    if args.command == "synth":               # likewise
        run_synth(args)
        return 0
    cfg = Config() if args.root is None else Config(paths=Paths(root=args.root))
    sig = cfg.signals
    if args.frame_size is not None:
        sig = replace(sig, frame_size=args.frame_size)
    if args.num_frames is not None:
        sig = replace(sig, num_frames=args.num_frames)
    if args.snr_values is not None:
        sig = replace(sig, snr_values={i: str(v) for i, v in enumerate(args.snr_values)})
    if getattr(args, "mods", None) is not None:
        from .config import with_modulations
        try:
            sig = with_modulations(sig, split_mods(args.mods))
        except ValueError as e:
            raise SystemExit(f"--mods: {e}")
    cfg = replace(cfg, signals=sig)
    if args.command == "train":
        # tensors on torch's runtime: this command never skips the import
        from .train import run_training
        given = {name: v for name, v in (("epochs", args.epochs), ("batch_size", args.batch_size), ("learning_rate", args.lr),
                                         ("dropout", args.dropout), ("optimizer", args.optimizer), ("activation", args.activation),
                                         ("random_state", args.seed)) if v is not None}
        sweep = {key: [float(v) for v in text.split(",")] for key, text in (("lr", args.sweep_lr), ("dropout", args.sweep_dropout))
                 if text is not None}
        run_training(replace(cfg, training=replace(cfg.training, **given)), device=args.device, sweep=sweep or None)
        return 0
    if args.command == "classify":
        # tensors on torch's runtime: this command never skips the import
        from .classifier import run_classification
        run_classification(cfg, args.model, mode=args.mode, from_iq=args.from_iq, device=args.device)
        return 0
    if args.command == "quantize":
        from .quantize import run_quantization
        run_quantization(cfg, args.model, mode=args.mode, layout=args.layout, evaluate=args.evaluate, device=args.device,
                         normalize=not args.no_normalize)
        return 0
    if args.command == "extract":
        if args.devices is not None and args.device is not None:
            raise SystemExit("--device and --devices exclude each other")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 and "RANK" in os.environ:
            if args.devices is not None:
                raise SystemExit("--devices drives several GPUs from ONE process; under a launcher every rank has its own")
            _run_as_rank(cfg, args)
            return 0
        # One process, host containers in, files out: nothing here touches a torch tensor, so the import (a second of
        # start-up) can be skipped -- by loading the library first, not by changing the environment
        from . import _lib
        if skip_torch:
            _lib.load(skip_torch=True)
        from .feature_extraction import run_extraction
        ids = resolve_features(args.features, cfg)
        if args.devices is not None:
            run_extraction(cfg, devices=_parse_devices(args.devices), resume=args.resume, feature_ids=ids)
        else:
            run_extraction(cfg, device=args.device, resume=args.resume, feature_ids=ids)
    return 0


if __name__ == "__main__":
    sys.exit(main(skip_torch=True))
