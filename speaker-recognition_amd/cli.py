"""Command line -- mirrors the reference's ``src/speaker-recognition.py`` (:21-100):

    speaker-recognition.py -t enroll  -i "./bob/ ./mary/ ./person*" -m model.out
    speaker-recognition.py -t predict -i "./*.wav" -m model.out
    speaker-recognition.py -t predict -i "./*.wav" -m model.out --reject-threshold 0.5
    speaker-recognition.py -t enroll  -i "./bob/ ./mary/" -m model.out --covariance full
    speaker-recognition.py -t enroll  -i "./bob/ ./mary/" -m model.out --remove-silence
    speaker-recognition.py -t enroll  -i "./bob/ ./mary/" -m model.out --feature-norm warp --norm-window 301

Wav files in each input directory are labelled with the directory's basename; wildcard inputs
must be quoted (they go to glob).  Extra options (not in the reference) select the feature
framing / model order so that the BASELINE.json configs can be run from the shell.
"""
from __future__ import annotations

import argparse
import glob
import itertools
import os
import sys

from scipy.io import wavfile

from .interface import ModelInterface


def read_wav(fname):
    """src/gui/utils.py:10-13."""
    fs, signal = wavfile.read(fname)
    assert len(signal.shape) == 1, "Only Support Mono Wav File!"
    return fs, signal


def get_args(argv=None):
    parser = argparse.ArgumentParser(description="Speaker Recognition Command Line Tool",
                                     formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-t", "--task", help='Task to do: "enroll", "predict", "timeline", "diarize" or "embed"', required=True)
    parser.add_argument("-i", "--input", help="Input Files(to predict) or Directories(to enroll)", required=True)
    parser.add_argument("-m", "--model", help="Model file to save(in enroll) or use(in predict); diarize needs none", default=None)
    parser.add_argument("--mixtures", type=int, default=32, help="GMM order per speaker (default 32, gmmset.py:16)")
    parser.add_argument("--win-length-ms", type=float, default=32)
    parser.add_argument("--win-shift-ms", type=float, default=16)
    parser.add_argument("--fft-size", type=int, default=2048)
    parser.add_argument("--deltas", type=int, default=0, choices=[0, 1, 2], help="append delta orders")
    parser.add_argument("--no-lpc", action="store_true", help="MFCC half of mix_feature only (13 dims)")
    parser.add_argument("--seed", type=int, default=-1, help="EM initialisation seed (-1: random)")
    parser.add_argument("--covariance", choices=["diag", "full"], default="diag",
                        help="enroll: speaker model covariance (diag: the C++ back-end's models; full: the reference CLI's "
                             "scikit-learn GaussianMixture, skgmm.py)")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--gpus", type=int, default=1,
                        help="predict: shard the input files over this many GPUs from one process (0 = all visible)")
    parser.add_argument("--reject-threshold", type=float, default=None,
                        help="predict: open-set decision -- print None for a file whose best speaker's per-frame margin over the "
                             "UBM is below this (only for a model enrolled from a UBM)")
    parser.add_argument("--top-c", type=int, default=None,
                        help="predict: top-C Gaussian selection -- per frame only the N best components of the UBM are evaluated in "
                             "every speaker model (an approximation; default off; only for a diagonal model enrolled from a UBM)")
    parser.add_argument("--remove-silence", action="store_true",
                        help="drop silent frames before the feature stage (the reference's filters/silence.py, on the GPU). enroll: "
                             "stored in the model; predict: applied even if the model was enrolled without it")
    parser.add_argument("--feature-norm", choices=["warp", "cmn", "cmvn"], default=None,
                        help="short-time feature normalisation behind the feature stage, on the GPU (warp: feature warping; cmn / "
                             "cmvn: sliding-window mean / mean and variance). enroll: stored in the model; predict: the model's own "
                             "setting holds unless the flag is given")
    parser.add_argument("--norm-window", type=int, default=None, help="frames of the --feature-norm window (2 .. 1024; default 301)")
    parser.add_argument("--window", type=float, default=1.5, help="timeline: seconds of a window (default 1.5, the reference GUI's)")
    parser.add_argument("--hop", type=float, default=0.4, help="timeline: seconds between two windows (default 0.4)")
    parser.add_argument("--smooth", choices=["none", "hold", "viterbi"], default="hold",
                        help="timeline: none (the best model per window), hold (the GUI's rule: a new label shows once two windows in "
                             "a row agree) or viterbi (the best path under --switch-penalty)")
    parser.add_argument("--switch-penalty", type=float, default=None,
                        help="timeline, --smooth viterbi: the price of a label change, in nats per frame of window score (no default)")
    parser.add_argument("--min-duration", type=float, default=None, help="timeline, --smooth viterbi: seconds a turn lasts at least")
    parser.add_argument("--rttm", default=None, help="diarize: also write the segments to this file in the RTTM format")
    parser.add_argument("--speakers", type=int, default=None, help="diarize: exactly this many speakers")
    parser.add_argument("--max-speakers", type=int, default=None, help="diarize: at most this many speakers")
    parser.add_argument("--out", default=None, help="embed: the .npz to write (names, embeddings)")
    parser.add_argument("--penalty", type=float, default=1.0, help="diarize: the weight of the BIC penalty (default 1; larger: fewer speakers)")
    args = parser.parse_args(argv)
    if args.task != "diarize" and args.model is None:
        parser.error("the following arguments are required: -m/--model")
    if args.speakers is not None and args.max_speakers is not None:
        parser.error("--speakers and --max-speakers exclude each other")
    for name in ("speakers", "max_speakers"):
        if getattr(args, name) is not None and getattr(args, name) < 1:
            parser.error("--%s must be >= 1" % name.replace("_", "-"))
    if not args.penalty > 0:
        parser.error("--penalty must be > 0")
    if args.task == "embed" and args.out is None:
        parser.error("embed needs --out")
    return args


def task_enroll(input_dirs, output_model, args=None):
    m = _make_interface(args)
    input_dirs = [os.path.expanduser(k) for k in input_dirs.strip().split()]
    dirs = itertools.chain(*(glob.glob(d) for d in input_dirs))
    dirs = [d for d in dirs if os.path.isdir(d)]
    if len(dirs) == 0:
        print("No valid directory found!")
        sys.exit(1)
    training_stats = []
    for d in dirs:
        label = os.path.basename(d.rstrip("/"))
        wavs = sorted(glob.glob(d + "/*.wav"))
        if len(wavs) == 0:
            print("No wav file found in {0}".format(d))
            continue
        print("Label '{0}' has files: {1}".format(label, ", ".join(wavs)))
        total_len = 0
        for wav in wavs:
            fs, signal = read_wav(wav)
            print("   File '{}' has frequency={} and length={}".format(wav, fs, len(signal)))
            total_len += len(signal)
            m.enroll(label, fs, signal)
        training_stats.append((label, total_len))
    print("--------------------------------------------")
    for label, total_len in training_stats:
        print("Total length of training data for '{}' is {}".format(label, total_len))
    print("For best accuracy, please make sure all labels have similar amount of training data!")
    m.train()
    m.dump(output_model)


def _feature_norm_setting(args):
    """The ``feature_norm`` value the flags ask for, None without --feature-norm (--norm-window alone changes nothing)."""
    mode = getattr(args, "feature_norm", None)
    if mode is None:
        return None
    window = getattr(args, "norm_window", None)
    return mode if window is None else dict(mode=mode, window=window)


def task_predict(input_files, input_model, gpus=1, reject_threshold=None, remove_silence=False, top_c=None, feature_norm=None):
    m = ModelInterface.load(input_model)
    if remove_silence:              # the flag overrides a model enrolled without it; a model's own setting holds otherwise
        m.remove_silence = True
    if feature_norm is not None:    # likewise
        m.feature_norm = feature_norm
        m._norm_setting()
    out = []
    files = sorted(glob.glob(os.path.expanduser(input_files)))
    if top_c is not None:
        try:
            m._check_topc()
            if top_c < 1:
                raise ValueError("N must be >= 1")
        except ValueError as e:
            print("--top-c: %s" % e)
            sys.exit(2)
        if gpus != 1:
            print("--top-c: top-C scoring of a file list runs on one GPU (--gpus 1)")
            sys.exit(2)
        # every file in one batch (interface.predict_many_topc); with --reject-threshold the open-set rule decides on its sums
        labels = m.predict_many_topc([read_wav(f) for f in files], top_c, reject_threshold)
        for f, label in zip(files, labels):
            print(f, "->", label)
            out.append((f, label))
        return out
    if reject_threshold is not None:
        try:
            m._check_reject()
        except ValueError as e:
            print("--reject-threshold: %s" % e)
            sys.exit(2)
        if gpus != 1:
            print("--reject-threshold: the open-set decision of a file list runs on one GPU (--gpus 1)")
            sys.exit(2)
        # every file in one batch, decided on the device (interface.predict_many_with_reject)
        labels = m.predict_many_with_reject([read_wav(f) for f in files], reject_threshold)
        for f, label in zip(files, labels):
            print(f, "->", label)
            out.append((f, label))
        return out
    if gpus != 1:
        # every file in one utterance-sharded pass over the node's GPUs (interface.predict_many)
        labels = m.predict_many([read_wav(f) for f in files], gpus=gpus)
        for f, label in zip(files, labels):
            print(f, "->", label)
            out.append((f, label))
        return out
    for f in files:
        fs, signal = read_wav(f)
        label = m.predict(fs, signal)
        print(f, "->", label)
        out.append((f, label))
    return out


def task_timeline(input_files, input_model, args):
    """One line per segment of every input file: ``<file> <start s> <end s> <name or None>``."""
    m = ModelInterface.load(input_model)
    fn = _feature_norm_setting(args)
    if fn is not None:
        m.feature_norm = fn
        m._norm_setting()
    if args.smooth == "viterbi" and args.switch_penalty is None:
        print("--smooth viterbi needs --switch-penalty (there is no data-tuned default)")
        sys.exit(2)
    if args.reject_threshold is not None:
        try:
            m._check_reject()
        except ValueError as e:
            print("--reject-threshold: %s" % e)
            sys.exit(2)
    out = []
    for f in sorted(glob.glob(os.path.expanduser(input_files))):
        fs, signal = read_wav(f)
        segs = m.timeline(fs, signal, window_s=args.window, hop_s=args.hop, smooth=args.smooth, switch_penalty=args.switch_penalty,
                          min_duration_s=args.min_duration, reject_threshold=args.reject_threshold)
        for a, b, name in segs:
            print("%s %.2f %.2f %s" % (f, a, b, name))
        out.append((f, segs))
    return out


def task_diarize(input_files, args):
    """One line per segment of every input file: ``<file> <start s> <end s> <spkN>``; with --rttm the same segments in RTTM."""
    from .timeline import to_rttm
    m = _make_interface(args)
    kw = {} if args.switch_penalty is None else dict(switch_penalty=args.switch_penalty)
    out, rttm = [], []
    for f in sorted(glob.glob(os.path.expanduser(input_files))):
        fs, signal = read_wav(f)
        segs = m.diarize(fs, signal, penalty=args.penalty, n_speakers=args.speakers, max_speakers=args.max_speakers, window_s=args.window,
                         hop_s=args.hop, min_duration_s=args.min_duration, **kw)
        for a, b, name in segs:
            print("%s %.2f %.2f %s" % (f, a, b, name))
        rttm.append(to_rttm(segs, recording_id=os.path.splitext(os.path.basename(f))[0]))
        out.append((f, segs))
    if args.rttm:
        with open(args.rttm, "w") as fh:
            fh.write("".join(rttm))
    return out


def task_embed(input_files, input_model, args):
    """One embedding per input file through the network ``-m net.npz`` (xvector.XVector.save): writes ``names`` and ``embeddings``
    [n, E] to ``--out``.  Features: MFCC (+ LPC-15 unless --no-lpc or --deltas, as the other tasks), per-utterance CMVN, and the
    --win-length-ms / --win-shift-ms / --fft-size / --deltas / --feature-norm flags."""
    import numpy as np

    from .core import Batch, MfccExtractor
    from .xvector import XVector
    net = XVector.load(input_model)
    files = sorted(glob.glob(os.path.expanduser(input_files)))
    if not files:
        print("No wav file found!")
        sys.exit(1)
    wavs = [read_wav(f) for f in files]
    rates = sorted(set(fs for fs, _ in wavs))
    if len(rates) != 1:
        print("embed: the files have different sample rates (%s); embed them one rate at a time" % ", ".join(str(r) for r in rates))
        sys.exit(2)
    ex = MfccExtractor(rates[0], win_length_ms=args.win_length_ms, win_shift_ms=args.win_shift_ms, FFT_SIZE=args.fft_size,
                       n_lpc=0 if args.no_lpc or args.deltas > 0 else 15)
    emb = ex.embed_batch(net, Batch.from_pcm([sig for _, sig in wavs]), nd=args.deltas, norm=args.feature_norm,
                         norm_window=301 if args.norm_window is None else args.norm_window)
    with open(args.out, "wb") as fh:
        np.savez(fh, names=np.asarray(files), embeddings=emb)
    for f in files:
        print(f)
    return files, emb


def _make_interface(args):
    if args is None:
        return ModelInterface()
    fk = {}
    if args.win_length_ms != 32:
        fk["win_length_ms"] = args.win_length_ms
    if args.win_shift_ms != 16:
        fk["win_shift_ms"] = args.win_shift_ms
    if args.fft_size != 2048:
        fk["FFT_SIZE"] = args.fft_size
    return ModelInterface(gmm_order=args.mixtures, feature_kwargs=fk, diff=args.deltas > 0,
                          nd=max(1, args.deltas), lpc=not args.no_lpc and args.deltas == 0,
                          gmm_kwargs={"seed": args.seed}, covariance_type=args.covariance,
                          remove_silence=bool(getattr(args, "remove_silence", False)), feature_norm=_feature_norm_setting(args))


def main(argv=None):
    args = get_args(argv)
    from . import _lib
    _lib.set_device(args.device)
    if args.task == "enroll":
        task_enroll(args.input, args.model, args)
    elif args.task == "predict":
        task_predict(args.input, args.model, args.gpus, args.reject_threshold, args.remove_silence, args.top_c, _feature_norm_setting(args))
    elif args.task == "timeline":
        task_timeline(args.input, args.model, args)
    elif args.task == "diarize":
        task_diarize(args.input, args)
    elif args.task == "embed":
        task_embed(args.input, args.model, args)
    else:
        print('task must be "enroll", "predict", "timeline", "diarize" or "embed"')
        sys.exit(2)


if __name__ == "__main__":
    main()
