"""The score methods behind `--score`, one record each: what the method accepts on the command line, as data, and the three
steps `eval_ood_detection.py` drives it through — `check_args`, `prepare` (the fit or the bank, once per run) and `score` (one
set).  The records call the public functions of mcm_amd/detection.py; they add no arithmetic of their own.  DESIGN.md, "Adding a
score", says what goes where."""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Any, Callable, Dict

import numpy as np

from . import detection as det
from . import dist as mdist


@dataclass
class Run:
    """What a method's `prepare` and `score` see of one run of the driver."""
    args: Any
    net: Any
    log: Any
    rank: int
    ws: int
    sources: dict            # per set: where its images came from (ends up in data_sources.json)
    test_labels: list
    train_loader: Callable   # () -> the loader of the "train" set (--subset / --max_count applied), recorded in `sources`
    on_dev: bool             # scores stay on the device (the method allows it and --host-metrics is off)


@dataclass(frozen=True)
class Method:
    name: str
    needs_train: bool = False        # fits something on the "train" set
    bank: str = "prompt"             # "prompt": the prompt bank of the ID labels; "own": one the method builds; "none"
    # the switches process_args refuses with this method, with the refusal's text: "ctx" (--ctx), "fp16x2" (--dtype fp16x2),
    # "refine" (--refine-threshold on / exact), "maha_fit" (--maha-fit device), "predict" (--predict)
    refuse: Dict[str, str] = field(default_factory=dict)
    refine: bool = False             # has a re-scoring arm for threshold refinement; without one main() refuses on / exact
    auto_refine: str = "auto"        # what --refine-threshold auto resolves to in process_args ("auto": left to main())
    temperature: str = "--T"         # the flag that carries the method's temperature ...
    ctx_T: bool = False              # ... and whether --ctx-T takes its place under --ctx
    on_dev: bool = False             # scores can stay on the device (else host arrays)
    note_pillow: bool = False        # the per-set count of files decoded by Pillow is recorded (so far the MCM family only)
    check_args: Callable = lambda args, error: None      # the method's own flags: error(text) refuses
    prepare: Callable = lambda run: None                 # (run) -> state
    score: Callable = None                               # (run, state, loader, what, in_dist) -> scores of one set


ONLY_MAHA = {"maha_fit": "--maha-fit device needs --score maha (no other score fits anything)"}
NO_REFINE = "--refine-threshold on needs a 16-bit --dtype and an MCM-family --score"
NO_BANK_PREDICT = ("--predict needs a concept-matching --score (MCM, energy, max-logit, entropy, var): the training-set "
                   "baselines (--score maha, --score knn) have no prompt bank to match against")


def _positive(x):
    return x > 0.0 and np.isfinite(x)


def _clip_score(run, state, loader, what, in_dist):
    """`get_ood_scores_clip`, or with --predict `get_ood_predictions_clip`: the same scores, plus the set's predictions written to
    predictions_<what>.npz (rank 0) and, for the ID set, the zero-shot accuracy line."""
    args, net = run.args, run.net
    if not args.predict:
        return det.get_ood_scores_clip(args, net, loader, run.test_labels, in_dist=in_dist, device_out=run.on_dev)
    scores, idx, prob, labels = det.get_ood_predictions_clip(args, net, loader, run.test_labels, topk=args.predict, device_out=True)
    if run.rank == 0:
        idx_h, labels_h = idx.cpu().numpy(), labels.cpu().numpy()
        np.savez(os.path.join(args.log_directory, f"predictions_{what}.npz"), idx=idx_h, prob=prob.cpu().numpy(),
                 scores=scores.cpu().numpy(), labels=labels_h)
        if in_dist:
            k5 = min(5, args.predict)
            acc = det.zero_shot_accuracy(idx_h, labels_h, ks=(1, k5))
            run.log.debug(f"zero-shot ID accuracy: top-1 {100 * acc[1]:.2f} %, top-{k5} {100 * acc[k5]:.2f} % over {len(labels_h)} "
                          "images (loader label i is taken to be concept i, as in the reference's loaders)"
                          + ("" if args.weights else " — seeded synthetic weights: a plumbing check, not an accuracy"))
    return scores if run.on_dev else scores.cpu().numpy().astype(np.float32, copy=False)


def _glmcm_check(args, error):
    if not np.isfinite(args.gl_lambda):
        error("--gl-lambda must be finite")


def _glmcm_prepare(run):
    run.log.debug(f"--score GL-MCM: -(S_G + {run.args.gl_lambda} S_L) at T = {run.args.T}, {run.net.local_rows} patch rows per image")


def _maha_prepare(run):
    """(classwise_mean, precision), as reference eval_ood_detection.py:72-79 gets them.  world_size > 1: the host fit (a host-side
    float64 step over the training features) runs on rank 0 only; with --maha-fit device every rank fits its shard of the training
    set and the running sums are all-reduced (rank 0 writes the files).  Either way the two statistics are then broadcast and every
    rank scores its own shard of each test set."""
    import torch

    args, net = run.args, run.net
    args.feat_dim = net.geo.proj_dim
    os.makedirs(args.template_dir, exist_ok=True)
    if args.generate and (run.rank == 0 or args.maha_fit == "device"):
        (det.get_mean_prec_device if args.maha_fit == "device" else det.get_mean_prec)(args, net, run.train_loader())
    # like the reference (:77-78) the statistics are always read back from the files get_mean_prec wrote —
    # or that an earlier run wrote, which is what `--generate ""` (argparse's only falsy bool) is for
    stats = {"classwise_mean": torch.empty((args.n_cls, args.feat_dim)), "precision": torch.empty((args.feat_dim, args.feat_dim))}
    missing = None
    if run.rank == 0:
        for what in stats:
            f = os.path.join(args.template_dir, det.maha_file_name(args, what))
            if not os.path.exists(f):
                missing = f
                break
            stats[what] = torch.load(f, map_location="cpu").float().contiguous()
    if run.ws > 1:  # every rank learns whether rank 0 found the files BEFORE anybody waits in the broadcast
        ok = torch.tensor([0.0 if missing else 1.0])
        mdist.broadcast_tensors([ok], src=0)
        if float(ok[0]) == 0.0 and missing is None:
            missing = "the statistics files (see rank 0's message)"
    if missing:
        raise SystemExit(f"--generate is off and {missing} does not exist: run once with --generate True")
    if run.ws > 1:
        mdist.broadcast_tensors([stats["classwise_mean"], stats["precision"]], src=0)
    return stats["classwise_mean"], stats["precision"]


def _knn_prepare(run):
    """(bank, k): every rank encodes its shard of the training set; the bank is all-gathered and stays in HBM for the run."""
    args = run.args
    bank = det.get_knn_bank(args, run.net, run.train_loader())
    k = args.knn_k or det.knn_auto_k(len(bank))
    if k > len(bank):
        raise SystemExit(f"--knn-k {k} exceeds the bank's {len(bank)} rows")
    run.log.debug(f"--score knn: k = {k}{'' if args.knn_k else ' (auto)'}, bank of {len(bank)} unit-norm training features "
                  f"x {bank.shape[1]} ({run.sources['train']['kind']})")
    return bank, k


def _neglabel_check(args, error):
    if not args.neg_words:
        error("--score neglabel needs --neg-words FILE (one candidate word per line)")
    if args.neg_count < 0 or not 0.0 < args.neg_frac <= 1.0 or not 0.0 <= args.neg_quantile <= 1.0:
        error("--neg-count must be >= 0, --neg-frac in (0, 1], --neg-quantile in [0, 1]")
    if not 1 <= args.neg_groups <= 1024:
        error("--neg-groups G: G must be 1..1024")
    if not _positive(args.neg_T):
        error("--neg-T must be positive and finite")


def _neglabel_prepare(run):
    args, log = run.args, run.log
    with open(args.neg_words, encoding="utf-8") as f:
        words = f.read().splitlines()
    log.debug(f"--score neglabel: --T {args.T} is ignored; the softmax temperature is --neg-T {args.neg_T}")
    bank = det.get_neglabel_bank(args, run.net, run.test_labels, words)
    log.debug(f"--score neglabel: K = {bank['K']} ID labels, C = {bank['C']} candidate words from {args.neg_words}, "
              f"M = {bank['M']} kept, G = {bank['G']} groups of gs = {bank['gs']}; kept d from "
              f"{float(bank['d'].min()):.6f} to {float(bank['d'].max()):.6f} (quantile {args.neg_quantile})")
    return bank


def _vim_check(args, error):
    if args.vim_dim < 0:
        error("--vim-dim D: D must be 0 or 1..proj_dim - 1")
    if not _positive(args.vim_T):
        error("--vim-T must be positive and finite")


def _vim_prepare(run):
    args, net, log = run.args, run.net, run.log
    try:
        det.vim_principal_dim(net.geo.proj_dim, args.vim_dim)   # (before the training set is encoded)
        log.debug(f"--score vim: --T {args.T} is ignored; the temperature of the logits is --vim-T {args.vim_T}")
        fit = det.get_vim_fit(args, net, run.train_loader(), run.test_labels)
    except ValueError as e:  # a D the geometry does not allow; the subspace is not determined, or alpha is not a number
        raise SystemExit(str(e))
    lam = fit["eigenvalues"]
    log.debug(f"--score vim: D = {fit['D']}{'' if args.vim_dim else ' (auto)'}, R = {fit['R']}, n = {fit['n']} unit-norm "
              f"training features ({run.sources['train']['kind']}), alpha = {fit['alpha']:.6g}, lambda_D = {lam[fit['R']]:.6e}, "
              f"lambda_(D+1) = {lam[fit['R'] - 1]:.6e}, lambda_max = {lam[-1]:.6e}")
    if fit["alpha"] <= 0.0:
        log.debug("NOTE: alpha is not positive, so the residual enters the score with the wrong sign (seeded synthetic weights "
                  "can produce this; a trained checkpoint should not)")
    return fit


METHODS = {m.name: m for m in [
    *(Method(kind, refuse=ONLY_MAHA, refine=True, ctx_T=True, on_dev=True, note_pillow=True, score=_clip_score)
      for kind in ("MCM", "energy", "max-logit", "entropy", "var")),   # (the kinds of config.SCORE_KINDS, in the order of --help)
    Method("maha", needs_train=True, bank="none", refuse={"predict": NO_BANK_PREDICT}, prepare=_maha_prepare,
           score=lambda run, st, loader, what, in_dist: det.get_Mahalanobis_score(run.args, run.net, loader, *st, in_dist=in_dist)),
    Method("knn", needs_train=True, bank="none", refuse={**ONLY_MAHA, "refine": NO_REFINE, "predict": NO_BANK_PREDICT},
           prepare=_knn_prepare,
           score=lambda run, st, loader, what, in_dist: det.get_knn_score(run.args, run.net, loader, *st)),
    Method("neglabel", bank="own", temperature="--neg-T", check_args=_neglabel_check, prepare=_neglabel_prepare,
           refuse={**ONLY_MAHA, "refine": NO_REFINE,
                   "ctx": "--ctx is not available with --score neglabel (its mined negatives are template prompts and would sit in "
                          "another space than the ID rows)",
                   "predict": "--predict is not available with --score neglabel (its kernel returns group masses, not matched "
                              "concepts)"},
           score=lambda run, st, loader, what, in_dist: det.get_neglabel_score(run.args, run.net, loader, st)),
    Method("GL-MCM", auto_refine="off", ctx_T=True, check_args=_glmcm_check, prepare=_glmcm_prepare,
           refuse={**ONLY_MAHA, "fp16x2": "--score GL-MCM has no split-activation arm: --dtype fp16x2 is not available with it",
                   "refine": "--refine-threshold on / exact is not available with --score GL-MCM (no re-scoring arm for the local "
                             "term)",
                   "predict": "--predict is not available with --score GL-MCM"},
           score=lambda run, st, loader, what, in_dist: det.get_glmcm_scores(run.args, run.net, loader, run.test_labels)),
    Method("vim", needs_train=True, auto_refine="off", temperature="--vim-T", check_args=_vim_check, prepare=_vim_prepare,
           refuse={**ONLY_MAHA, "refine": NO_REFINE,
                   "predict": "--predict is not available with --score vim (its kernel returns a residual and an energy, not "
                              "matched concepts)"},
           score=lambda run, st, loader, what, in_dist: det.get_vim_score(run.args, run.net, loader, st)),
]}
