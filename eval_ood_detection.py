"""eval_ood_detection.py — same CLI as the reference (eval_ood_detection.py:15-51): every flag and default is kept, the rest is
additive.  Drives the MI355X-native hot path: model → loaders → the --score's record of mcm_amd/scores.py (`prepare` once, `score`
for the ID set and then per OOD set; what a score accepts on the command line is that record's to say) → AUROC / AUPR / FPR95 →
log + CSV.

Data.  `--root-dir` is honoured the way the reference's loaders read it (utils/train_eval_util.py:87-146):
`<root>/<in_dataset>/val/<class>/*` (ImageNet: `<root>/ImageNet/val`) for the ID set and
`<root>/ImageNet_OOD_dataset/{iNaturalist,SUN,Places,dtd/images}` for the OOD sets, read by
mcm_amd.folder.ImageFolderU8 (Pillow decode on the host; Resize + CenterCrop + ToTensor + Normalize on the
GPU, bit-exact with the reference's transform).  When a folder is missing — always the case offline — that
set is the seeded synthetic set of mcm_amd.synth with the reference's dataset size (generated in HBM, image i a
function of (seed, i) only, so per-rank shards see the same pixels), every set with its own seed, and the log,
the console and `<log_directory>/data_sources.json` say so per set.  The fine-grained
ID suites (bird200 / car196 / food101 / pet37) have their own archive formats in the reference
(dataloaders/*.py); only their synthetic form exists here.
Under `torchrun` each rank scores a contiguous shard and the shards are all-gathered (rank 0 reports)."""
import argparse
import logging
import os

import numpy as np

from mcm_amd.scores import METHODS, NO_REFINE, Run
from utils.common import get_num_cls, get_test_labels, setup_seed
from utils.detection_util import get_and_print_results, print_measures

# dataset sizes (external knowledge, as in the reference's loaders)
N_ID = {"ImageNet": 50000, "ImageNet10": 500, "ImageNet20": 1000, "ImageNet100": 5000,
        "bird200": 5794, "food101": 25250, "pet37": 3669, "car196": 8041}
N_OOD = {"iNaturalist": 10000, "SUN": 10000, "places365": 10000, "dtd": 5640,
         "ImageNet10": 500, "ImageNet20": 1000}


def parser():
    p = argparse.ArgumentParser(description="Evaluates MCM Score for CLIP",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--in_dataset", default="ImageNet", type=str,
                   choices=["ImageNet", "ImageNet10", "ImageNet20", "ImageNet100", "pet37", "food101",
                            "car196", "bird200"], help="in-distribution dataset")
    p.add_argument("--root-dir", default="datasets", type=str, help="root dir of datasets")
    p.add_argument("--name", default="eval_ood", type=str, help="unique ID for the run")
    p.add_argument("--seed", default=5, type=int, help="random seed")
    p.add_argument("--gpu", default=0, type=int, help="the GPU indice to use")
    p.add_argument("-b", "--batch-size", default=512, type=int, help="mini-batch size")
    p.add_argument("--T", type=int, default=1, help="temperature parameter")
    p.add_argument("--model", default="CLIP", type=str, help="model architecture")
    p.add_argument("--CLIP_ckpt", type=str, default="ViT-B/16",
                   choices=["ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px",
                            # OpenCLIP-trained (LAION-2B) checkpoints in HF layout: the exact GELU in both towers
                            "ViT-B/32-laion2b", "ViT-B/16-laion2b", "ViT-L/14-laion2b",
                            # ... and OpenCLIP's ViT-H/14: a 1280-wide vision tower with 80-wide heads
                            "ViT-H/14-laion2b"],
                   help="which pretrained img encoder to use")
    p.add_argument("--score", default="MCM", type=str,
                   choices=list(METHODS), help="score options")
    # Mahalanobis baseline (--score maha), reference eval_ood_detection.py:38-44
    p.add_argument("--feat_dim", type=int, default=512)
    p.add_argument("--normalize", type=bool, default=False)
    p.add_argument("--generate", type=bool, default=True)
    p.add_argument("--template_dir", type=str, default="img_templates")
    p.add_argument("--subset", default=False, type=bool)
    p.add_argument("--max_count", default=250, type=int)
    # additive
    p.add_argument("--weights", default=None, help="CLIP checkpoint (.safetensors / state_dict); default: seeded synthetic")
    p.add_argument("--dtype", default="fp16", choices=["bf16", "fp16", "fp16x2", "fp32"],
                   help="MFMA operand format of the vision tower (fp16 holds AUROC / AUPR to the fp32 arm at 1e-4 and, with threshold "
                        "refinement, FPR95 too; fp16x2 = every activation as a hi + lo fp16 pair: every score within one fp32 ulp of "
                        "the fp32 arm's at half the fp16 arm's speed, 3.7 x the fp32 arm's; the text tower is always fp32)")
    p.add_argument("--synthetic-weights", default="fp16-exact", choices=["fp16-exact", "fp32"],
                   help="without --weights: seeded parameters rounded to fp16 values, as the reference's checkpoints are "
                        "(default), or as drawn (fp32-valued: the 16-bit arms then run the split-weight GEMMs)")
    p.add_argument("--weight-operands", default="auto", choices=["auto", "single", "split"],
                   help="16-bit modes: one operand per GEMM weight, or W_hi + W_lo (exact for fp32-valued weights, twice "
                        "the GEMM work); auto = split exactly when a weight is not a number of the operand dtype")
    p.add_argument("--refine-threshold", default="auto", choices=["auto", "on", "exact", "off"],
                   help="re-score the images whose 16-bit score lies within a few noise widths of the FPR95 threshold with a "
                        "better arm (a few hundred images per run), so that FPR95 is the exact arithmetic's number and not merely "
                        "within 1 - 8 images of it (mcm_amd/refine.py).  on: --dtype fp16 re-scores with the split-activation arm "
                        "of the SAME handle (mcm_score_x2: within one fp32 ulp of the exact-fp32 arm's score, no second model in "
                        "HBM); --dtype bf16 with an exact-fp32 handle.  exact: additionally the handful of images within a few "
                        "fp32 ulps of the threshold go through an exact-fp32 handle, so the count is that arm's image for image.  "
                        "auto = on for --dtype fp16 / bf16 with an MCM-family --score.  Under torchrun every rank re-scores only "
                        "the window images of its own shard")
    p.add_argument("--host-metrics", action="store_true",
                   help="AUROC/AUPR/FPR95 with sklearn on the host (the reference's route) instead of the device kernels")
    p.add_argument("--synthetic-n", default=None, type=int, help="cap synthetic dataset sizes (smoke runs)")
    p.add_argument("--synthetic", action="store_true", help="never look under --root-dir; seeded synthetic sets only")
    p.add_argument("--templates", default=None, metavar="FILE",
                   help="prompt-ensemble bank (BASELINE config 5): one template per line with {c} or {}, or a .py "
                        "file in the style of the reference's utils/imagenet_templates.py (its 80-template list)")
    p.add_argument("--tokenizer-dir", default=None, help="directory with the checkpoint's vocab.json + merges.txt")
    p.add_argument("--data-dir", default="data", help="the reference's data/ directory (class-name files)")
    p.add_argument("--decoder", default=None, choices=["device", "pillow"],
                   help="how image files under --root-dir are decoded: pillow (default: Pillow in worker processes — the reference's "
                        "decoder, utils/train_eval_util.py:96-146 through torchvision's ImageFolder) or device (opt-in: JPEG entropy "
                        "decoding on host threads, the rest of libjpeg's work + Resize + CenterCrop on the GPU, Pillow for files that "
                        "are not Huffman YCbCr / grayscale JPEGs); same pixels either way")
    p.add_argument("--full-round-batch", action="store_true",
                   help="raise --batch-size to the next batch (within 4 x) at which every vision GEMM fills its last tile round of "
                        "the persistent grid on this device (mcm_amd.config.ClipGeometry.full_round_batches; ViT-B/16 on 256 CUs: "
                        "512 -> 665, +2.6 ... 3.2 %% images/sec; ViT-L/14: 256 -> 318; the chosen batch, or that there is none, is logged).  "
                        "Scores do not depend on the batch they were computed in")
    p.add_argument("--predict", nargs="?", type=int, const=5, default=0, metavar="K",
                   help="also return the K (1..8; 5 when given without a value) best-matching concepts of every image and their "
                        "softmax probabilities, from the same fused launch as the score: the ID set's top-1 / top-min(5,K) zero-shot "
                        "accuracy goes to the log (loader label i is taken to be concept i, as in the reference's loaders) and every "
                        "set's idx / prob / scores / labels to predictions_<set>.npz in the log directory (rank 0 under torchrun).  "
                        "Threshold refinement keeps working and patches the SCORES only: predictions are those of the arm that "
                        "scored the image first, so for the few hundred re-scored images prob[:,0] and -score differ in their last "
                        "bits.  Not available with --score maha / knn")
    p.add_argument("--maha-fit", default="host", choices=["host", "device"],
                   help="how --score maha fits its statistics: host (the reference's recipe: every training feature copied to the "
                        "host, torch.cov in float64 there, on rank 0 only under torchrun) or device (running fp64 sums in HBM, one "
                        "kernel per batch, every rank fitting its own shard of the training set and one all-reduce at the end; "
                        "same class means bit for bit, the covariance within its fp64 error budget)")
    p.add_argument("--knn-k", default=0, type=int, metavar="K",
                   help="--score knn (deep k-nearest neighbours, Sun et al. 2022: the distance from an image's unit-norm feature "
                        "to its K-th nearest neighbour among the training features, no prompt bank): K, 1..1024 and at most the "
                        "bank's rows; 0 (default) = min(1024, max(1, round(bank rows / 1281))), their k = 1000 at ImageNet-1k "
                        "scaled linearly.  The bank is the \"train\" set (--subset / --max_count as for --score maha), encoded by "
                        "every rank's shard and all-gathered")
    p.add_argument("--neg-words", default=None, metavar="FILE",
                   help="--score neglabel (NegLabel, Jiang et al. 2024: the share of an image's softmax mass on the ID prompts of a "
                        "bank extended by mined negative labels, against every group of negatives alone, averaged): the candidate "
                        "words, one per line (required with this score; empty lines, duplicates and ID class names are dropped)")
    p.add_argument("--neg-count", default=0, type=int, metavar="M", help="--score neglabel: keep the M candidates farthest from "
                   "the ID labels (0 = --neg-frac decides)")
    p.add_argument("--neg-frac", default=0.15, type=float, help="--score neglabel: keep round(FRAC x candidates) words")
    p.add_argument("--neg-quantile", default=0.95, type=float, metavar="Q",
                   help="--score neglabel: a candidate's distance from the ID labels is the Q quantile (linear interpolation) of its "
                        "similarities to them; the K - floor(Q (K - 1)) largest are needed, at most 1024")
    p.add_argument("--neg-groups", default=100, type=int, metavar="G",
                   help="--score neglabel: the kept words are cut into min(G, M) consecutive groups of floor(M / G); 1..1024")
    p.add_argument("--neg-T", default=0.01, type=float, help="--score neglabel: the softmax temperature (--T is ignored there)")
    p.add_argument("--gl-lambda", default=1.0, type=float, metavar="L",
                   help="--score GL-MCM (Miyai et al.: MCM plus a local term, the best softmax match of any single image patch's "
                        "value-path feature): the score is -(S_G + L S_L); default 1")
    p.add_argument("--vim-dim", default=0, type=int, metavar="D",
                   help="--score vim (ViM, Wang et al. 2022: alpha x the norm of an image's unit-norm feature outside the principal "
                        "subspace of the training features, minus the energy of its logits): the principal dimension D, "
                        "1..proj_dim - 1; 0 (default) = proj_dim // 2 below 768, 512 for 768 <= proj_dim < 2048, 1000 above.  The "
                        "training set is the \"train\" set (--subset / --max_count as for --score knn), every rank fitting its shard")
    p.add_argument("--vim-T", default=0.01, type=float, help="--score vim: the temperature of the logits (--T is ignored there)")
    p.add_argument("--ctx", default=None, metavar="FILE",
                   help="learned prompt contexts (CoOp, Zhou et al. 2022; LoCoOp, Miyai et al. 2023): the prompt bank of every "
                        "concept-matching score is CoOp's \"X X ... X classname.\" with the n_ctx context vectors of FILE in place "
                        "of the X — a CoOp / LoCoOp checkpoint (prompt_learner/model.pth.tar-N: state_dict['ctx'], shared "
                        "[n_ctx, width] or per class [K, n_ctx, width]), a state dict with 'ctx', or a .npy of the array.  Not with "
                        "--templates or --score maha / knn / neglabel")
    p.add_argument("--ctx-position", default="end", choices=["end", "middle", "front"],
                   help="--ctx: where the class name sits among the context vectors (CoOp's CLASS_TOKEN_POSITION)")
    p.add_argument("--ctx-T", default=0.01, type=float,
                   help="--ctx: the temperature of the MCM-family and GL-MCM scores (--T is ignored there: the contexts were "
                        "trained through softmax(100 cos), and --T is an int by the reference's contract)")
    return p


def process_args(argv=None):
    p = parser()
    args = p.parse_args(argv)
    method = METHODS[args.score]   # what this score accepts is the record's to say (mcm_amd/scores.py)
    asked = {"ctx": bool(args.ctx), "fp16x2": args.dtype == "fp16x2", "refine": args.refine_threshold in ("on", "exact"),
             "maha_fit": args.maha_fit == "device", "predict": bool(args.predict)}

    def refused(*switches):
        for switch in switches:
            if asked[switch] and switch in method.refuse:
                p.error(method.refuse[switch])

    if args.ctx:
        if args.templates:
            p.error("--ctx and --templates exclude each other (a learned context replaces the template's words)")
        if method.bank == "none":
            p.error(f"--ctx needs a score with a prompt bank: --score {args.score} has none")
        refused("ctx")
        if not (args.ctx_T > 0.0 and np.isfinite(args.ctx_T)):
            p.error("--ctx-T must be positive and finite")
        if method.ctx_T:
            args.T = args.ctx_T
    method.check_args(args, p.error)
    if not 0 <= args.knn_k <= 1024:   # (for every score: the flag is accepted with all of them)
        p.error("--knn-k K: K must be 1..1024 (0 = chosen from the bank size)")
    refused("fp16x2", "refine", "maha_fit", "predict")
    if args.refine_threshold == "auto":
        args.refine_threshold = method.auto_refine
    if args.predict and not 1 <= args.predict <= 8:
        p.error("--predict K: K must be 1..8")
    if args.decoder:
        os.environ["MCM_GPU_JPEG"] = "1" if args.decoder == "device" else "0"
    if args.templates:
        from mcm_amd.detection import read_templates

        args.templates = read_templates(args.templates)
    args.n_cls = get_num_cls(args)
    args.log_directory = f"results/{args.in_dataset}/{args.score}/{args.model}_{args.CLIP_ckpt}_T_{args.T}_ID_{args.name}"
    os.makedirs(args.log_directory, exist_ok=True)
    return args


def setup_log(args):
    log = logging.getLogger(__name__)
    log.handlers.clear()
    fmt = logging.Formatter("%(asctime)s : %(message)s")
    for h in (logging.FileHandler(os.path.join(args.log_directory, "ood_eval_info.log"), mode="w"),
              logging.StreamHandler()):
        h.setFormatter(fmt)
        log.addHandler(h)
    log.setLevel(logging.DEBUG)
    return log


# where the reference's loaders look (utils/train_eval_util.py:96-146), relative to --root-dir
OOD_DIRS = {"iNaturalist": ("ImageNet_OOD_dataset", "iNaturalist"), "SUN": ("ImageNet_OOD_dataset", "SUN"),
            "places365": ("ImageNet_OOD_dataset", "Places"), "dtd": ("ImageNet_OOD_dataset", "dtd", "images"),
            "ImageNet10": ("ImageNet10", "train"), "ImageNet20": ("ImageNet20", "val")}
SEEDS = {"id": 1, "train": 7, "iNaturalist": 11, "SUN": 12, "places365": 13, "dtd": 14, "ImageNet10": 15,
         "ImageNet20": 16}


def _loader(args, net, what, n, ood, sources):
    """The loader for one set: the real folder when it exists under --root-dir, else the seeded synthetic
    set (recorded in `sources`, which ends up in the log and in data_sources.json)."""
    from mcm_amd.synth import DevicePatternLoader

    if what in ("id", "train"):
        sub = (args.in_dataset, "val" if what == "id" else "train")
    else:
        sub = OOD_DIRS[what]
    path = os.path.join(args.root_dir, *sub)
    if not args.synthetic and os.path.isdir(path) and args.in_dataset.startswith("ImageNet"):
        from mcm_amd.folder import ImageFolderU8

        from mcm_amd.folder import FolderIndex

        index = FolderIndex(path)
        if what == "train" and args.subset and args.in_dataset == "ImageNet":
            # reference utils/train_eval_util.py:54-64: the first max_count images of every class — and, like
            # there, only for ImageNet (its ImageNet10/20/100 branch ignores `subset`)
            index = index.first_per_class(args.max_count)
        loader = ImageFolderU8(index, net, args.batch_size)
        sources[what] = {"kind": "folder", "path": path, "n": len(loader.dataset)}
        return loader
    if args.synthetic_n:
        n = min(n, args.synthetic_n)
    seed = SEEDS[what]
    sources[what] = {"kind": "synthetic", "n": n, "seed": seed, "why": f"{path} not found"}
    return DevicePatternLoader(n, net.geo.image_size, args.n_cls, args.batch_size, net.device, ood=ood, seed=seed)


def _note_pillow_files(net, sources, what, log):
    """How many files of the set just scored were decoded by Pillow inside the JPEG pipe (files that are not Huffman
    YCbCr / grayscale JPEGs, or that show any irregularity): recorded with the set's data source."""
    total = sum(p.fallback_images for p in net.__dict__.get("_jpeg_pipes", {}).values())
    seen = net.__dict__.get("_pillow_files_seen", 0)
    if what in sources and sources[what].get("kind") == "folder":
        sources[what]["decoded_by_pillow"] = total - seen
        if total - seen:
            log.debug(f"{what}: {total - seen} file(s) decoded by Pillow (not taken by the device JPEG route)")
    net.__dict__["_pillow_files_seen"] = total


def main(argv=None):
    import json

    import torch

    from mcm_amd import dist as mdist
    from mcm_amd.config import HUB_IDS
    from mcm_amd.engine import build_model

    args = process_args(argv)
    method = METHODS[args.score]
    setup_seed(args.seed)
    assert torch.cuda.is_available()
    ndev = torch.cuda.device_count()
    ws_env = int(os.environ.get("WORLD_SIZE", "1"))
    # more ranks than devices (a 1-GPU box running the 2-rank logic check): the ranks share devices and the
    # score all-gather goes over gloo with a host bounce, because RCCL refuses two ranks on one device
    # (LOCAL_WORLD_SIZE: the ranks of THIS node — a multi-node torchrun has WORLD_SIZE > device_count() with one GPU per rank)
    ws_local = int(os.environ.get("LOCAL_WORLD_SIZE", ws_env))
    rank, ws, local = mdist.init_from_env(backend="gloo" if ws_local > ndev else None)
    log = setup_log(args)
    dev = (local % ndev) if ws > 1 else args.gpu
    torch.cuda.set_device(dev)
    if args.full_round_batch:   # (resolved here, not in process_args: the tile rounds depend on THIS device's CU count)
        from mcm_amd.config import geometry

        cus = torch.cuda.get_device_properties(dev).multi_processor_count // 8 * 8   # the persistent GEMMs' grid
        better = geometry(args.CLIP_ckpt).full_round_batches(args.batch_size, 4 * args.batch_size, cus=cus) if cus >= 8 else []
        if better:
            log.debug(f"--full-round-batch: batch {args.batch_size} -> {better[0]} (every vision GEMM of {args.CLIP_ckpt} fills its last "
                      f"tile round on {cus} CUs; the activation workspace grows with it)")
            args.batch_size = better[0]
        else:
            log.debug(f"--full-round-batch: no batch in [{args.batch_size}, {4 * args.batch_size}] fills every GEMM's last tile round "
                      f"for {args.CLIP_ckpt} on {cus} CUs; keeping batch {args.batch_size}")
    # the split-activation workspace of an fp16 handle (include/mcm.h mcm_config.x2_max_batch): the whole run goes
    # through that arm with --dtype fp16x2 (full batch: twice the activation bytes); threshold refinement re-scores a few hundred
    # images, for which half the batch costs nothing extra; otherwise the workspace is not allocated at all
    will_refine = args.refine_threshold != "off" and method.refine
    x2_batch = 0 if args.dtype == "fp16x2" else (max(1, args.batch_size // 2) if (args.dtype == "fp16" and will_refine) else -1)
    net = build_model(args.CLIP_ckpt, weights=args.weights, device=dev, precision=args.dtype,
                      max_batch=args.batch_size, synthetic_regime=args.synthetic_weights,
                      weight_operands=args.weight_operands, x2_max_batch=x2_batch)
    net.eval()
    if args.dtype != "fp32":
        log.debug(f"vision GEMM weights: {net.weights_inexact} element(s) are not {args.dtype} numbers -> "
                  f"{'split-weight GEMMs (W_hi + W_lo, exact for the weight operand)' if net.split_weights else 'one operand per weight'}")
        if net.weights_inexact and not net.split_weights:
            log.debug("NOTE: --weight-operands single ROUNDS those weights: measured 1.5 - 2e-4 in AUROC against the fp32 "
                      "reference in this regime (DESIGN.md section 2.1)")
    if args.dtype == "bf16":
        log.debug("NOTE: bf16 operands do not hold the reference's AUROC / FPR95 to 1e-4 (measured 1e-4 ... 1e-3 against "
                  "HF fp32, DESIGN.md section 2.1); --dtype fp16 (the default) does")
    if args.ctx:
        from mcm_amd.prompts import load_context

        try:
            c = load_context(args.ctx)
        except (ValueError, OSError) as e:
            raise SystemExit(f"--ctx: {e}")
        if c.ctx.shape[-1] != net.geo.t_width:
            raise SystemExit(f"--ctx {args.ctx}: context vectors are {c.ctx.shape[-1]} wide, the text tower of {args.CLIP_ckpt} {net.geo.t_width}")
        log.debug(f"--ctx {args.ctx}: n_ctx = {c.n_ctx}, {'per-class (' + str(c.ctx.shape[0]) + ' classes)' if c.per_class else 'shared'} "
                  f"context, class name at the {args.ctx_position}"
                  + (f"; --T is ignored, the temperature is --ctx-T {args.ctx_T}" if method.ctx_T else ""))
    args.ckpt = HUB_IDS[args.CLIP_ckpt]  # reference utils/train_eval_util.py:19-22 (ckpt_mapping)
    if args.in_dataset == "ImageNet10":
        out_datasets = ["ImageNet20"]
    elif args.in_dataset == "ImageNet20":
        out_datasets = ["ImageNet10"]
    else:
        out_datasets = ["iNaturalist", "SUN", "places365", "dtd"]
    sources = {}
    test_loader = _loader(args, net, "id", N_ID[args.in_dataset], False, sources)
    test_labels = get_test_labels(args, test_loader)
    on_dev = not args.host_metrics and method.on_dev  # scores stay in HBM; three metrics come back

    def train_loader():
        n_train = min(N_ID[args.in_dataset], args.max_count * args.n_cls) if args.subset else N_ID[args.in_dataset]
        return _loader(args, net, "train", n_train, False, sources)

    run = Run(args, net, log, rank, ws, sources, test_labels, train_loader, on_dev)

    def score_set(loader, what, in_dist):   # (the one place every set of every score goes through)
        scores = method.score(run, state, loader, what, in_dist)
        if method.note_pillow:
            _note_pillow_files(net, sources, what, log)
        return scores

    state = method.prepare(run)
    in_score = score_set(test_loader, "id", True)
    net.warn_if_saturated(f"the ID set {args.in_dataset}")
    refiner, net32 = None, None
    refinable = method.refine and args.dtype in ("fp16", "bf16")  # (fp16x2 / fp32 runs ARE exact-grade arms; with
                                                                  # --host-metrics the scores are host arrays: refined in place too)
    if args.refine_threshold != "off" and refinable:
        from mcm_amd.detection import prompt_bank
        from mcm_amd.refine import Rescorer, ThresholdRefiner

        bank = prompt_bank(args, net, test_labels)  # (the 16-bit handle's text tower is exact fp32: one bank for every arm)
        set_loaders = {"id": test_loader}
        use_x2 = net.x2_max_batch > 0   # fp16 handles: the split-activation arm, same weights, same workspace
        if not use_x2 or args.refine_threshold == "exact":
            # the exact-fp32 arm over the same weights: the only re-scorer of a bf16 run (its batch as large as the window
            # asks for), the inner-window re-scorer of `exact` (a handful of images: a small workspace)
            net32 = build_model(args.CLIP_ckpt, weights=args.weights, device=dev, precision="fp32",
                                max_batch=min(args.batch_size, 256 if not use_x2 else 32), synthetic_regime=args.synthetic_weights)
        first = Rescorer(net.x2_scorer() if use_x2 else net32, bank, set_loaders, args.T, args.score)
        second = Rescorer(net32, bank, set_loaders, args.T, args.score) if (use_x2 and net32 is not None) else None
        refiner = ThresholdRefiner(first, rescore_exact=second)
        refiner.fit_id(in_score if on_dev else torch.from_numpy(in_score))
        how = "the split-activation arm of this handle" if use_x2 else "an exact-fp32 handle"
        log.debug("threshold refinement: 16-bit score noise (max over %d calibration images) %.2e, window +-%.2e around the "
                  "FPR95 threshold, %d ID images re-scored by %s" % (refiner.stats["calibration_images"],
                  refiner.stats["noise_max_abs"], refiner.stats["delta"], refiner.stats["rescored"]["id"], how))
        if second is not None:
            log.debug("threshold refinement, inner window +-%.2e: %d ID images re-scored by the exact-fp32 arm"
                      % (refiner.stats["delta2"], refiner.stats["rescored_exact"]["id"]))
    elif args.refine_threshold in ("on", "exact"):   # (an MCM-family score at an exact-grade --dtype, or --score maha)
        raise SystemExit(NO_REFINE)
    auroc_list, aupr_list, fpr_list = [], [], []
    result = {"in_score": in_score, "out_scores": {}, "rank": rank, "world_size": ws, "sources": sources,
              "log_directory": args.log_directory, "batch_size": args.batch_size}
    for out_dataset in out_datasets:
        log.debug(f"Evaluting OOD dataset {out_dataset}")
        ood_loader = _loader(args, net, out_dataset, N_OOD[out_dataset], True, sources)
        log.debug(f"data source: {sources[out_dataset]}")
        out_score = score_set(ood_loader, out_dataset, False)
        if refiner is not None:
            set_loaders[out_dataset] = ood_loader
            refiner.apply(out_dataset, out_score if on_dev else torch.from_numpy(out_score))
            log.debug(f"threshold refinement: {refiner.stats['rescored'][out_dataset]} images of {out_dataset} re-scored"
                      + (f", {refiner.stats['rescored_exact'][out_dataset]} of them by the exact-fp32 arm" if second is not None else ""))
        result["out_scores"][out_dataset] = out_score
        net.warn_if_saturated(out_dataset)
        if rank == 0:
            get_and_print_results(args, log, in_score, out_score, auroc_list, aupr_list, fpr_list, net=net)
    result["measures"] = {d: (a, p, f) for d, a, p, f in zip(out_datasets, auroc_list, aupr_list, fpr_list)}
    if rank == 0:
        log.debug("\n\nMean Test Results")
        print_measures(log, np.mean(auroc_list), np.mean(aupr_list), np.mean(fpr_list), method_name=args.score)
        import pandas as pd

        rows = {d: [100 * f, 100 * a, 100 * p] for d, f, a, p in zip(out_datasets, fpr_list, auroc_list, aupr_list)}
        rows["AVG"] = [100 * np.mean(fpr_list), 100 * np.mean(auroc_list), 100 * np.mean(aupr_list)]
        pd.DataFrame.from_dict(rows, orient="index", columns=["FPR95", "AUROC", "AUPR"]).round(2).to_csv(
            os.path.join(args.log_directory, f"{args.name}.csv"))
        synthetic = [k for k, v in sources.items() if v["kind"] == "synthetic"]
        if synthetic or not args.weights:
            log.debug(f"NOTE: synthetic inputs ({', '.join(synthetic) or 'none'}; weights: "
                      f"{'checkpoint' if args.weights else 'seeded synthetic'}) — these numbers are arithmetic "
                      "checks, not the paper's accuracy")
        with open(os.path.join(args.log_directory, "data_sources.json"), "w") as f:
            json.dump({"weights": args.weights or "seeded synthetic", "sets": sources}, f, indent=1)
    if refiner is not None:
        result["refine"] = dict(refiner.stats, rescorer="x2" if use_x2 else "fp32", rescored_by_this_rank=first.scored_here,
                                rank=rank, world_size=ws)
        with open(os.path.join(args.log_directory, f"refine_rank{rank}.json"), "w") as f:  # (every rank: who re-scored what)
            json.dump(result["refine"], f, indent=1)
        if net32 is not None:
            net32.close()
    # programmatic callers (tests) get the scores back; as device tensors they outlive the handle (torch owns them)
    net.close()
    if ws > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return result


if __name__ == "__main__":
    main()
