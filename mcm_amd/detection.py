"""The hot path's host side: `get_ood_scores_clip` and its reporting helpers, re-written
from scratch with the reference's signatures (utils/detection_util.py:209-265).

Differences from the reference that do not change results:
  * the prompt bank is tokenised and encoded ONCE per call instead of once per batch
    (reference :228-231 is loop-invariant);
  * the per-batch body runs as one fused native call (`net.score_images`), so only [b]
    scores exist per batch and they stay in HBM until the dataset is done (the reference
    copies the whole [b,K] softmax to the host every batch, :236);
  * under torch.distributed (one process per GPU) each rank scores a contiguous shard of the
    batches and the shards are all-gathered, so every rank returns the full vector in the
    reference's sample order.
"""
from __future__ import annotations

import numpy as np

from . import dist as mdist
from .abi import DEFINES
from .config import SCORE_KINDS
from .metrics import get_measures
from .tokenizer import load_tokenizer

PROMPT = "a photo of a {c}"  # reference utils/detection_util.py:228 (no trailing period)


def _tokenizer(args, net=None):
    """args.tokenizer_dir (additive) wins over args.ckpt.  The hash stand-in is allowed only with synthetic
    weights: the net records that itself (`net.synthetic_weights`, set by build_model / NativeCLIP), so a
    reference-shaped caller that has only `args.ckpt` and hands over a NativeCLIP built from a real checkpoint
    is refused instead of getting meaningless ids; a net that does not say falls back to `args.weights`."""
    src = getattr(args, "tokenizer_dir", None) or getattr(args, "ckpt", "")
    synthetic = getattr(net, "synthetic_weights", None)
    if synthetic is None:
        synthetic = not getattr(args, "weights", None)
    return load_tokenizer(src, allow_hash=bool(synthetic))


def encode_prompt_bank(args, net, test_labels):
    """`text_features` of the reference (:228-231): K prompts → [K,P] unit-norm fp32."""
    tokenizer = _tokenizer(args, net)
    text_inputs = tokenizer([PROMPT.format(c=c) for c in test_labels], padding=True, return_tensors="pt")
    return _unit_text_features(net, text_inputs)


# A small built-in template set for the prompt-ensemble bank (BASELINE config 5).  The reference
# ships OpenAI's 80 ImageNet templates as data but never uses them; pass your own list (e.g. read
# from that file) through `templates=` to reproduce the 80-template recipe.
DEFAULT_TEMPLATES = ["a photo of a {c}", "a blurry photo of a {c}", "a close-up photo of a {c}",
                     "a photo of the {c}", "a drawing of a {c}", "a bright photo of a {c}",
                     "a cropped photo of a {c}", "a photo of a small {c}", "a photo of a large {c}"]


def encode_prompt_ensemble(args, net, test_labels, templates=None):
    """CLIP zero-shot ensemble bank: per class, encode every template, normalise, average,
    re-normalise → [K,P].  Still a [K,P] bank, so the scoring path is unchanged."""
    templates = list(templates or DEFAULT_TEMPLATES)
    labels = list(test_labels)
    tokenizer = _tokenizer(args, net)
    prompts = [t.format(c=c) if "{c}" in t else t.format(c) for c in labels for t in templates]  # class-major
    tok = tokenizer(prompts, padding=True, return_tensors="pt")
    feats = _unit_text_features(net, tok)
    return net.reduce_bank(feats, len(labels), len(templates))


def _unit_text_features(net, tok):
    """`get_text_features(...).float()` followed by `/= norm` (reference :229-231).  A NativeCLIP fuses
    the normalisation; any other `net` honouring the HF contract is normalised here."""
    import inspect

    try:
        fused = "normalize" in inspect.signature(net.get_text_features).parameters
    except (TypeError, ValueError):
        fused = False
    if fused:
        return net.get_text_features(input_ids=tok["input_ids"], attention_mask=tok["attention_mask"],
                                     normalize=True)
    f = net.get_text_features(input_ids=tok["input_ids"], attention_mask=tok["attention_mask"]).float()
    return f / f.norm(dim=-1, keepdim=True).clamp_min(1e-30)


def prompt_bank(args, net, test_labels):
    """The [K,P] unit-norm bank for (labels, templates, tokenizer source), encoded once per `net`: a CLI run
    scores one ID and four OOD sets against the same bank (the reference re-encodes it every BATCH, :228-231;
    round 2 re-encoded it every dataset — 5 s per call with 80 templates x 1000 classes).  The key holds
    everything the bank depends on; T and the score kind do not enter it.  With `args.ctx` (a learned-context file, --ctx) the
    prompts are CoOp's, the context vectors in place of the template's words (mcm_amd/prompts.py), and the key also holds the
    file and `args.ctx_position`; without that attribute key and behaviour are what they always were."""
    templates = getattr(args, "templates", None)
    ctx = getattr(args, "ctx", None)
    key = (tuple(str(c) for c in test_labels), tuple(templates) if templates else None,
           getattr(args, "tokenizer_dir", None) or getattr(args, "ckpt", ""))
    if ctx:
        if templates:
            raise ValueError("a learned context (args.ctx) and a template ensemble (args.templates) exclude each other")
        key += (str(ctx), getattr(args, "ctx_position", None) or "end")
    cache = getattr(net, "_bank_cache", None)
    if cache is None:
        try:
            cache = net._bank_cache = {}
        except AttributeError:  # a net that refuses attributes: no caching
            cache = {}
    if key not in cache:
        cache.clear()  # one bank at a time (a bank is K x P floats; keep the handle small)
        if ctx:
            from .prompts import encode_context_bank

            cache[key] = encode_context_bank(args, net, test_labels)
        else:
            cache[key] = (encode_prompt_ensemble(args, net, test_labels, templates) if templates
                          else encode_prompt_bank(args, net, test_labels))
    return cache[key]


def read_templates(path):
    """Prompt templates from a user file (`--templates`).  Two formats:
      * a text file, one template per line, the class name marked `{c}` or `{}`;
      * a Python file in the style of the reference's utils/imagenet_templates.py (a list of
        `lambda c: f'a bad photo of a {c}.'`): the f-string bodies of the file's FIRST list are
        extracted, nothing is executed."""
    import re

    text = open(path, encoding="utf-8").read()
    if path.endswith(".py"):
        m = re.search(r"=\s*\[(.*?)^\]", text, re.S | re.M)  # the first list only (the 80 templates); the
        text = m.group(1) if m else text                      # file's later subsets repeat entries
        out = [m.group(2) for m in re.finditer(r"""f(['"])((?:(?!\1).)*\{c\}(?:(?!\1).)*)\1""", text)]
    else:
        out = [ln.strip() for ln in text.splitlines() if ln.strip() and not ln.lstrip().startswith("#")]
    if not out or not all(("{c}" in t) or ("{}" in t) for t in out):
        raise ValueError(f"{path}: no templates found, or a template without a {{c}} / {{}} placeholder")
    return out


def get_ood_scores_clip(args, net, loader, test_labels, in_dist=False, device_out=False):
    """Scores every sample of `loader` against the concept bank `test_labels`.

    Same contract as reference utils/detection_util.py:209-249: reads `args.ckpt`,
    `args.model`, `args.score`, `args.T`; `loader` yields `(images[b,3,S,S] fp32, labels)`
    in dataset order; returns float32 ndarray `[len(loader.dataset)]` of *negated*
    confidences (lower = more ID) for MCM / max-logit / energy / var and the entropy for
    'entropy'.  `in_dist` and the labels are unused, as in the reference.
    `device_out=True` (an addition) returns the same vector as a device tensor instead, for
    `get_and_print_results(..., net=net)` to evaluate without a host round trip.
    """
    import torch

    if getattr(args, "model", "CLIP") != "CLIP":
        raise ValueError(f"unsupported --model {args.model!r} (the reference only defines CLIP)")
    if args.score not in SCORE_KINDS:
        raise ValueError(f"unsupported --score {args.score!r} for get_ood_scores_clip")
    if not hasattr(net, "score_images"):
        raise TypeError("net must be a mcm_amd NativeCLIP (fused score_images path); "
                        "there is no eager fallback")
    with torch.no_grad():
        text_features = prompt_bank(args, net, test_labels)
        return _scores_over_shards(loader, text_features.device, device_out,
                                   lambda images: net.score_images(images, text_features, float(args.T), args.score))


def _scores_over_shards(loader, device, device_out, score_batch):
    """The sharding and gathering of `get_ood_scores_clip`, for any per-batch score `score_batch(images) -> [b]` device
    tensor: this rank's contiguous index shard of `loader.dataset` (batch-range shards where the loader cannot be split by
    index), all-gathered in dataset order where a process group exists.  Call under `torch.no_grad()`.  Returns the
    [len(loader.dataset)] scores as a device tensor (`device_out`) or a float32 ndarray."""
    import torch

    n_total = len(loader.dataset)
    batches, by_index = _shard_batches(loader, n_total, None, opaque_ok=True)
    parts = [score_batch(images) for images, _labels in batches]
    if by_index:  # (also in a 1-rank group: the collective really runs — RCCL on a GPU box)
        full = _gather_shards(parts, n_total, device)
    else:  # batch-range shards of an opaque loader: sizes follow the batch split
        local = torch.cat(parts) if parts else torch.empty(0, dtype=torch.float32, device=device)
        full = _gather_batch_shards(local, n_total, mdist.world()[1]).detach()[:n_total]
    if device_out:
        return full
    return full.cpu().numpy().astype(np.float32, copy=False).copy()


def get_glmcm_scores(args, net, loader, test_labels, device_out=False):
    """`--score GL-MCM` (Miyai et al.): per sample -(S_G + lambda S_L) against the concept bank `test_labels`, S_G the MCM
    term of the global feature and S_L the best softmax match of any single patch's local feature
    (`net.score_images_glmcm`); reads `args.T` and `args.gl_lambda` (default 1).  Larger = more OOD.  The
    prompt bank, the per-rank index shards and the all-gather are those of `get_ood_scores_clip`; every sample is scored.
    Returns a float32 ndarray [len(loader.dataset)], or the device tensor with `device_out=True`."""
    import torch

    if not hasattr(net, "score_images_glmcm"):
        raise TypeError("get_glmcm_scores needs a net with score_images_glmcm (a NativeCLIP); there is no eager fallback")
    lam = float(getattr(args, "gl_lambda", 1.0))
    with torch.no_grad():
        text_features = prompt_bank(args, net, test_labels)
        return _scores_over_shards(loader, text_features.device, device_out,
                                   lambda images: net.score_images_glmcm(images, text_features, float(args.T), lam))


def get_ood_predictions_clip(args, net, loader, test_labels, topk=5, device_out=False):
    """`get_ood_scores_clip` that also says which concepts every sample matched: the zero-shot prediction a consumer of
    the reference takes from the [b,K] softmax it copies to the host every batch (utils/detection_util.py:232-236), here
    from the same fused launch that writes the score (`net.score_images(..., topk=)`), so [b,K] still never exists.

    Same prompt-bank cache, same contiguous per-rank shards and same sample order as `get_ood_scores_clip`.  Returns
    `(scores [n] fp32, idx [n,topk] int32, prob [n,topk] fp32, labels [n] int64)`: the scores `get_ood_scores_clip`
    returns, the bank rows of the topk largest similarities per sample (best first, ties to the lower row, -1 where
    nothing is left), their softmax(sim / T), and the loader's own labels in the same order — ndarrays, or device
    tensors with `device_out=True`.  Under world_size > 1 the four arrays are all-gathered to every rank; the loader
    must then be one `shard_loader` can split by sample index."""
    import torch

    if getattr(args, "model", "CLIP") != "CLIP":
        raise ValueError(f"unsupported --model {args.model!r} (the reference only defines CLIP)")
    if args.score not in SCORE_KINDS:
        raise ValueError(f"unsupported --score {args.score!r} for get_ood_predictions_clip")
    if not hasattr(net, "score_images"):
        raise TypeError("net must be a mcm_amd NativeCLIP (fused score_images path); there is no eager fallback")
    topk = int(topk)
    n_total = len(loader.dataset)
    with torch.no_grad():
        text_features = prompt_bank(args, net, test_labels)
        dev = text_features.device
        batches, _ = _shard_batches(loader, n_total, "get_ood_predictions_clip under world_size > 1 needs a loader with "
                                    ".shard(lo, hi) or a torch DataLoader over a map-style dataset")
        parts = ([], [], [], [])
        for images, labels in batches:
            s, i, p = net.score_images(images, text_features, float(args.T), args.score, topk=topk)
            for dst, t in zip(parts, (s, i, p, torch.as_tensor(labels).reshape(-1).to(device=dev, dtype=torch.int64))):
                dst.append(t)
        full = tuple(_gather_shards(p, n_total, dev, width, dtype) for p, (width, dtype) in zip(parts, (
            (None, torch.float32), (topk, torch.int32), (topk, torch.float32), (None, torch.int64))))
    if device_out:
        return full
    return tuple(t.cpu().numpy().copy() for t in full)


def zero_shot_accuracy(idx, labels, ks=(1, 5)):
    """Top-k zero-shot accuracy from `get_ood_predictions_clip`'s `idx` [n,topk] and `labels` [n]: {k: fraction of the
    samples whose label is among their first k indices}.  A -1 slot (no candidate) never matches; a k beyond the topk
    the indices were computed with cannot be answered and raises."""
    idx = np.asarray(idx.detach().cpu() if hasattr(idx, "detach") else idx)
    labels = np.asarray(labels.detach().cpu() if hasattr(labels, "detach") else labels).reshape(-1)
    if idx.ndim != 2 or idx.shape[0] != labels.shape[0]:
        raise ValueError(f"idx must be [n,topk] and labels [n], got {idx.shape} and {labels.shape}")
    out = {}
    for k in ks:
        if not 1 <= int(k) <= idx.shape[1]:
            raise ValueError(f"top-{k} accuracy needs 1 <= k <= topk = {idx.shape[1]}")
        first = idx[:, :int(k)].astype(np.int64)
        hit = ((first == labels.astype(np.int64)[:, None]) & (first >= 0)).any(axis=1)
        out[int(k)] = float(hit.mean()) if hit.size else float("nan")
    return out


def shard_loader(loader, lo: int, hi: int):
    """A loader over samples [lo, hi) of `loader.dataset`, in order — a rank's shard BEFORE any decode happens.
    The build's own loaders have `.shard`; a torch-style DataLoader (map-style `dataset`, `batch_size`, the reference's
    kind: utils/train_eval_util.py:96-146, shuffle=False) is re-built over `Subset(dataset, range(lo, hi))` with the same
    batch size, workers and collate function; anything else returns None (the caller falls back to skipping batches)."""
    if hasattr(loader, "shard"):
        return loader.shard(lo, hi)
    ds, bs = getattr(loader, "dataset", None), getattr(loader, "batch_size", None)
    if ds is None or not bs or not hasattr(ds, "__getitem__"):
        return None
    try:
        from torch.utils.data import DataLoader, Subset
    except Exception:
        return None
    if not isinstance(loader, DataLoader):
        return None
    kw = dict(batch_size=bs, shuffle=False, num_workers=loader.num_workers, collate_fn=loader.collate_fn,
              pin_memory=loader.pin_memory, drop_last=False)
    if loader.num_workers > 0:
        kw.update(prefetch_factor=loader.prefetch_factor, persistent_workers=False)
    return DataLoader(Subset(ds, range(lo, hi)), **kw)


def _my_range(n):
    """This rank's contiguous share [lo, hi) of n items in order: all of them for one rank, else its `shard_range`."""
    rank, ws = mdist.world()
    return mdist.shard_range(n, rank, ws) if ws > 1 else (0, n)


_BY_INDEX = "--score {} under world_size > 1 needs a loader that can be sharded by index"


def _shard_batches(loader, n, what, opaque_ok=False):
    """(batches, by_index): this rank's (images, labels) batches of samples [0, n) of `loader.dataset`, in order — all of them
    for one rank, the rank's `shard_range` under world_size > 1, the last batch cut to the range's end, images and labels alike
    (by_index: `_gather_shards` joins the ranks' results).  A loader `shard_loader` cannot split by index is refused with the
    TypeError text `what` (raised by this call and not by the first batch) — or, with `opaque_ok`, walked by every rank, which
    keeps its `shard_range` of the BATCHES (every rank still pays its decode; by_index is False: only the owning rank knows its
    shard's size, `_gather_batch_shards` joins them)."""
    lo, hi = _my_range(n)
    batches = shard_loader(loader, lo, hi) if mdist.world()[1] > 1 else loader
    if batches is None:
        if not opaque_ok:
            raise TypeError(what)
        blo, bhi = _my_range(len(loader))
        return (batch for i, batch in enumerate(loader) if blo <= i < bhi), False

    def walk():
        seen = 0
        for images, labels in (batches if hi > lo else ()):
            if seen >= hi - lo:
                break
            if images.shape[0] > hi - lo - seen:
                images, labels = images[: hi - lo - seen], labels[: hi - lo - seen]
            yield images, labels
            seen += images.shape[0]

    return walk(), True


def _feature_home(args, net):
    """(device, width) of the feature rows of `net`, for the empty shard of a rank without samples."""
    P = getattr(getattr(net, "geo", None), "proj_dim", None) or getattr(args, "feat_dim", 0)
    return getattr(net, "device", None) or "cpu", int(P)


def _gather_shards(parts, n_total, device, width=None, dtype=None):
    """What `_shard_batches` produced by index on every rank, in dataset order, on every rank: this rank's `parts` joined (no
    part: an empty tensor of `dtype`, fp32 by default, on `device`: [0] values or [0, width] rows), all-gathered where a process
    group exists, cut to n_total."""
    import torch

    dtype = dtype or torch.float32
    local = torch.cat(parts) if parts else torch.empty((0,) if width is None else (0, width), dtype=dtype, device=device)
    if mdist.group_active():
        scores = width is None and dtype == torch.float32
        local = (mdist.all_gather_scores if scores else mdist.all_gather_rows)(local, n_total)
    return local.detach()[:n_total]


def _score_loader(loader, n, what, device, fn):
    """The body of the feature-space scores: samples [0, n) of `loader` scored by `fn(images) -> [b]` device scores, batch by
    batch over this rank's shard (`what`: the --score named where the loader cannot be sharded by index), gathered to every
    rank: a float32 ndarray [n]."""
    import torch

    with torch.no_grad():
        out = [fn(images) for images, _labels in _shard_batches(loader, n, _BY_INDEX.format(what))[0]]
    return _gather_shards(out, n, device).cpu().numpy().astype(np.float32)


def get_mean_prec(args, net, train_loader):
    """Mahalanobis fit: (classwise_mean [n_cls, feat_dim], precision [feat_dim, feat_dim]), with the
    results and side effects of reference utils/detection_util.py:146-174.  Two behaviours of the
    reference that a drop-in has to reproduce, stated as the maths they amount to:

      * the reference records, per label, the index of the BATCH a sample came from and then uses those
        numbers as row indices into the matrix of all features (:159-160,164-165).  So class c's "mean"
        is  sum_b n[c,b] * F[b] / sum_b n[c,b],  n[c,b] = samples of class c in batch b, F[b] = the b-th
        feature ROW.  It is computed here as one [n_cls, n_batches] x [n_batches, P] product in float64;
      * one covariance over all features, inverted in float64, cast to float32 (:168-169).

    Features come from `net.get_image_features(pixel_values=...)` — the plain HF contract (raw
    projections; L2-normalised when args.normalize).  Writes the reference's two .pt files."""
    import os

    import torch

    feats, counts = [], []
    with torch.no_grad():
        for images, labels in train_loader:
            f = net.get_image_features(pixel_values=images).float()
            if args.normalize:
                f = f / f.norm(dim=-1, keepdim=True)
            feats.append(f.cpu())
            # labels >= n_cls are ignored, like the reference's per-class loop (:161-166) never visits them
            lab = labels.detach().cpu().numpy() if hasattr(labels, "detach") else np.asarray(labels)
            counts.append(np.bincount(lab.astype(np.int64).reshape(-1), minlength=args.n_cls)[: args.n_cls])
    F = torch.cat(feats)                                    # [n, P] float32, dataset order
    n_cb = torch.from_numpy(np.stack(counts, axis=1).astype(np.float64))  # [n_cls, n_batches]
    rows = F[: n_cb.shape[1]].double()                       # the rows the reference's indices select
    classwise_mean = ((n_cb @ rows) / n_cb.sum(dim=1, keepdim=True)).float()
    if args.normalize:
        classwise_mean = classwise_mean / classwise_mean.norm(dim=-1, keepdim=True)
    precision = torch.linalg.inv(torch.cov(F.T.double())).float()
    print(f"cond number: {torch.linalg.cond(precision)}")
    tdir = getattr(args, "template_dir", None)
    if tdir:
        os.makedirs(tdir, exist_ok=True)
        for what, t in (("classwise_mean", classwise_mean), ("precision", precision)):
            torch.save(t, os.path.join(tdir, maha_file_name(args, what)))
    return classwise_mean, precision


def get_mean_prec_device(args, net, train_loader, return_cov=False):
    """`get_mean_prec` as a streaming, sharded fit: the same results and files, from constant-size running statistics
    that stay in HBM until the training set ends (`net.maha_fit_accumulate`: one fp64 kernel per batch) instead of every
    feature on the host.  `net` must have `maha_fit_state` / `maha_fit_accumulate` (a NativeCLIP); `get_mean_prec` stays
    the route for any other `net`.

      * features: the same ops as `get_mean_prec` (`get_image_features`, then `f / f.norm()` in torch when
        args.normalize), so the rows are the same bits;
      * the covariance comes from gram = sum x x^T and sum = sum x of the SHIFTED rows x = f - shift, finalised on the
        host in fp64 as (gram - sum sum^T / n) / (n - 1) and inverted by the same LAPACK call.  The shift is the fp32
        column mean of the batch that starts at sample 0 (rank 0's first; broadcast before any rank accumulates).  It
        does not change the covariance, only the error: without it gram - sum sum^T / n cancels for features far from
        the origin;
      * the reference's class-"mean" rule (`get_mean_prec`'s docstring): sample g counts into n_cb[label, g // batch_size]
        and the feature rows g < n_batches are copied into a [n_batches, P] buffer as they stream past; the means are the
        same fp64 `n_cb @ rows / n_c` expression on the same values: bit-equal to the host route's;
      * world_size > 1: every rank takes `shard_range` of the training set, and gram, sum, n, the rows and the counts go
        through one all-reduce each (sums with zeros: exact).  A loader that cannot be sharded by index is refused.

    The batch size is the loader's `batch_size` (args.batch_size for a loader without one).  Returns (classwise_mean,
    precision) on every rank, with `return_cov=True` also the fp64 covariance; rank 0 writes the two .pt files."""
    import os

    import torch

    if not hasattr(net, "maha_fit_accumulate"):
        raise TypeError("get_mean_prec_device needs a net with maha_fit_state / maha_fit_accumulate (a NativeCLIP); "
                        "get_mean_prec is the host route")
    import itertools

    rank = mdist.world()[0]
    n_total = len(train_loader.dataset)
    bs = int(getattr(train_loader, "batch_size", None) or args.batch_size)
    n_batches = -(-n_total // bs)
    batches = _shard_batches(train_loader, n_total, _BY_INDEX.format("maha"))[0]
    g0 = _my_range(n_total)[0]

    def features(batch):
        f = net.get_image_features(pixel_values=batch[0]).float()
        if args.normalize:
            f = f / f.norm(dim=-1, keepdim=True)
        return f, batch[1]

    n_cb = np.zeros((args.n_cls, n_batches), np.float64)
    with torch.no_grad():
        first = []
        shift = torch.zeros(args.feat_dim, dtype=torch.float32)
        if rank == 0:  # the batch that starts at global sample 0
            first = [features(batch) for batch in itertools.islice(batches, 1)]
            if first:
                shift = first[0][0].mean(dim=0)
        mdist.broadcast_tensors([shift], src=0)
        state = net.maha_fit_state(shift)
        dev = state["gram"].device
        rows = torch.zeros((n_batches, state["gram"].shape[0]), dtype=torch.float32, device=dev)
        for f, labels in itertools.chain(first, map(features, batches)):
            b = f.shape[0]
            net.maha_fit_accumulate(f, state)
            if g0 < n_batches:  # the rows the reference's batch indices select
                rows[g0: min(g0 + b, n_batches)] = f[: n_batches - g0].to(dev)
            # labels >= n_cls are ignored, like the reference's per-class loop (:161-166) never visits them
            lab = labels.detach().cpu().numpy() if hasattr(labels, "detach") else np.asarray(labels)
            lab = lab.astype(np.int64).reshape(-1)[:b]
            keep = lab < args.n_cls
            np.add.at(n_cb, (lab[keep], (g0 + np.arange(b)[keep]) // bs), 1.0)
            g0 += b
        gram, fsum = state["gram"], state["sum"]
        n_t = torch.tensor([float(state["n"])], dtype=torch.float64, device=dev)
        ncb_t = torch.from_numpy(n_cb).to(dev)
        for t in (gram, fsum, n_t, rows, ncb_t):
            mdist.all_reduce_sum(t)
    n = float(n_t.cpu()[0])
    n_cb = ncb_t.cpu()
    classwise_mean = ((n_cb @ rows.cpu().double()) / n_cb.sum(dim=1, keepdim=True)).float()
    if args.normalize:
        classwise_mean = classwise_mean / classwise_mean.norm(dim=-1, keepdim=True)
    G, S = gram.cpu(), fsum.cpu()
    cov = (G - torch.outer(S, S) / n) / (n - 1.0)
    precision = torch.linalg.inv(cov).float()
    print(f"cond number: {torch.linalg.cond(precision)}")
    tdir = getattr(args, "template_dir", None)
    if tdir and rank == 0:
        os.makedirs(tdir, exist_ok=True)
        for what, t in (("classwise_mean", classwise_mean), ("precision", precision)):
            torch.save(t, os.path.join(tdir, maha_file_name(args, what)))
    if return_cov:
        return classwise_mean, precision, cov
    return classwise_mean, precision


def maha_file_name(args, what):
    """File names of the stored Mahalanobis statistics (reference :171-172, eval_ood_detection.py:77-78)."""
    return f"{args.model}_{what}_{args.in_dataset}_{args.max_count}_{args.normalize}.pt"


def get_Mahalanobis_score(args, net, test_loader, classwise_mean, precision, in_dist=True):
    """`--score maha`: per sample min_c 0.5 (f - mu_c) P (f - mu_c)^T — what reference
    utils/detection_util.py:176-207 returns (the negated max of -0.5 d_c) — with the per-class loop of
    torch.mm pairs replaced by the native kernels (one quadratic form + C dot products per image).
    Keeps the reference's loop rule that for OOD sets (`in_dist=False`) iteration stops at batch
    `len(dataset) // batch_size`, i.e. a trailing partial batch is NOT scored (:185-186)."""
    state = net.maha_prepare(classwise_mean, precision)
    total_len = len(test_loader.dataset)
    # the samples the reference scores: everything for the ID set, whole batches only for an OOD set
    n_scored = total_len if in_dist else min(total_len, (total_len // args.batch_size) * args.batch_size)

    def score(images):
        features = net.get_image_features(pixel_values=images).float()
        if args.normalize:
            features = features / features.norm(dim=-1, keepdim=True)
        return net.maha_scores(features, state)

    # image-sharded like get_ood_scores_clip: a contiguous index range per rank, all-gathered at the end
    return _score_loader(test_loader, n_scored, "maha", state["prec"].device, score)


def knn_auto_k(n_bank):
    """The k of `--score knn` for a bank of n_bank rows: Sun et al.'s k = 1000 at ImageNet-1k's 1 281 167 training images
    (k = 10 at their 1 % subset), scaled linearly and kept inside what `knn_scores` takes: min(1024, max(1, round(n / 1281)))."""
    return min(1024, max(1, int(round(int(n_bank) / 1281))))


def _unit_image_features(net, images):
    """`get_image_features` then `f / f.norm()` in torch: the k-NN score is defined on unit rows, whatever args.normalize says."""
    f = net.get_image_features(pixel_values=images).float()
    return f / f.norm(dim=-1, keepdim=True)


def get_knn_bank(args, net, train_loader):
    """`--score knn`: the bank of unit-norm training features, [n_train, P] fp32 on the net's device, in dataset order, on
    every rank.  Under world_size > 1 every rank encodes its `shard_range` of the training set (a loader that cannot be
    sharded by index is refused, as by `get_Mahalanobis_score`) and the shards are all-gathered: the bank is replicated like
    the prompt bank, images are sharded like everywhere else.  A feature does not depend on the batch it was computed in, so
    the bank holds the same bits at every world size."""
    import torch

    if not hasattr(net, "knn_scores"):
        raise TypeError("get_knn_bank needs a net with knn_scores (a NativeCLIP); there is no eager fallback")
    n_total = len(train_loader.dataset)
    with torch.no_grad():
        batches = _shard_batches(train_loader, n_total, _BY_INDEX.format("knn"))[0]
        parts = [_unit_image_features(net, images) for images, _labels in batches]
        return _gather_shards(parts, n_total, *_feature_home(args, net)).contiguous()


def get_knn_score(args, net, loader, bank, k):
    """`--score knn`: per sample sqrt(2 - 2 v_k), v_k the k-th largest dot product of its unit-norm feature with the rows
    of `bank` (`get_knn_bank`) — the distance to the k-th nearest training feature; larger = more OOD.  Sharded and gathered
    like `get_ood_scores_clip`; EVERY sample is scored (the drop-the-last-batch rule belongs to the reference's Mahalanobis
    function only).  Returns a float32 ndarray [len(loader.dataset)]."""
    k = int(k)
    if not 1 <= k <= len(bank):
        raise ValueError(f"--score knn: k = {k} needs 1 <= k <= the bank's {len(bank)} rows")
    return _score_loader(loader, len(loader.dataset), "knn", bank.device,
                         lambda images: net.knn_scores(_unit_image_features(net, images), bank, k))


NEG_MAX_GROUPS = DEFINES["MCM_NEG_MAX_GROUPS"]


def clean_negative_words(words, id_names):
    """Step 1 of the mining: the candidate words in file order, stripped; empty lines, later duplicates and words equal to an ID
    class name are dropped (all comparisons case-insensitive)."""
    seen = {str(c).strip().lower() for c in id_names}
    out = []
    for w in words:
        w = str(w).strip()
        if w and w.lower() not in seen:
            seen.add(w.lower())
            out.append(w)
    return out


def _candidate_features(args, net, cands):
    """[C, P] unit-norm fp32 text features of the candidate words through the ID labels' prompt template, on every rank: each
    rank encodes its `shard_range` of the candidates and the rows are all-gathered, as `get_knn_bank` does for images.  The
    whole list is tokenised on every rank, so a row's padded length does not depend on the world size."""
    import torch

    C = len(cands)
    lo, hi = _my_range(C)
    templates = getattr(args, "templates", None)
    with torch.no_grad():
        if hi <= lo:
            local = None
        elif templates:
            local = encode_prompt_ensemble(args, net, cands[lo:hi], templates)
        else:
            tok = _tokenizer(args, net)([PROMPT.format(c=c) for c in cands], padding=True, return_tensors="pt")
            local = _unit_text_features(net, {"input_ids": tok["input_ids"][lo:hi], "attention_mask": tok["attention_mask"][lo:hi]})
        return _gather_shards([] if local is None else [local.float().contiguous()], C, *_feature_home(args, net)).contiguous()


def _mine(args, net, id_names, words):
    """The mining of `mine_negative_labels`, with everything `get_neglabel_bank` needs next to it."""
    import torch

    if not hasattr(net, "knn_scores"):
        raise TypeError("mining negative labels needs a net with knn_scores (a NativeCLIP); there is no eager fallback")
    id_names = list(id_names)
    K = len(id_names)
    cands = clean_negative_words(words, id_names)
    C = len(cands)
    if K < 1 or C < 1:
        raise ValueError(f"--score neglabel: {K} ID names and {C} candidate words are left after cleaning; both must be at least 1")
    q = float(getattr(args, "neg_quantile", 0.95))
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"--neg-quantile {q}: must lie in [0, 1]")
    h = q * (K - 1)
    lo = int(np.floor(h))
    k = K - lo
    if k > 1024:
        raise ValueError(f"--score neglabel: the {q} quantile over {K} ID labels needs the {k} largest similarities of every "
                         "candidate, and knn_scores returns at most 1024: raise --neg-quantile")
    id_bank = prompt_bank(args, net, id_names)
    cand = _candidate_features(args, net, cands)
    with torch.no_grad():
        _, topv = net.knn_scores(cand, id_bank, k, return_values=True)
    topv = topv.detach().cpu().numpy().astype(np.float64)
    a_lo, a_hi = topv[:, K - 1 - lo], topv[:, max(K - 2 - lo, 0)]
    d = a_lo + (h - lo) * (a_hi - a_lo)
    count = int(getattr(args, "neg_count", 0) or 0)
    M = count if count > 0 else int(round(float(getattr(args, "neg_frac", 0.15)) * C))
    M = min(M, C)
    if M < 1:
        raise ValueError(f"--score neglabel: no candidate is kept (--neg-count / --neg-frac select {M} of {C})")
    order = np.lexsort((np.arange(C), d))[:M]          # d ascending, candidate index ascending among equals
    G = min(int(getattr(args, "neg_groups", 100)), M)
    if not 1 <= G <= NEG_MAX_GROUPS:
        raise ValueError(f"--neg-groups: {G} groups; 1 .. {NEG_MAX_GROUPS} are supported")
    gs = M // G
    order = order[:G * gs]
    return {"words": [cands[i] for i in order], "d": d[order], "index": order, "cand": cand, "id_bank": id_bank,
            "K": K, "C": C, "M": M, "G": G, "gs": gs}


def mine_negative_labels(args, net, id_names, words):
    """NegLabel's mining (Jiang et al., ICLR 2024): from the candidate `words` keep the ones farthest from the ID labels.
    d[c] = the `args.neg_quantile` (default 0.95) quantile, linearly interpolated, of candidate c's similarities to the K ID
    prompts, from the device's top-k values (`net.knn_scores(..., return_values=True)`) and finished in fp64; the
    M = `args.neg_count`, or round(`args.neg_frac` (0.15) x C), candidates with the smallest d are kept, ordered by (d, index),
    cut into G = min(`args.neg_groups` (100), M) consecutive groups of gs = M // G; the last M - G gs are dropped.
    Returns (the G gs selected words in that order, their d as a float64 ndarray)."""
    m = _mine(args, net, id_names, words)
    return m["words"], m["d"]


def get_neglabel_bank(args, net, id_names, words):
    """`--score neglabel`: the bank [K + G gs, P] of unit-norm fp32 text features — the K ID prompts, then the mined negatives
    group after group — with its geometry: {"bank", "K", "G", "gs", "words", "d", "C", "M"}.  Replicated on every rank, and
    the same bits at every world size (every rank mines the same gathered candidate features)."""
    import torch

    m = _mine(args, net, id_names, words)
    idx = torch.as_tensor(np.ascontiguousarray(m["index"]), dtype=torch.long, device=m["cand"].device)
    bank = torch.cat([m["id_bank"].float().to(m["cand"].device), m["cand"].index_select(0, idx)]).contiguous()
    return {"bank": bank, "K": m["K"], "G": m["G"], "gs": m["gs"], "words": m["words"], "d": m["d"], "C": m["C"], "M": m["M"]}


def get_neglabel_score(args, net, loader, bank_info):
    """`--score neglabel`: per sample -(1/G) sum_g S_g, S_g the softmax mass at temperature `args.neg_T` (0.01) of its unit-norm
    feature on the ID prompts against negative group g alone (`net.neglabel_scores`); larger = more OOD.  Sharded and gathered
    like `get_knn_score`; EVERY sample is scored.  Returns a float32 ndarray [len(loader.dataset)]."""
    if not hasattr(net, "neglabel_scores"):
        raise TypeError("get_neglabel_score needs a net with neglabel_scores (a NativeCLIP); there is no eager fallback")
    bank, K, G, gs = bank_info["bank"], int(bank_info["K"]), int(bank_info["G"]), int(bank_info["gs"])
    T = float(getattr(args, "neg_T", 0.01))
    return _score_loader(loader, len(loader.dataset), "neglabel", bank.device,
                         lambda images: net.neglabel_scores(_unit_image_features(net, images), bank, K, G, gs, T=T))


def vim_principal_dim(P, D=0):
    """The principal dimension of `--score vim` at feature width P: `D` when given, else the paper's rule — P // 2 below 768,
    512 for 768 <= P < 2048, 1000 above.  1 <= D < P is required (the null space keeps R = P - D >= 1 rows)."""
    P, D = int(P), int(D or 0)
    if D == 0:
        D = P // 2 if P < 768 else (512 if P < 2048 else 1000)
    if not 1 <= D < P:
        raise ValueError(f"--vim-dim D: D must be 0 or 1..proj_dim - 1 (D = {D}, proj_dim = {P})")
    return D


def vim_null_space(gram, n, D):
    """The null-space basis of ViM from gram = sum_i x_i x_i^T (fp64 [P,P]) of n rows, on the host in fp64: the eigenpairs of
    M = gram / n (`torch.linalg.eigh`, ascending), NS [R,P] = the eigenvectors of the R = P - D smallest eigenvalues as rows,
    rounded to fp32.  Returns (NS, eigenvalues [P] fp64 ascending: lambda_max = [-1], lambda_D = [R], lambda_{D+1} = [R - 1]).
    Refused where the subspace is not determined: lambda_D - lambda_{D+1} <= 64 eps_fp64 lambda_max (a training set of fewer
    than D rows is such a case: both are zero up to rounding)."""
    import torch

    M = torch.as_tensor(gram, dtype=torch.float64).detach().cpu()
    P = int(M.shape[0])
    n, D = int(n), int(D)
    if M.shape != (P, P) or n < 1 or not 1 <= D < P:
        raise ValueError(f"vim_null_space: gram {tuple(M.shape)}, n = {n}, D = {D}: a square gram, n >= 1 and 1 <= D < P are required")
    R = P - D
    lam, vec = torch.linalg.eigh(M / float(n))
    gap, lam_max = float(lam[R] - lam[R - 1]), float(lam[-1])
    if not gap > 64.0 * float(np.finfo(np.float64).eps) * lam_max:
        raise ValueError(f"--score vim: the principal subspace of dimension D = {D} is not determined by these {n} training rows: "
                         f"lambda_D = {float(lam[R]):.6e}, lambda_(D+1) = {float(lam[R - 1]):.6e}, lambda_max = {lam_max:.6e} "
                         "(a training set of fewer than D rows, or a flat spectrum): choose another --vim-dim")
    return vec[:, :R].T.contiguous().float(), lam


def get_vim_fit(args, net, train_loader, test_labels):
    """`--score vim` (Wang et al., CVPR 2022), the fit: {"bank", "K", "R", "D", "alpha", "T", "n", "eigenvalues"}.
      * every rank encodes its `shard_range` of the training set and keeps its shard of unit-norm features on the device (they
        are not gathered); their uncentred fp64 Gram matrix comes from the running sums of the Mahalanobis fit
        (`net.maha_fit_accumulate`, no shift: the zero-shot head has no bias, ViM's origin is 0) and goes through one all-reduce
        with n;
      * `vim_null_space` runs on every rank on the same bits: D = `vim_principal_dim(P, args.vim_dim)`, R = P - D;
      * bank [K + R, P] = the prompt bank, then the basis rows;
      * alpha = sum_i max_k logit[i, k] / sum_i resid[i] over ALL training rows (not the paper's sample of them), from one
        `net.vim_scores(..., alpha=0, return_parts=True)` pass over the shard, both sums in fp64 and all-reduced.  The score
        kernel takes it as fp32.
    A loader that cannot be sharded by index is refused under world_size > 1, as by `get_knn_bank`."""
    import logging

    import torch

    if not hasattr(net, "vim_scores") or not hasattr(net, "maha_fit_accumulate"):
        raise TypeError("get_vim_fit needs a net with vim_scores and maha_fit_accumulate (a NativeCLIP); there is no eager fallback")
    T = float(getattr(args, "vim_T", 0.01))
    n_total = len(train_loader.dataset)
    with torch.no_grad():
        state = net.maha_fit_state(None)
        shard = []
        for images, _labels in _shard_batches(train_loader, n_total, _BY_INDEX.format("vim"))[0]:
            f = _unit_image_features(net, images).contiguous()
            net.maha_fit_accumulate(f, state)
            shard.append(f)
        gram = state["gram"]
        dev = gram.device
        n_t = torch.tensor([float(state["n"])], dtype=torch.float64, device=dev)
        for t in (gram, n_t):
            mdist.all_reduce_sum(t)
        n = int(round(float(n_t.cpu()[0])))
        if n < 1:
            raise ValueError("--score vim: the training set is empty")
        P = int(gram.shape[0])
        D = vim_principal_dim(P, getattr(args, "vim_dim", 0))
        ns, lam = vim_null_space(gram, n, D)
        prompts = prompt_bank(args, net, test_labels).float()
        K, R = int(prompts.shape[0]), P - D
        bank = torch.cat([prompts.to(dev), ns.to(dev)]).contiguous()
        sums = torch.zeros(2, dtype=torch.float64, device=dev)  # sum maxlogit, sum resid
        for f in shard:
            _, parts = net.vim_scores(f, bank, K, T=T, alpha=0.0, return_parts=True)
            sums[0] += parts[:, 2].double().sum()
            sums[1] += parts[:, 0].double().sum()
        mdist.all_reduce_sum(sums)
    top, res = (float(v) for v in sums.cpu())
    alpha = top / res if res != 0.0 else float("nan")
    if res == 0.0 or not np.isfinite(alpha):
        raise ValueError(f"--score vim: alpha = sum max-logit / sum residual = {top} / {res} is not a finite number: the training "
                         "features have no component outside the principal subspace (or are not finite)")
    if alpha <= 0.0:
        logging.getLogger(__name__).warning(
            f"--score vim: alpha = {alpha:.6g} is not positive (sum max-logit = {top:.6g}): the residual enters the score with the "
            "wrong sign; seeded synthetic weights can produce this, a trained checkpoint should not")
    return {"bank": bank, "K": K, "R": R, "D": D, "alpha": alpha, "T": T, "n": n, "eigenvalues": lam.numpy()}


def get_vim_score(args, net, loader, fit):
    """`--score vim`: per sample alpha * resid - lse (`net.vim_scores` against `fit["bank"]` of `get_vim_fit`): the norm of its
    unit-norm feature's component in the null space of the training features' principal subspace, scaled to logit units, minus
    the energy of its logits at temperature fit["T"]; larger = more OOD.  Sharded and gathered like `get_knn_score`; EVERY
    sample is scored.  Returns a float32 ndarray [len(loader.dataset)]."""
    if not hasattr(net, "vim_scores"):
        raise TypeError("get_vim_score needs a net with vim_scores (a NativeCLIP); there is no eager fallback")
    bank, K = fit["bank"], int(fit["K"])
    T, alpha = float(fit["T"]), float(fit["alpha"])
    return _score_loader(loader, len(loader.dataset), "vim", bank.device,
                         lambda images: net.vim_scores(_unit_image_features(net, images), bank, K, T=T, alpha=alpha))


def _gather_batch_shards(local, n_total, ws):
    """All-gather score shards whose sizes only the owning rank knows (batch-range split of a generic
    loader: the last batch may be short, batch sizes need not be uniform).  Counts are exchanged first;
    the payload buffer is sized by the largest shard and sliced by the true counts."""
    import torch
    import torch.distributed as dist

    home = local.device
    if dist.get_backend() == "gloo" and local.is_cuda:  # ranks sharing a device (logic checks): host bounce
        local = local.cpu()
    cnt = torch.tensor([local.numel()], dtype=torch.int64, device=local.device)
    cnts = torch.empty(ws, dtype=torch.int64, device=local.device)
    dist.all_gather_into_tensor(cnts, cnt)
    cnts = [int(c) for c in cnts.cpu()]
    if sum(cnts) != n_total:
        raise RuntimeError(f"rank shards hold {sum(cnts)} scores, the dataset has {n_total}")
    cap = max(max(cnts), 1)
    buf = torch.zeros(cap, dtype=torch.float32, device=local.device)
    buf[: local.numel()] = local
    out = torch.empty(ws * cap, dtype=torch.float32, device=local.device)
    dist.all_gather_into_tensor(out, buf)
    return torch.cat([out[r * cap: r * cap + cnts[r]] for r in range(ws)]).to(home)


def print_measures(log, auroc, aupr, fpr, method_name="Ours", recall_level=0.95):
    """Same output format as reference utils/detection_util.py:37-45."""
    pct = int(100 * recall_level)
    if log is None:
        print("FPR{:d}:\t\t\t{:.2f}".format(pct, 100 * fpr))
        print("AUROC: \t\t\t{:.2f}".format(100 * auroc))
        print("AUPR:  \t\t\t{:.2f}".format(100 * aupr))
    else:
        log.debug("\t\t\t\t" + method_name)
        log.debug("  FPR{:d} AUROC AUPR".format(pct))
        log.debug("& {:.2f} & {:.2f} & {:.2f}".format(100 * fpr, 100 * auroc, 100 * aupr))


def get_and_print_results(args, log, in_score, out_score, auroc_list, aupr_list, fpr_list, net=None):
    """Reference utils/detection_util.py:253-265: the scores are negated confidences, so the
    metrics are taken on their negation with ID as the positive class.  Device tensors (from
    `get_ood_scores_clip(..., device_out=True)`) are evaluated by the native metric kernels
    of `net`; ndarrays go through the host implementation exactly like the reference."""
    if hasattr(in_score, "is_cuda"):
        if net is None or not hasattr(net, "measures"):
            raise TypeError("device score tensors need net= (a NativeCLIP) for the metric kernels")
        auroc, aupr, fpr = net.measures(in_score, out_score, negate=True)
        in_score, out_score = in_score[:3].cpu().numpy(), out_score[:3].cpu().numpy()
    else:
        auroc, aupr, fpr = get_measures(-in_score, -out_score)
    print(f"in score samples (random sampled): {in_score[:3]}, out score samples: {out_score[:3]}")
    auroc_list.append(auroc)
    aupr_list.append(aupr)
    fpr_list.append(fpr)
    print_measures(log, auroc, aupr, fpr, args.score)
