"""Learned prompt contexts (CoOp, Zhou et al. 2022; LoCoOp, Miyai et al. 2023): from a checkpoint file to a prompt bank.

CoOp replaces the words of "a photo of a" by `n_ctx` free vectors in embedding space and trains them; its forward is: token-embed
the tokenised prompt "X X ... X classname.", overwrite the n_ctx placeholder positions with the learned vectors, add the position
embedding, run the unchanged text tower, pool at the largest id, project.  Learned vectors are not token ids, so they enter the
native path through `NativeCLIP.get_text_features_ctx` (include/mcm.h mcm_encode_text_ctx): ids for the ordinary positions, a slot
map for the context positions, and the context itself.

  load_context         a CoOp / LoCoOp checkpoint, a bare state dict or a .npy  ->  the context as float32
  context_prompts      (tokenizer, labels, n_ctx, position)  ->  ids [K,S], slots [K,S] in CoOp's three layouts
  encode_context_bank  (args, net, labels)  ->  the [K,P] unit-norm bank `detection.prompt_bank` hands to every score
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .tokenizer import BOS, EOS

POSITIONS = ("end", "middle", "front")   # CoOp's TRAINER.COOP.CLASS_TOKEN_POSITION
PLACEHOLDER = 0                          # the id under a context slot: never looked up, below EOS so pooling passes over it
MAX_LEN = 77


class Context(NamedTuple):
    ctx: np.ndarray      # float32 [n_ctx, width] (shared) or [K, n_ctx, width] (per class, CoOp's CSC)
    n_ctx: int
    per_class: bool


def load_context(path) -> Context:
    """The learned context of `path` as float32 (a 16-bit checkpoint is widened exactly), with n_ctx and whether it is per class.
    `path` is a CoOp / LoCoOp checkpoint (`prompt_learner/model.pth.tar-50`: a torch.save'd dict whose "state_dict" holds `ctx`
    next to `token_prefix` / `token_suffix`, which are ignored: they are embeddings of the training run's class names), a bare
    state dict with `ctx`, or a .npy holding the array itself.  Loaded with weights_only=True: nothing in the file is executed."""
    path = str(path)
    if path.endswith(".npy"):
        arr = np.load(path, allow_pickle=False)
    else:
        import torch

        try:
            obj = torch.load(path, map_location="cpu", weights_only=True)
        except Exception as e:
            raise ValueError(f"{path}: torch.load(weights_only=True) cannot read it ({type(e).__name__}: {str(e).splitlines()[0] if str(e) else ''}); "
                             "re-save the ctx tensor alone as a .npy (np.save(file, ctx.float().cpu().numpy())) and pass that") from e
        if isinstance(obj, dict) and isinstance(obj.get("state_dict"), dict):
            obj = obj["state_dict"]
        if not isinstance(obj, dict) or "ctx" not in obj:
            raise ValueError(f"{path}: no `ctx` entry (expected a CoOp checkpoint with state_dict['ctx'], or a state dict with 'ctx')")
        t = obj["ctx"]
        arr = t.detach().to(torch.float32).numpy() if hasattr(t, "detach") else np.asarray(t)
    if not np.issubdtype(arr.dtype, np.floating):
        raise ValueError(f"{path}: ctx must hold floats, got {arr.dtype}")
    if arr.ndim not in (2, 3) or 0 in arr.shape:
        raise ValueError(f"{path}: ctx must be [n_ctx, width] or [classes, n_ctx, width], got shape {tuple(arr.shape)}")
    arr = np.ascontiguousarray(arr, dtype=np.float32)
    if not np.isfinite(arr).all():
        raise ValueError(f"{path}: ctx holds a non-finite value")
    return Context(arr, int(arr.shape[-2]), arr.ndim == 3)


def _name_tokens(tokenizer, labels):
    """Per label the tokens of `label.replace("_", " ") + "."` through the tokenizer's call contract — the row without BOS, up
    to the first EOS; the last token is the "." (CoOp's `suffix[:name_len]` then `"."`) — and the id the tokenizer pads with."""
    out = tokenizer([str(c).replace("_", " ") + "." for c in labels], padding=True, return_tensors="np")
    ids = np.asarray(out["input_ids"])
    names, pad = [], EOS
    for row in ids:
        end = int(np.argmax(row == EOS)) if (row == EOS).any() else len(row)
        names.append([int(t) for t in row[1:end]])
        if end + 1 < len(row):
            pad = int(row[end + 1])
    return names, pad


def context_prompts(tokenizer, labels, n_ctx: int, position: str = "end"):
    """(ids [K,S] int32, slots [K,S] int32) of CoOp's prompts for `labels`; with half = n_ctx // 2:
        end     BOS, ctx x n_ctx, name, ".", EOS
        middle  BOS, ctx x half, name, ctx x (n_ctx - half), ".", EOS
        front   BOS, name, ctx x n_ctx, ".", EOS
    slots is -1 at an ordinary token and j at the position of context row j (in order, 0 ... n_ctx - 1); ids holds PLACEHOLDER
    there.  Rows are padded behind EOS, as the tokenizer pads, to the longest prompt.  A prompt longer than 77 raises."""
    if position not in POSITIONS:
        raise ValueError(f"position must be one of {POSITIONS}, got {position!r}")
    n_ctx = int(n_ctx)
    if n_ctx < 1:
        raise ValueError("n_ctx must be at least 1")
    names, pad = _name_tokens(tokenizer, labels)
    half = n_ctx // 2
    rows = []
    for label, name in zip(labels, names):
        if not name:
            raise ValueError(f"label {label!r} tokenises to nothing")
        body, dot = [(t, -1) for t in name[:-1]], [(name[-1], -1)]
        ctx = [(PLACEHOLDER, j) for j in range(n_ctx)]
        if position == "end":
            mid = ctx + body
        elif position == "middle":
            mid = ctx[:half] + body + ctx[half:]
        else:
            mid = body + ctx
        row = [(BOS, -1)] + mid + dot + [(EOS, -1)]
        if len(row) > MAX_LEN:
            raise ValueError(f"the prompt of label {label!r} has {len(row)} tokens with n_ctx = {n_ctx}; the text tower takes {MAX_LEN}")
        rows.append(row)
    S = max(len(r) for r in rows)
    ids = np.full((len(rows), S), pad, dtype=np.int32)
    slots = np.full((len(rows), S), -1, dtype=np.int32)
    for k, r in enumerate(rows):
        ids[k, :len(r)] = [t for t, _ in r]
        slots[k, :len(r)] = [j for _, j in r]
    return ids, slots


def encode_context_bank(args, net, labels):
    """The [K,P] unit-norm prompt bank of `labels` under the learned context `args.ctx` (a file `load_context` reads), laid out by
    `args.ctx_position` (default "end").  A per-class context must hold exactly len(labels) classes."""
    from .detection import _tokenizer

    labels = list(labels)
    c = load_context(args.ctx)
    if c.per_class and c.ctx.shape[0] != len(labels):
        raise ValueError(f"{args.ctx}: a per-class context of {c.ctx.shape[0]} classes, but {len(labels)} labels to score against")
    ids, slots = context_prompts(_tokenizer(args, net), labels, c.n_ctx, getattr(args, "ctx_position", None) or "end")
    return net.get_text_features_ctx(ids, slots, c.ctx, normalize=True)
