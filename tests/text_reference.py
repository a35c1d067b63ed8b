"""The text tower in numpy float64, for the tests that sweep the prompt length (test_text_reference.py proves it on the CPU,
test_gpu_text_lengths.py holds the HIP text tower to it).

text_tower_fp64 restates HF `CLIPTextModel` + `text_projection` from the HF-named state dict: token + position embedding,
pre-LN layers with a causal softmax, the geometry's activation, final_layer_norm, the row of the first position that holds the
largest id, the projection.  Every operation, the softmax included, runs in float64: HF's own `CLIPModel(...).double()` keeps
`softmax(..., dtype=torch.float32)` in its eager attention, so its "fp64" text features carry an fp32 softmax (about 1e-7)
and move when pads are added; this restatement does not.  Nothing here comes from the project's kernels or from oracle/.

length_prompts builds the prompts of the length sweep: the same prompt at every padded length S, one per EOS position."""
import math

import numpy as np

BOS, EOS = 49406, 49407

try:
    from scipy.special import erf as _erf
except ImportError:  # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])


def _ln(x, g, b, eps):
    mu = x.mean(axis=-1, keepdims=True)
    c = x - mu
    var = (c * c).mean(axis=-1, keepdims=True)
    return c / np.sqrt(var + eps) * g + b


def _act(x, kind):
    if kind == "quick_gelu":
        return x / (1.0 + np.exp(-1.702 * x))
    if kind == "gelu":
        return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))
    raise ValueError(kind)


class TextTowerFp64:
    """The text-tower weights of `sd` widened to float64 once (the token table stays as it is: rows are widened as they are
    looked up); call it with ids [K, S] -> (hidden [K, S, D] after final_layer_norm, pooled [K, P])."""

    def __init__(self, geo, sd):
        self.geo = geo
        self._tok = sd["text_model.embeddings.token_embedding.weight"]
        self._w = {k: np.asarray(v, np.float64) for k, v in sd.items()
                   if (k.startswith("text_model.") and "token_embedding" not in k and not k.endswith("position_ids"))
                   or k == "text_projection.weight"}

    def __call__(self, ids):
        geo, w = self.geo, self._w
        ids = np.asarray(ids)
        K, S = ids.shape
        H, D = geo.t_heads, geo.t_width
        hd = D // H
        x = np.asarray(self._tok[ids], np.float64) + w["text_model.embeddings.position_embedding.weight"][:S]
        future = np.triu(np.ones((S, S), bool), 1)
        for i in range(geo.t_layers):
            p = f"text_model.encoder.layers.{i}."

            def lin(a, name):
                return a @ w[p + name + ".weight"].T + w[p + name + ".bias"]

            h = _ln(x, w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], geo.ln_eps)
            q, k, v = (lin(h, "self_attn." + n).reshape(K, S, H, hd).transpose(0, 2, 1, 3) for n in ("q_proj", "k_proj", "v_proj"))
            s = (q * hd ** -0.5) @ k.transpose(0, 1, 3, 2)               # [K, H, S(query), S(key)]
            s = np.where(future, -np.inf, s)
            e = np.exp(s - s.max(axis=-1, keepdims=True))
            a = (e / e.sum(axis=-1, keepdims=True)) @ v
            x = x + lin(a.transpose(0, 2, 1, 3).reshape(K, S, D), "self_attn.out_proj")
            h = _ln(x, w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], geo.ln_eps)
            x = x + lin(_act(lin(h, "mlp.fc1"), geo.t_hidden_act), "mlp.fc2")
        hidden = _ln(x, w["text_model.final_layer_norm.weight"], w["text_model.final_layer_norm.bias"], geo.ln_eps)
        first_max = ids.argmax(axis=1)                                   # numpy's argmax: the FIRST position of the largest id
        pooled = hidden[np.arange(K), first_max] @ w["text_projection.weight"].T
        return hidden, pooled


def text_tower_fp64(geo, sd, ids):
    """(hidden [K, S, D], pooled [K, P]) of ids [K, S], float64 throughout (see the module's header)."""
    return TextTowerFp64(geo, sd)(ids)


def unit(a):
    a = np.asarray(a, np.float64)
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


# ---- the prompts of the length sweep -----------------------------------------------------------------------------------
def _body(seed, n):
    """[BOS, r_1, r_2, ...][:n], the r drawn from [1, BOS) by `seed` alone: a prefix of the same sequence at every n."""
    r = np.random.default_rng(seed).integers(1, BOS, size=80)
    return np.concatenate([[BOS], r])[:n]


def eos_positions(S):
    """EOS positions of the sweep at padded length S: {0, 1, S // 2, S - 2, S - 1} within [0, S - 1]."""
    return sorted({p for p in (0, 1, S // 2, S - 2, S - 1) if 0 <= p < S})


def garbage_position(S):
    """EOS position of the row that carries ids after its first EOS."""
    return S // 3


def prompt(p):
    """The prompt whose EOS sits at position p, at its own length p + 1: [BOS, r_1, ...][:p] + [EOS], r seeded by p alone."""
    return np.concatenate([_body(1000 + p, p), [EOS]]).astype(np.int64)


def garbage_prompt(p):
    """The prefix of the garbage row with its EOS at p (its own r sequence, so it is no copy of prompt(p))."""
    return np.concatenate([_body(5000 + p, p), [EOS]]).astype(np.int64)


def pad_to(row, S, garbage_seed=None):
    """row padded to S with EOS; garbage_seed: ids from [1, BOS) instead (all lower than the EOS before them)."""
    row = np.asarray(row, np.int64)
    n = S - row.shape[0]
    assert n >= 0
    tail = np.full(n, EOS, np.int64) if garbage_seed is None else \
        np.random.default_rng(garbage_seed).integers(1, BOS, size=n).astype(np.int64)
    return np.concatenate([row, tail])


def length_prompts(S):
    """(ids [K, S] int64, keys): one row per EOS position of eos_positions(S), padded with EOS, then the garbage row (EOS at
    S // 3, random lower ids after it).  keys[i] = ("eos", p) / ("garbage", p) names the prompt of row i: the same key is the
    same prompt at every S, and every row holds an EOS."""
    rows, keys = [], []
    for p in eos_positions(S):
        rows.append(pad_to(prompt(p), S))
        keys.append(("eos", p))
    g = garbage_position(S)
    rows.append(pad_to(garbage_prompt(g), S, garbage_seed=7000 + S))
    keys.append(("garbage", g))
    return np.stack(rows), keys


def reference_rows(tower, keys, cache):
    """fp64 pooled rows [len(keys), P] of the prompts named by keys, each computed ONCE at its own length (cache: a dict the
    caller keeps): pads and whatever follows the first EOS cannot reach the pooled row of a causal tower
    (test_text_reference.py::test_pad_invariance holds the restatement to that within 1e-12)."""
    out = []
    for key in keys:
        if key not in cache:
            kind, p = key
            cache[key] = tower((prompt(p) if kind == "eos" else garbage_prompt(p))[None, :])[1][0]
        out.append(cache[key])
    return np.stack(out)
