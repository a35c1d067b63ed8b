"""The envelope of geometries mcm_create accepts (include/mcm.h, the comment above mcm_create), as named points the suite runs
and as one predicate, and the cases just outside it.  Every point is inside the envelope and away from the shipped
checkpoints' shapes: widths that are 64 x an odd number (an odd number of 64-element K-steps in every 16-bit GEMM), widths with
whole 256-column LayerNorm slots plus a partial one (320, 1088), head counts 1, 3, 4 and 8 x 80, 5, 6, 15, 17, proj_dim down to
4 and off every power of two, patch sizes 4, 7, 8, 24 and 64, the 2-token tower (image_size == patch_size), one-layer towers and
text towers of 32, 248 and MAX_POSITIONS_LIMIT positions.  At most 2 layers and small images: the CPU oracle runs each in
seconds.  A plain module (no torch, no GPU): tests/test_geometry_envelope_cpu.py and tests/test_gpu_geometry_envelope.py share it."""
import dataclasses

from mcm_amd.config import TEST_GEOMETRIES, ClipGeometry

# The longest prompt the text tower's causal fp32 attention launches (attention.hip attn_f32_kernel keeps K [L][65], V [L][64],
# 4 query rows and 4 logit rows of a head in LDS: (133 L + 256) * 4 bytes against 160 KiB); mcm_create refuses more positions.
ATTN_F32_LDS_CAP = 160 * 1024


def attn_f32_lds_bytes(L):
    return (L * 65 + L * 64 + 4 * 64 + 4 * L) * 4


MAX_POSITIONS_LIMIT = max(L for L in range(1, 1024) if attn_f32_lds_bytes(L) <= ATTN_F32_LDS_CAP)
assert MAX_POSITIONS_LIMIT == 306

_TINY = TEST_GEOMETRIES["tiny"]


def _g(name, **kw):
    kw.setdefault("v_layers", 2)
    kw.setdefault("t_layers", 2)
    return ClipGeometry(name, **kw)


ENVELOPE = {g.name: g for g in [
    # ViT-S-like: 6 heads, an even number of K-steps, 384 = one whole LayerNorm slot and a half
    _g("w384", image_size=64, patch_size=16, v_width=384, v_heads=6, v_mlp=1536, t_width=384, t_heads=6, t_mlp=1536,
       proj_dim=384),
    # 3 and 5 heads, odd K-step counts everywhere (192 = 3 x 64, 448 = 7 x 64, 320 = 5 x 64, 704 = 11 x 64), P = 8
    _g("w192", image_size=32, patch_size=8, v_width=192, v_heads=3, v_mlp=448, t_width=320, t_heads=5, t_mlp=704,
       proj_dim=100),
    # 320 as 4 heads of 80, one layer per tower (the first layer is the last), 2 vision tokens, one text head, proj_dim 4
    _g("w320-h4x80-2tok", image_size=32, patch_size=32, v_width=320, v_heads=4, v_layers=1, v_mlp=1280, t_width=64,
       t_heads=1, t_layers=1, t_mlp=64, proj_dim=4),
    # 320 as 5 heads of 64, the MLP as narrow as the tower, P = 7 (generic patchify, padded K)
    _g("w320-h5x64", image_size=28, patch_size=7, v_width=320, v_heads=5, v_mlp=320, t_width=128, t_heads=2, t_mlp=512,
       proj_dim=260),
    # 17 and 15 heads: the wide LayerNorm with a partial fifth vector, QKV 3264 and 2880 wide, P = 4
    _g("w1088", image_size=16, patch_size=4, v_width=1088, v_heads=17, v_mlp=1088, t_width=960, t_heads=15, t_mlp=960,
       proj_dim=1020),
    # the text tower at other lengths than 77 (Long-CLIP has 248 positions); the vision tower is tiny's
    dataclasses.replace(_TINY, name="pos32", max_positions=32),
    dataclasses.replace(_TINY, name="pos248", max_positions=248),
    dataclasses.replace(_TINY, name=f"pos{MAX_POSITIONS_LIMIT}", max_positions=MAX_POSITIONS_LIMIT),
    dataclasses.replace(_TINY, name="tiny-1L", v_layers=1, t_layers=1),
    # P = 64: the largest patch the pixel-gathering GEMM takes; P = 24: patchify8 at a patch that is no power of two
    _g("p64", image_size=128, patch_size=64, v_width=128, v_heads=2, v_mlp=512, t_width=128, t_heads=2, t_mlp=512, proj_dim=64),
    _g("p24", image_size=48, patch_size=24, v_width=128, v_heads=2, v_mlp=512, t_width=128, t_heads=2, t_mlp=512, proj_dim=64),
]}
# the geometries whose vision tower differs from tiny's (the text-length ones score with tiny's vision tower)
TEXT_ONLY = ("pos32", "pos248", f"pos{MAX_POSITIONS_LIMIT}")


def accepted(geo, max_prompt_tokens=1024 * 77, max_batch=8):
    """mcm_create's acceptance rules (mcm_api.hip, after "unknown hidden_act"): None when the geometry is accepted, else the
    distinguishing words of the refusal's message."""
    g = geo
    if g.v_hidden_act not in ("quick_gelu", "gelu") or g.t_hidden_act not in ("quick_gelu", "gelu"):
        return "unknown hidden_act"
    if g.v_heads <= 0 or g.t_heads <= 0 or g.v_width not in (g.v_heads * 64, g.v_heads * 80) or g.t_width != g.t_heads * 64:
        return "head_dim must be 64 or 80"
    if g.patch_size <= 0 or g.image_size % g.patch_size:
        return "multiple of patch_size"
    if (g.v_width % 64 or g.t_width % 64 or g.v_mlp % 64 or g.t_mlp % 64 or g.v_width > 1280 or g.t_width > 1024
            or g.proj_dim % 4 or g.proj_dim > 1024):
        return "widths must be multiples of 64"
    if max_batch <= 0 or max_prompt_tokens <= 0 or g.max_positions <= 0 or max_prompt_tokens < g.max_positions:
        return "bad workspace bounds"
    if g.v_layers < 1 or g.t_layers < 1:
        return "must be at least 1"
    if g.max_positions > MAX_POSITIONS_LIMIT:
        return f"max_positions exceeds {MAX_POSITIONS_LIMIT}"
    if (g.image_size // g.patch_size) ** 2 + 1 > 1025:
        return "more than 1025 vision tokens"
    return None


def _out(base, **kw):
    return dataclasses.replace(ENVELOPE[base], name=base + "-" + "-".join(f"{k}={v}" for k, v in kw.items()), **kw)


def prompt_lengths(max_positions):
    """The sequence lengths S a text tower of max_positions positions is run at: 1, both sides of 77, the last two."""
    return sorted({s for s in (1, 77, 78, max_positions - 1, max_positions) if 1 <= s <= max_positions})


def prompts(K, S, seed, vocab_size=49408):
    """int32 [K, S] token ids as the tokenizer pads them: BOS, words, EOS (the largest id: the pooled position), EOS padding;
    prompt 0 fills the whole row, the others end anywhere from the second position on.  S == 1: the row is the EOS alone."""
    import numpy as np

    bos, eos = vocab_size - 2, vocab_size - 1
    rng = np.random.default_rng(seed)
    ids = np.full((K, S), eos, np.int32)
    for k in range(K):
        n = S if k == 0 else int(rng.integers(min(2, S), S + 1))      # tokens of prompt k, BOS and EOS included
        if S > 1:
            ids[k, 0] = bos
            ids[k, 1:n - 1] = rng.integers(1, bos - 1, size=max(n - 2, 0))
    return ids


# one step outside the envelope in each direction: (geometry, kwargs of accepted())
REFUSED = [
    (_out("w320-h5x64", v_heads=6), {}),                       # 320 / 6 is neither 64 nor 80
    (_out("w320-h4x80-2tok", t_width=80, t_heads=1), {}),      # 80-wide heads in the text tower
    (_out("w384", image_size=65), {}),
    (_out("w1088", v_width=1344, v_heads=21), {}),             # past 1280
    (_out("w1088", t_width=1088, t_heads=17), {}),             # past 1024
    (_out("w192", v_mlp=480), {}),                             # no multiple of 64
    (_out("w192", t_mlp=96), {}),
    (_out("w192", proj_dim=102), {}),
    (_out("w1088", proj_dim=1028), {}),
    (_out("pos248", max_positions=0), {}),
    (dataclasses.replace(ENVELOPE["pos248"], name="pos248-max_prompt_tokens=247"), {"max_prompt_tokens": 247}),
    (_out("tiny-1L", v_layers=0), {}),
    (_out("tiny-1L", t_layers=0), {}),
    (_out("pos248", max_positions=MAX_POSITIONS_LIMIT + 1), {}),
    (_out("w1088", image_size=132), {}),                       # 33 x 33 + 1 tokens
]
