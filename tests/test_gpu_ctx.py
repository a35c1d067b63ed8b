"""Learned prompt contexts on the GPU: text_embed_ctx_kernel, mcm_encode_text_ctx, NativeCLIP.get_text_features_ctx and --ctx.

The idea the tests rest on: overwriting rows of a COPY of the token table with the context rows, and giving those row numbers
as ordinary ids, is the same computation through the unchanged path.  The fp32 add `row + pos` is the same add either way, so
the context entry on a handle built from the seeded state dict and get_text_features on a handle built from the edited state
dict must agree bit for bit; and tests/text_reference.TextTowerFp64 on the edited state dict (proved on the CPU by
test_text_reference.py) is the float64 reference.  One edited table per geometry holds every context of every case, each in
rows of its own (40000 ...: below EOS, and no id that the class names use), so one edited handle serves all cases.

  1. the kernel alone (mcm_debug_op_text_embed_ctx) against numpy float32, bit for bit, rim untouched;
  2. the whole entry against the edited-table handle, bit for bit, in three passes (the last ragged) and in one;
  3. the entry against float64 at the tower tolerances of test_gpu_text_lengths.py ("BUDGET text-ctx ..." lines, run with -s);
  4. get_text_features keeps its bits around a context call;
  5. every refusal: its code, nothing launched, a message;
  6. the CLI with --ctx on a file holding the token rows of "a photo of a" equals the plain token path, bit for bit."""
import ctypes
import itertools
import types
import warnings

import numpy as np
import pytest

from tests import gpu_scaffold as gs
from tests import text_reference as tr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL, ERANGE = -1, -7
TOK = "text_model.embeddings.token_embedding.weight"
LABELS = ["tench", "toilet_paper", "great_white_shark", "ox", "a_very_long_winded_class_name"]
K = len(LABELS)
N_CTX, POSITIONS, KINDS = (1, 4, 16), ("end", "middle", "front"), ("gauss", "photo")
BASE = 40000                       # first table row that holds a context row in the edited table
FP32_ATOL, COS_FLOOR = 2e-4, {"fp16": 0.99998, "bf16": 0.999}   # test_gpu_text_lengths.py's tower tolerances
CASES = list(itertools.product(KINDS, (False, True), N_CTX, POSITIONS))   # (kind, per_class, n_ctx, position)


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # the hash tokenizer says that its ids are stand-ins
        yield


_ptr = gs.ptr


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


# ---- contexts, prompts and the edited table ------------------------------------------------------------------------------
_WORLD = {}     # geometry name -> dict(geo, sd, sd_edit, ctx, row0, end, tower, ref)


def _world(name):
    """Per geometry, built once and left unchanged: the seeded state dict, the contexts of every (kind, per_class) at n_ctx = 16
    (n_ctx = 1, 4 use their first rows), and the edited state dict whose token table holds them from row BASE on."""
    from mcm_amd.config import geometry
    from mcm_amd.tokenizer import HashTokenizer
    from mcm_amd.weights import synth_state_dict

    if name in _WORLD:
        return _WORLD[name]
    geo = geometry(name)
    sd = synth_state_dict(geo, 0)
    D, nmax = geo.t_width, max(N_CTX)
    rng = np.random.default_rng(11)
    words = np.asarray(HashTokenizer()(["a photo of a"], return_tensors="np")["input_ids"])[0, 1:5]
    ctx, row0 = {}, {}
    table = sd[TOK].copy()          # (the seeded arrays are read-only and shared)
    nxt = BASE
    for kind, per_class in itertools.product(KINDS, (False, True)):
        sets = K if per_class else 1
        if kind == "gauss":         # as CoOp initialises a context: N(0, 0.02^2)
            c = (0.02 * rng.standard_normal((sets, nmax, D))).astype(np.float32)
        else:                       # the token rows of "a photo of a", repeated to n_ctx rows; class k starts at word k
            c = np.stack([sd[TOK][words[(np.arange(nmax) + k) % 4]] for k in range(sets)]).astype(np.float32)
        ctx[kind, per_class], row0[kind, per_class] = c, nxt
        table[nxt:nxt + sets * nmax] = c.reshape(-1, D)
        nxt += sets * nmax
    assert nxt < tr.EOS
    sd_edit = dict(sd)
    sd_edit[TOK] = table
    _WORLD[name] = w = dict(geo=geo, sd=sd, sd_edit=sd_edit, ctx=ctx, row0=row0, end=nxt, tower=None, ref={})
    return w


def _case(w, case, S=None):
    """(ids, slots, ctx, ids_edit) of a case: the context call's arguments and the ordinary ids that mean the same on the edited
    table — under slot j of prompt k the number of the table row that holds ctx[set(k), j].  S: pad (with EOS) to that length."""
    from mcm_amd.prompts import context_prompts
    from mcm_amd.tokenizer import HashTokenizer

    kind, per_class, n_ctx, position = case
    ids, slots = context_prompts(HashTokenizer(), LABELS, n_ctx, position)
    if S is not None:
        pad = S - ids.shape[1]
        ids = np.pad(ids, ((0, 0), (0, pad)), constant_values=tr.EOS)
        slots = np.pad(slots, ((0, 0), (0, pad)), constant_values=-1)
    assert not ((ids >= BASE) & (ids < w["end"])).any() and (ids.max(axis=1) == tr.EOS).all()   # no class token on a context's row
    c = w["ctx"][kind, per_class][:, :n_ctx]
    set_of = np.arange(K)[:, None] if per_class else np.zeros((K, 1), np.int64)
    rows = w["row0"][kind, per_class] + set_of * max(N_CTX) + slots
    ids_edit = np.where(slots >= 0, rows, ids).astype(np.int32)
    return ids, slots, (c if per_class else c[0]), ids_edit


def _net(w, edited, arm="fp32", mpt=1024 * 77, harness=False):
    from mcm_amd.engine import NativeCLIP

    return NativeCLIP(w["geo"], w["sd_edit"] if edited else w["sd"], precision=arm, max_batch=4, max_prompt_tokens=mpt,
                      harness=harness)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_harness():
    net = _net(_world("tiny"), False, "fp16", 256, harness=True)
    yield net
    net.close()


def _slot_pattern(S, n_ctx, rng):
    """[5, S]: row 0 a slot at position 0 and at the last one, row 1 no slot, row 2 all slots, row 3 a random mix, row 4 the last
    position only."""
    slot = np.full((5, S), -1, np.int32)
    slot[0, 0], slot[0, S - 1] = 0, n_ctx - 1
    slot[2] = np.arange(S) % n_ctx
    mix = rng.random(S) < 0.5
    slot[3, mix] = rng.integers(0, n_ctx, size=int(mix.sum()))
    slot[4, S - 1] = 0
    return slot


@pytest.mark.parametrize("per_set", [False, True], ids=["shared", "per-prompt"])
@pytest.mark.parametrize("D", [4, 100, 1024, 1028])
def test_kernel_is_a_gather_and_one_fp32_add_bit_for_bit(tiny_harness, D, per_set):
    """D = 4 the smallest width, 100 a ragged one, 1024 the last with one turn of the per-thread column loop, 1028 the first with
    a second.  x lies inside a larger buffer of NaN: the rows in front of it and behind it stay NaN."""
    net = tiny_harness
    Kk, S, V, n_ctx, rim = 5, 9, 50, 4, 3
    rng = np.random.default_rng(D + per_set)
    tok = (0.5 * rng.standard_normal((V, D))).astype(np.float32)
    pos = (0.1 * rng.standard_normal((S, D))).astype(np.float32)
    n_sets = Kk if per_set else 1
    ctx = (0.02 * rng.standard_normal((n_sets, n_ctx, D))).astype(np.float32)
    ids = rng.integers(0, V, size=(Kk, S)).astype(np.int32)
    ids.flat[0], ids.flat[-1] = V - 1, V - 1     # the largest id under a slot (row 0, row 4): a placeholder is never looked up
    slot = _slot_pattern(S, n_ctx, rng)
    buf = torch.full(((Kk * S + 2 * rim) * D,), float("nan"), device="cuda")
    x = buf[rim * D:(rim + Kk * S) * D]
    assert x.data_ptr() % 16 == 0
    tok_d, pos_d, ctx_d = (torch.from_numpy(a).cuda() for a in (tok, pos, ctx))
    rc = net._lib.mcm_debug_op_text_embed_ctx(net._h, _vp(ids), _vp(slot), V, _ptr(tok_d), _ptr(pos_d), _ptr(ctx_d), n_ctx, n_sets,
                                              _ptr(x), Kk, S, D, None)
    assert rc == 0, net._lib.mcm_last_error(net._h)
    torch.cuda.synchronize()
    sets = np.arange(Kk)[:, None] if per_set else np.zeros((Kk, 1), np.int64)
    src = np.where((slot < 0)[..., None], tok[ids], ctx[sets, np.maximum(slot, 0)])
    want = (src + pos[None, :S]).astype(np.float32).reshape(Kk * S, D)
    got = buf.cpu().numpy()
    assert np.array_equal(got[rim * D:(rim + Kk * S) * D].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert np.isnan(got[:rim * D]).all() and np.isnan(got[(rim + Kk * S) * D:]).all()
    assert net.kernel_faults == 0


def test_kernel_entry_refusals(tiny_harness):
    net = tiny_harness
    t = torch.full((256,), float("nan"), device="cuda")
    ids, slot = np.zeros(4, np.int32), np.full(4, -1, np.int32)

    def call(ids=ids, slot=slot, V=4, ctx=_ptr(t), n_ctx=1, n_sets=1, Kk=1, S=4, D=4):
        return net._lib.mcm_debug_op_text_embed_ctx(net._h, _vp(ids), _vp(slot), V, _ptr(t), _ptr(t), ctx, n_ctx, n_sets,
                                                    _ptr(t), Kk, S, D, None)

    assert call(D=6, S=1) == EINVAL                                          # D % 4
    assert call(slot=np.array([-1, 1, -1, -1], np.int32)) == EINVAL          # a slot past n_ctx
    assert call(slot=np.array([-2, -1, -1, -1], np.int32)) == EINVAL
    assert call(ids=np.array([0, 4, 0, 0], np.int32)) == EINVAL              # an id outside the table
    assert call(n_sets=2) == EINVAL                                          # neither 1 nor K
    assert call(ctx=ctypes.c_void_p(t.data_ptr() + 4)) == EINVAL             # not 16-byte aligned
    assert call(ctx=None) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(t).all()                                              # nothing was launched


# ---- 2. the whole entry against the edited-table handle, bit for bit -------------------------------------------------------
def _equal_on_pair(name, mpt, S):
    w = _world(name)
    a, b = _net(w, False, "fp32", mpt), _net(w, True, "fp32", mpt)
    differ = []
    try:
        for case in CASES:
            ids, slots, ctx, ids_edit = _case(w, case, S)
            for normalize in (True, False):
                got = a.get_text_features_ctx(ids, slots, ctx, normalize=normalize)
                want = b.get_text_features(input_ids=torch.from_numpy(ids_edit), normalize=normalize)
                assert torch.isfinite(got).all(), (case, normalize)
                if not torch.equal(_bits(got), _bits(want)):
                    differ.append(f"{case} normalize={normalize}: max |difference| {float((got - want).abs().max()):.3g}")
        assert a.kernel_faults == 0 and b.kernel_faults == 0
    finally:
        a.close()
        b.close()
    assert not differ, "\n".join(differ)


@pytest.mark.parametrize("name", ["tiny", "H14-2L"])
def test_entry_equals_the_edited_table_in_three_passes(name):
    """max_prompt_tokens = 154 at S = 77 with K = 5: passes of 2, 2 and 1 prompts, so a per-class set index crosses passes."""
    _equal_on_pair(name, 154, 77)


@pytest.mark.parametrize("name", ["tiny", "H14-2L"])
def test_entry_equals_the_edited_table_in_one_pass(name):
    _equal_on_pair(name, 1024 * 77, None)


# ---- 3. against float64 ----------------------------------------------------------------------------------------------------
def _reference(w, case):
    """fp64 pooled rows [K, P] of a case: TextTowerFp64 on the edited state dict at the prompts' own length, computed once."""
    if w["tower"] is None:
        w["tower"] = tr.TextTowerFp64(w["geo"], w["sd_edit"])
    if case not in w["ref"]:
        w["ref"][case] = w["tower"](_case(w, case)[3])[1]
    return w["ref"][case]


def _cos(a, b):
    return np.sum(tr.unit(a) * tr.unit(b), axis=-1)


@pytest.mark.parametrize("arm", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "B16-2L"])
def test_entry_against_fp64(name, arm):
    """The criteria of test_gpu_text_lengths.py::_length_sweep: max abs 2e-4 on unit rows (both forms) and on the raw rows relative
    to max(1, max |raw|), asked of every arm (the text tower is fp32 in all of them), and the 16-bit arms' cosine floors.  The
    handle runs every case at S = 77 in three passes; the reference rows are those of the unpadded prompts."""
    w = _world(name)
    net = _net(w, False, arm, 154)
    missed, worst = [], (np.zeros(2), None)
    try:
        for case in CASES:
            want = _reference(w, case)
            ids, slots, ctx, _ = _case(w, case, 77)
            txt = net.get_text_features_ctx(ids, slots, ctx, normalize=True).cpu().numpy().astype(np.float64)
            raw = net.get_text_features_ctx(ids, slots, ctx).cpu().numpy().astype(np.float64)
            assert np.isfinite(txt).all() and np.isfinite(raw).all(), case
            err = np.maximum(np.abs(txt - tr.unit(want)).max(axis=1), np.abs(tr.unit(raw) - tr.unit(want)).max(axis=1))
            err = np.maximum(err, np.abs(raw - want).max(axis=1) / max(1.0, float(np.abs(want).max())))
            one_minus_cos = 1.0 - np.minimum(_cos(txt, want), _cos(raw, want))
            bad = err > FP32_ATOL
            if arm != "fp32":
                bad |= ~(1.0 - one_minus_cos > COS_FLOOR[arm])
            if err.max() >= worst[0][0]:
                worst = (np.array([err.max(), one_minus_cos.max()]), case)
            for i in np.nonzero(bad)[0]:
                missed.append(f"{case} row {i}: max abs {err[i]:.3g}, 1 - cos {one_minus_cos[i]:.3g}")
        sat, faults = net.saturation_count(), net.kernel_faults
    finally:
        net.close()
    print(f"BUDGET text-ctx {name} {arm} worst max-abs {worst[0][0]:.3g} 1-cos {worst[0][1]:.3g} at {worst[1]}")
    assert sat == 0 and faults == 0, (sat, faults)
    assert not missed, "\n".join(missed)


# ---- 4. get_text_features keeps its bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mpt,S", [(154, 77), (1024 * 77, 9)])
def test_a_context_call_leaves_nothing_behind_in_the_id_staging(mpt, S):
    """The context call stages negative words in the buffers get_text_features uploads its ids through: the calls before and after
    it return the same bits."""
    w = _world("tiny")
    net = _net(w, False, "fp32", mpt)
    try:
        ids = torch.from_numpy(tr.length_prompts(S)[0])
        before = [net.get_text_features(input_ids=ids, normalize=n) for n in (True, False)]
        for case in (("gauss", True, 16, "end"), ("photo", False, 4, "middle")):
            cids, slots, ctx, _ = _case(w, case, 77 if S == 77 else None)
            net.get_text_features_ctx(cids, slots, ctx, normalize=True)
            after = [net.get_text_features(input_ids=ids, normalize=n) for n in (True, False)]
            assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(before, after)), case
        assert net.kernel_faults == 0
    finally:
        net.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def test_entry_refusals_launch_nothing_and_say_why():
    w = _world("tiny")
    net = _net(w, False, "fp32", 154)
    D, P = w["geo"].t_width, w["geo"].proj_dim
    try:
        ids, slots, ctx, _ = _case(w, ("gauss", False, 4, "end"))
        S = ids.shape[1]
        ctx_d = torch.from_numpy(np.ascontiguousarray(np.concatenate([ctx.reshape(-1), np.zeros(4, np.float32)]))).cuda()
        out = torch.full((K, P), float("nan"), device="cuda")
        err = lambda: net._lib.mcm_last_error(net._h).decode()   # noqa: E731

        def call(ids=ids, slots=slots, Kk=K, S=S, ctx=_ptr(ctx_d), n_ctx=4, n_sets=1, out_p=_ptr(out)):
            return net._lib.mcm_encode_text_ctx(net._h, _vp(ids), _vp(slots), Kk, S, ctx, n_ctx, n_sets, 1, out_p, None)

        def changed(a, where, value):
            b = a.copy()
            b[where] = value
            return b

        long_ids = np.pad(ids, ((0, 0), (0, 78 - S)), constant_values=tr.EOS)
        long_slots = np.pad(slots, ((0, 0), (0, 78 - S)), constant_values=-1)
        refused = [
            (dict(ids=None), EINVAL, "null"), (dict(slots=None), EINVAL, "null"), (dict(ctx=None), EINVAL, "null"),
            (dict(out_p=None), EINVAL, "null"),
            (dict(Kk=0), EINVAL, "positive"), (dict(S=0), EINVAL, "positive"), (dict(n_ctx=0), EINVAL, "positive"),
            (dict(n_sets=2), EINVAL, "n_sets"), (dict(n_sets=0), EINVAL, "n_sets"), (dict(n_sets=K + 1), EINVAL, "n_sets"),
            (dict(slots=changed(slots, (1, 2), 4)), EINVAL, "slot"), (dict(slots=changed(slots, (K - 1, S - 1), -2)), EINVAL, "slot"),
            (dict(ids=changed(ids, (2, 0), w["geo"].vocab_size)), EINVAL, "token id"), (dict(ids=changed(ids, (0, 1), -1)), EINVAL, "token id"),
            (dict(ctx=ctypes.c_void_p(ctx_d.data_ptr() + 4)), EINVAL, "aligned"),
            (dict(ids=long_ids, slots=long_slots, S=78), ERANGE, "max_position"),
        ]
        for kw, code, word in refused:
            assert call(**kw) == code, (kw.keys(), err())
            assert word in err(), (kw.keys(), err())
        torch.cuda.synchronize()
        assert torch.isnan(out).all()                            # nothing was launched
        assert call() == 0 and torch.isfinite(out).all()         # and the same arguments unchanged are taken
        # the Python front end
        good = np.zeros((4, D), np.float32)
        for bad in (np.zeros((4, D + 4), np.float32), np.zeros(D, np.float32), np.zeros((1, K, 4, D), np.float32),
                    np.zeros((K + 1, 4, D), np.float32), np.zeros((0, D), np.float32), np.zeros((4, D), np.int32)):
            with pytest.raises(ValueError):
                net.get_text_features_ctx(ids, slots, bad)
        with pytest.raises(ValueError):
            net.get_text_features_ctx(ids, slots[:, :-1], good)
        with pytest.raises(ValueError):
            net.get_text_features_ctx(long_ids, long_slots, good)
        for dt in (torch.float16, torch.bfloat16, torch.float64):    # any float dtype; a 16-bit one is widened exactly
            c16 = torch.from_numpy(ctx).to(dt)
            assert torch.equal(net.get_text_features_ctx(ids, slots, c16), net.get_text_features_ctx(ids, slots, c16.float().numpy()))
        assert net.kernel_faults == 0
    finally:
        net.close()


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------
CKPT, N, T_CTX = "ViT-B/32", 48, 0.02


@pytest.fixture(scope="module")
def plain_model():
    """A model built as the CLI builds it (seeded fp16-exact weights, fp16 arm, no split-activation workspace), its bank from the
    PLAIN token path on "a photo of a {name}." ids, and the ID / OOD pixels of the CLI's seeded synthetic sets."""
    import eval_ood_detection as cli
    from mcm_amd import detection
    from mcm_amd.config import HUB_IDS
    from mcm_amd.engine import build_model
    from mcm_amd.synth import DevicePatternLoader
    from utils.common import get_test_labels

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        net = build_model(CKPT, device=0, precision="fp16", max_batch=N, synthetic_regime="fp16-exact", x2_max_batch=-1)
        args = types.SimpleNamespace(in_dataset="ImageNet10", ckpt=HUB_IDS[CKPT], weights=None)
        labels = get_test_labels(args)
        tok = detection._tokenizer(args, net)
        ids = tok([f"a photo of a {c.replace('_', ' ')}." for c in labels], padding=True, return_tensors="pt")["input_ids"]
        words = np.asarray(tok(["a photo of a"], return_tensors="np")["input_ids"])[0, 1:5]
    bank = net.get_text_features(input_ids=ids, normalize=True)
    dev = torch.device("cuda", 0)
    px = {what: next(iter(DevicePatternLoader(N, net.geo.image_size, 10, N, dev, ood=ood, seed=cli.SEEDS[what])))[0]
          for what, ood in (("id", False), ("ImageNet20", True))}
    yield types.SimpleNamespace(net=net, bank=bank, px=px, words=words)
    net.close()


def _coop_file(path, plain_model):
    """A CoOp-style checkpoint: state_dict['ctx'] in fp16 (the seeded fp16-exact rows are fp16 numbers) next to the buffers a CoOp
    run also saves, which the loader ignores."""
    from mcm_amd.config import geometry
    from mcm_amd.weights import synth_state_dict

    rows = synth_state_dict(geometry(CKPT), 0, "fp16-exact")[TOK][plain_model.words]
    ctx = torch.from_numpy(rows.astype(np.float16))
    assert np.array_equal(ctx.float().numpy(), rows)
    torch.save({"state_dict": {"ctx": ctx, "token_prefix": torch.zeros(10, 1, 8, dtype=torch.float16),
                               "token_suffix": torch.zeros(10, 72, 8, dtype=torch.float16)}, "epoch": 50}, path)
    return str(path)


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


@pytest.mark.parametrize("score", ["MCM", "GL-MCM"])
def test_cli_with_the_rows_of_a_photo_of_a_equals_the_plain_token_path(tmp_path, monkeypatch, plain_model, score):
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    f = _coop_file(tmp_path / "model.pth.tar-50", plain_model)
    r = cli.main(["--in_dataset", "ImageNet10", "--CLIP_ckpt", CKPT, "--synthetic", "--synthetic-n", str(N), "-b", str(N),
                  "--score", score, "--ctx", f, "--ctx-T", str(T_CTX), "--T", "7", "--refine-threshold", "off", "--name", "ctx"])
    m = plain_model
    for what, got in (("id", r["in_score"]), ("ImageNet20", r["out_scores"]["ImageNet20"])):
        if score == "MCM":
            want = m.net.score_images(m.px[what], m.bank, T_CTX, "MCM")
        else:
            want = m.net.score_images_glmcm(m.px[what], m.bank, T_CTX, 1.0)
        got, want = _np(got).astype(np.float32), _np(want).astype(np.float32)
        assert got.shape == (N,) and np.isfinite(got).all()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, np.abs(got - want).max())
    log = open(tmp_path / r["log_directory"] / "ood_eval_info.log").read()
    assert "n_ctx = 4" in log and "shared" in log and "end" in log and "model.pth.tar-50" in log
