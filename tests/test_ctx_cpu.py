"""Learned prompt contexts, host side (no GPU): mcm_amd/prompts.py's loader and layouts, the --ctx flags, and the prompt-bank
cache key.  The kernel, the C entry and the end-to-end run are held in tests/test_gpu_ctx.py."""
import types
import warnings
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

BOS, EOS = 49406, 49407
X = 0      # prompts.PLACEHOLDER: the id under a context slot


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)            # the hash tokenizer says that its ids are stand-ins
        yield


def h(word):
    """HashTokenizer's id of a word (mcm_amd/tokenizer.py)."""
    return 1 + zlib.crc32(word.encode()) % (BOS - 1)


# ---- load_context ----------------------------------------------------------------------------------------------------------
def test_load_context_reads_the_three_formats_and_widens_fp16_exactly(tmp_path):
    from mcm_amd.prompts import load_context

    rng = np.random.default_rng(0)
    shared = (0.02 * rng.standard_normal((16, 32))).astype(np.float16)
    per_class = (0.02 * rng.standard_normal((7, 4, 32))).astype(np.float16)
    for arr, per in ((shared, False), (per_class, True)):
        t = torch.from_numpy(arr)
        coop = tmp_path / "model.pth.tar-50"     # CoOp's save_checkpoint: state_dict next to epoch / optimizer / scheduler
        torch.save({"state_dict": {"ctx": t, "token_prefix": torch.zeros(3, 1, 32, dtype=torch.float16),
                                   "token_suffix": torch.zeros(3, 60, 32, dtype=torch.float16)},
                    "epoch": 50, "optimizer": {"state": {}, "param_groups": []}, "scheduler": {"last_epoch": 50}}, coop)
        bare = tmp_path / "ctx.pt"
        torch.save({"ctx": t}, bare)
        npy16, npy32 = tmp_path / "ctx16.npy", tmp_path / "ctx32.npy"
        np.save(npy16, arr)
        np.save(npy32, arr.astype(np.float32))
        for f in (coop, bare, npy16, npy32, str(coop)):
            c = load_context(f)
            assert c.ctx.dtype == np.float32 and c.ctx.flags["C_CONTIGUOUS"]
            assert np.array_equal(c.ctx, arr.astype(np.float32))         # every fp16 number is an fp32 number
            assert (c.n_ctx, c.per_class) == (arr.shape[-2], per)
            assert load_context(f)[1] == c.n_ctx                          # a plain tuple too
    bf = tmp_path / "bf16.pt"
    t = torch.randn(4, 32).to(torch.bfloat16)
    torch.save({"ctx": t}, bf)
    assert np.array_equal(load_context(bf).ctx, t.float().numpy())


def test_load_context_refusals(tmp_path):
    from mcm_amd.prompts import load_context

    def saved(name, obj):
        torch.save(obj, tmp_path / name)
        return tmp_path / name

    with pytest.raises(ValueError, match="no `ctx`"):
        load_context(saved("a.pt", {"state_dict": {"token_prefix": torch.zeros(2, 1, 8)}}))
    with pytest.raises(ValueError, match="no `ctx`"):
        load_context(saved("b.pt", {"weights": torch.zeros(4, 8)}))
    with pytest.raises(ValueError, match="no `ctx`"):
        load_context(saved("c.pt", torch.zeros(4, 8)))                    # a bare tensor is not one of the formats
    for shape in ((8,), (2, 3, 4, 8), (0, 8), (4, 0)):
        with pytest.raises(ValueError, match="n_ctx, width"):
            load_context(saved("d.pt", {"ctx": torch.zeros(shape)}))
        np.save(tmp_path / "d.npy", np.zeros(shape, np.float32))
        with pytest.raises(ValueError, match="n_ctx, width"):
            load_context(tmp_path / "d.npy")
    for bad in (float("nan"), float("inf"), -float("inf")):
        t = torch.zeros(4, 8)
        t[2, 3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            load_context(saved("e.pt", {"state_dict": {"ctx": t.half()}}))
    np.save(tmp_path / "f.npy", np.zeros((4, 8), np.int64))
    with pytest.raises(ValueError, match="floats"):
        load_context(tmp_path / "f.npy")
    # a file that needs arbitrary unpickling is refused with the way out, and nothing of it runs
    marker = tmp_path / "ran"

    class Evil:
        def __reduce__(self):
            return (open, (str(marker), "w"))

    with pytest.raises(ValueError, match=r"re-save the ctx tensor alone as a \.npy"):
        load_context(saved("g.pt", {"state_dict": {"ctx": torch.zeros(4, 8)}, "extra": Evil()}))
    assert not marker.exists()
    (tmp_path / "h.pt").write_bytes(b"not a checkpoint")
    with pytest.raises(ValueError, match=r"\.npy"):
        load_context(tmp_path / "h.pt")


# ---- context_prompts -------------------------------------------------------------------------------------------------------
def test_context_prompts_three_positions_by_hand():
    """HashTokenizer: one id per whitespace-separated word, the period staying on the last word — so the name's last token, the
    one that CoOp's layouts keep behind the context in `middle` and `front`, is that word."""
    from mcm_amd.prompts import PLACEHOLDER, context_prompts
    from mcm_amd.tokenizer import HashTokenizer

    assert PLACEHOLDER == X and X < EOS
    tok, labels = HashTokenizer(), ["toilet_paper", "great white shark", "Ox"]
    tp, pp = h("toilet"), h("paper.")                         # the underscore became a space; "toilet_paper." would be one word
    g, wh, sh, ox = h("great"), h("white"), h("shark."), h("ox.")
    E = EOS
    ids, slots = context_prompts(tok, labels, 4, "end")
    assert ids.dtype == np.int32 and slots.dtype == np.int32
    assert ids.tolist() == [[BOS, X, X, X, X, tp, pp, E, E], [BOS, X, X, X, X, g, wh, sh, E], [BOS, X, X, X, X, ox, E, E, E]]
    assert slots.tolist() == [[-1, 0, 1, 2, 3, -1, -1, -1, -1]] * 3
    ids, slots = context_prompts(tok, labels, 5, "middle")    # half = 2: two rows in front of the name, three behind it
    assert ids.tolist() == [[BOS, X, X, tp, X, X, X, pp, E, E], [BOS, X, X, g, wh, X, X, X, sh, E], [BOS, X, X, X, X, X, ox, E, E, E]]
    assert slots.tolist() == [[-1, 0, 1, -1, 2, 3, 4, -1, -1, -1], [-1, 0, 1, -1, -1, 2, 3, 4, -1, -1], [-1, 0, 1, 2, 3, 4, -1, -1, -1, -1]]
    ids, slots = context_prompts(tok, labels, 2, "front")
    assert ids.tolist() == [[BOS, tp, X, X, pp, E, E], [BOS, g, wh, X, X, sh, E], [BOS, X, X, ox, E, E, E]]
    assert slots.tolist() == [[-1, -1, 0, 1, -1, -1, -1], [-1, -1, -1, 0, 1, -1, -1], [-1, 0, 1, -1, -1, -1, -1]]
    ids, slots = context_prompts(tok, ["ox"], 1, "middle")    # half = 0: no row in front of the name
    assert ids.tolist() == [[BOS, X, ox, E]] and slots.tolist() == [[-1, 0, -1, -1]]


@pytest.mark.parametrize("position", ["end", "middle", "front"])
@pytest.mark.parametrize("n_ctx", [1, 4, 16])
def test_context_prompts_pool_at_eos_and_keep_every_slot_in_front_of_it(position, n_ctx):
    from mcm_amd.prompts import context_prompts
    from mcm_amd.tokenizer import HashTokenizer

    labels = ["tench", "toilet_paper", "great_white_shark", "a_b_c_d_e_f_g"]
    ids, slots = context_prompts(HashTokenizer(), labels, n_ctx, position)
    assert ids.shape == slots.shape == (4, 1 + n_ctx + 7 + 1) and (ids[:, 0] == BOS).all()
    first_eos = ids.argmax(axis=1)                            # the pooled row: the first position of the largest id
    for k in range(4):
        assert ids[k].max() == EOS and ids[k, first_eos[k]] == EOS
        assert (ids[k, first_eos[k]:] == EOS).all()           # padded with EOS, as the tokenizer pads
        where = np.nonzero(slots[k] >= 0)[0]
        assert slots[k, where].tolist() == list(range(n_ctx)) and where.max() < first_eos[k] - 1   # the "." and EOS follow
        assert (ids[k, where] == X).all() and (ids[k, slots[k] < 0] != X).all()
        words = (labels[k].replace("_", " ") + ".").split()
        assert ids[k, (slots[k] < 0) & (np.arange(ids.shape[1]) < first_eos[k])].tolist() == [BOS] + [h(w) for w in words]


def test_context_prompts_refusals():
    from mcm_amd.prompts import context_prompts
    from mcm_amd.tokenizer import HashTokenizer

    tok = HashTokenizer()
    ids, _ = context_prompts(tok, ["_".join(["w"] * 59)], 16, "end")      # 1 + 16 + 59 + 1 = 77 still fits
    assert ids.shape == (1, 77)
    for position in ("end", "middle", "front"):
        with pytest.raises(ValueError, match="77"):
            context_prompts(tok, ["ox", "_".join(["w"] * 60)], 16, position)
    with pytest.raises(ValueError, match="position"):
        context_prompts(tok, ["ox"], 4, "back")
    with pytest.raises(ValueError, match="n_ctx"):
        context_prompts(tok, ["ox"], 0, "end")


# ---- the CLI's flags ---------------------------------------------------------------------------------------------------------
def test_cli_flags_defaults_and_refusals(tmp_path, monkeypatch):
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    words = tmp_path / "words.txt"
    words.write_text("a\nb\n")
    tmpl = tmp_path / "t.txt"
    tmpl.write_text("a photo of a {c}\n")
    extra = {"neglabel": ["--neg-words", str(words)]}
    for score in ("MCM", "energy", "max-logit", "entropy", "var", "maha", "knn", "neglabel", "GL-MCM", "vim"):
        a = cli.process_args(["--in_dataset", "ImageNet10", "--score", score] + extra.get(score, []))
        assert (a.ctx, a.ctx_position, a.ctx_T, a.T) == (None, "end", 0.01, 1)
        # without --ctx the other two flags parse and change nothing, whatever they hold
        a = cli.process_args(["--in_dataset", "ImageNet10", "--score", score, "--ctx-position", "front", "--ctx-T", "-3", "--T", "2"]
                             + extra.get(score, []))
        assert (a.ctx, a.ctx_position, a.ctx_T, a.T) == (None, "front", -3.0, 2)
    base = ["--in_dataset", "ImageNet10", "--ctx", "some.pth"]
    for score in ("MCM", "energy", "max-logit", "entropy", "var", "GL-MCM"):
        a = cli.process_args(base + ["--score", score, "--T", "5"])
        assert (a.ctx, a.ctx_position, a.ctx_T) == ("some.pth", "end", 0.01)
        assert a.T == 0.01                                     # --T is ignored: the scores read --ctx-T
        a = cli.process_args(base + ["--score", score, "--ctx-position", "middle", "--ctx-T", "0.05"])
        assert (a.ctx_position, a.T) == ("middle", 0.05)
    a = cli.process_args(base + ["--score", "vim", "--T", "5", "--vim-T", "0.02"])
    assert (a.T, a.vim_T, a.ctx) == (5, 0.02, "some.pth")      # vim's logits keep --vim-T
    assert cli.process_args(base + ["--predict", "3"]).predict == 3
    for bad in (["--templates", str(tmpl)], ["--score", "maha"], ["--score", "knn"], ["--score", "neglabel", "--neg-words", str(words)],
                ["--ctx-T", "0"], ["--ctx-T", "-1"], ["--ctx-T", "inf"], ["--ctx-T", "nan"], ["--ctx-position", "back"]):
        with pytest.raises(SystemExit):
            cli.process_args(base + bad)


# ---- prompt_bank ---------------------------------------------------------------------------------------------------------------
class _Net:
    """Counts encodes; a context call returns the prompts' slot counts so that the layout that reached it can be read back."""
    synthetic_weights = True

    def __init__(self):
        self.plain, self.ctx_calls = 0, []

    def get_text_features(self, input_ids, attention_mask=None, normalize=False):
        self.plain += 1
        return torch.ones(input_ids.shape[0], 4)

    def get_text_features_ctx(self, input_ids, slots, ctx, normalize=False):
        assert normalize is True and input_ids.shape == slots.shape and ctx.dtype == np.float32
        self.ctx_calls.append((np.asarray(input_ids).copy(), np.asarray(slots).copy(), np.asarray(ctx).copy()))
        return torch.full((input_ids.shape[0], 4), float(len(self.ctx_calls)))


def test_prompt_bank_encodes_once_per_labels_file_and_position(tmp_path):
    from mcm_amd import detection
    from mcm_amd.prompts import context_prompts
    from mcm_amd.tokenizer import HashTokenizer

    f1, f2, per = tmp_path / "a.npy", tmp_path / "b.npy", tmp_path / "csc.npy"
    np.save(f1, np.full((4, 8), 1.0, np.float16))
    np.save(f2, np.full((2, 8), 2.0, np.float32))
    np.save(per, np.full((3, 2, 8), 3.0, np.float32))
    net, labels = _Net(), ["cat", "dog"]
    args = types.SimpleNamespace(ckpt="x", templates=None, ctx=str(f1), ctx_position="end")
    a = detection.prompt_bank(args, net, labels)
    assert detection.prompt_bank(args, net, labels) is a and len(net.ctx_calls) == 1 and net.plain == 0
    ids, slots, ctx = net.ctx_calls[0]
    want = context_prompts(HashTokenizer(), labels, 4, "end")
    assert np.array_equal(ids, want[0]) and np.array_equal(slots, want[1]) and np.array_equal(ctx, np.ones((4, 8), np.float32))
    args.ctx_position = "front"                                # another position: re-encoded
    detection.prompt_bank(args, net, labels)
    assert len(net.ctx_calls) == 2 and np.array_equal(net.ctx_calls[1][1], context_prompts(HashTokenizer(), labels, 4, "front")[1])
    args.ctx = str(f2)                                         # another file
    detection.prompt_bank(args, net, labels)
    assert len(net.ctx_calls) == 3 and net.ctx_calls[2][2].shape == (2, 8)
    detection.prompt_bank(args, net, labels + ["eel"])         # other labels
    assert len(net.ctx_calls) == 4
    detection.prompt_bank(args, net, labels + ["eel"])
    assert len(net.ctx_calls) == 4
    args.ctx = str(per)                                        # a per-class context: its first dimension is the label count
    assert detection.prompt_bank(args, net, labels + ["eel"]).shape == (3, 4) and net.ctx_calls[4][2].shape == (3, 2, 8)
    with pytest.raises(ValueError, match="per-class"):
        detection.prompt_bank(args, net, labels)
    del args.ctx_position                                      # a caller that sets only `ctx`: the default layout
    detection.prompt_bank(args, net, labels + ["eel"])
    assert np.array_equal(net.ctx_calls[-1][1], context_prompts(HashTokenizer(), labels + ["eel"], 2, "end")[1])
    args.templates = ["a {c}"]
    with pytest.raises(ValueError, match="exclude"):
        detection.prompt_bank(args, net, labels)
    assert net.plain == 0


def test_prompt_bank_without_ctx_is_what_it_was():
    from mcm_amd import detection

    labels = ["cat", "dog"]
    key = (("cat", "dog"), None, "x")                          # the key of the parent commit, to the element
    for args in (types.SimpleNamespace(ckpt="x", templates=None), types.SimpleNamespace(ckpt="x", templates=None, ctx=None),
                 types.SimpleNamespace(ckpt="x", templates=None, ctx=None, ctx_position="front")):
        net = _Net()
        a = detection.prompt_bank(args, net, labels)
        assert detection.prompt_bank(args, net, labels) is a and net.plain == 1 and not net.ctx_calls
        assert list(net._bank_cache) == [key]
