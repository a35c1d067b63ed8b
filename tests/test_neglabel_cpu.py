"""The host side of `--score neglabel` on the CPU, through a stub net whose features are a function of the token ids / pixels,
whose `knn_scores` is torch top-k and whose `neglabel_scores` is the definition in fp64: the mining against brute-force
`torch.quantile` in fp64, `get_neglabel_bank` / `get_neglabel_score` against the direct computation in one process and under gloo
at world sizes 2 and 3 (empty and ragged shards), and the CLI's switches and refusals."""
import os
import socket
import types
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

P, BS = 8, 8


class _Set(torch.utils.data.Dataset):
    def __init__(self, n, seed):
        self.n, self.seed = n, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed + int(i))
        return torch.randn(3, 4, 4, generator=g), int(i) % 3


class _StubNet:
    """Text features = a function of the unpadded token ids (not unit: the routines must normalise); image features = the
    first P pixel values plus 0.5; knn_scores = torch top-k of the fp64 similarities, returned as fp32 like the device's;
    neglabel_scores = the definition in fp64.  `table`: word -> feature row overrides (ties, planted distances)."""

    def __init__(self, table=None):
        self.table = table or {}

    def get_text_features(self, input_ids, attention_mask=None):
        ids = input_ids.double() * attention_mask.double()
        freq = torch.arange(1, P + 1, dtype=torch.float64) * 0.37
        f = torch.sin(ids[:, :, None] * freq[None, None, :] * 1e-3).sum(dim=1) + 0.05
        for row_ids, feat in self.table.values():
            hit = [i for i in range(ids.shape[0]) if [int(t) for t, m in zip(input_ids[i], attention_mask[i]) if m] == row_ids]
            for i in hit:
                f[i] = torch.as_tensor(feat, dtype=torch.float64)
        return f.float()

    def get_image_features(self, pixel_values):
        return pixel_values.reshape(pixel_values.shape[0], -1)[:, :P].float() + 0.5

    def knn_scores(self, features, bank, k, splits=0, return_values=False):
        v = torch.topk(features.double() @ bank.double().T, int(k), dim=1).values
        s = torch.sqrt(torch.clamp(2.0 - 2.0 * v[:, -1], min=0.0)).float()
        return (s, v.float()) if return_values else s

    def neglabel_scores(self, features, bank, n_id, groups, group_size, T=0.01, splits=0, return_groups=False):
        logit = features.double() @ bank.double().T / float(np.float32(T))
        LI = torch.logsumexp(logit[:, :n_id], dim=1)
        LN = torch.logsumexp(logit[:, n_id:].reshape(-1, groups, group_size), dim=2)
        S = 1.0 / (1.0 + torch.exp(LN - LI[:, None]))
        s = (-S.mean(dim=1)).float()
        return (s, S.float()) if return_groups else s


def _args(**kw):
    base = dict(model="CLIP", normalize=False, feat_dim=P, batch_size=BS, ckpt="", weights=None, neg_count=0, neg_frac=0.15,
                neg_quantile=0.95, neg_groups=100, neg_T=0.01)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _loader(n, seed):
    return torch.utils.data.DataLoader(_Set(n, seed), batch_size=BS, shuffle=False)


def _tok_ids(word):
    """The unpadded hash-tokenizer ids of a word's prompt (the key of _StubNet.table)."""
    from mcm_amd.detection import PROMPT
    from mcm_amd.tokenizer import HashTokenizer

    t = HashTokenizer()([PROMPT.format(c=word)], padding=True, return_tensors="pt")
    return [int(x) for x in t["input_ids"][0]]


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-30)


def _text(net, words):
    from mcm_amd.detection import PROMPT
    from mcm_amd.tokenizer import HashTokenizer

    t = HashTokenizer()([PROMPT.format(c=w) for w in words], padding=True, return_tensors="pt")
    return _unit(net.get_text_features(input_ids=t["input_ids"], attention_mask=t["attention_mask"]).float())


def _brute_force(net, id_names, cands, q, M, G):
    """(selected words, their d) by torch.quantile in fp64 on the similarities the device would return (fp32 values)."""
    sim = (_text(net, cands).double() @ _text(net, id_names).double().T).float().double()
    d = torch.quantile(sim, q, dim=1, interpolation="linear").numpy()
    order = sorted(range(len(cands)), key=lambda i: (d[i], i))[:M]
    G = min(G, M)
    order = order[:G * (M // G)]
    return [cands[i] for i in order], d[order], G, M // G


def _words(n, prefix="w"):
    return [f"{prefix}{i:03d}x" for i in range(n)]


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # the hash tokenizer says that its ids are stand-ins
        yield


@pytest.mark.parametrize("K,q", [(7, 0.95), (7, 0.5), (5, 0.75), (1, 0.95), (4, 0.0), (4, 1.0), (30, 0.9)])
def test_mining_equals_brute_force_quantile(K, q):
    """q (K - 1): 5.7, 3 (an integer), 3 (an integer), 0 (K = 1), 0, 3 (the maximum), 26.1."""
    from mcm_amd.detection import mine_negative_labels

    net, ids, cands = _StubNet(), _words(K, "id"), _words(40)
    words, d = mine_negative_labels(_args(neg_quantile=q, neg_count=12, neg_groups=3), net, ids, cands)
    want_w, want_d, _, _ = _brute_force(net, ids, cands, q, 12, 3)
    assert words == want_w and d.dtype == np.float64
    np.testing.assert_allclose(d, want_d, rtol=1e-13, atol=1e-15)


def test_cleaning_duplicates_id_names_and_the_trim():
    from mcm_amd.detection import clean_negative_words, get_neglabel_bank, mine_negative_labels

    ids = ["Dog", "cat ", "sea lion"]
    raw = ["  apple ", "", "DOG", "pear", "Apple", "   ", "cat", "plum", "sea lion", "fig", "pear", "kiwi", "lime", "date"]
    cands = clean_negative_words(raw, ids)
    assert cands == ["apple", "pear", "plum", "fig", "kiwi", "lime", "date"]
    net = _StubNet()
    # M = 7 kept, G = 3 groups of gs = 2: the last word of the selection order is dropped
    words, d = mine_negative_labels(_args(neg_count=7, neg_groups=3), net, ids, raw)
    want_w, want_d, G, gs = _brute_force(net, ids, cands, 0.95, 7, 3)
    assert (G, gs) == (3, 2) and words == want_w and len(words) == 6 and (np.diff(d) >= 0).all()
    np.testing.assert_allclose(d, want_d, rtol=1e-13)
    # --neg-frac: round(0.15 x 7) = 1 word, one group of one; G > M: as many groups as words
    info = get_neglabel_bank(_args(), net, ids, raw)
    assert (info["K"], info["C"], info["M"], info["G"], info["gs"]) == (3, 7, 1, 1, 1) and info["bank"].shape == (4, P)
    info = get_neglabel_bank(_args(neg_count=5, neg_groups=100), net, ids, raw)
    assert (info["M"], info["G"], info["gs"]) == (5, 5, 1) and len(info["words"]) == 5
    info = get_neglabel_bank(_args(neg_count=50), net, ids, raw)                    # more asked for than there are
    assert (info["M"], info["G"], info["gs"]) == (7, 7, 1)


def test_ties_are_ordered_by_candidate_index():
    from mcm_amd.detection import mine_negative_labels

    ids, cands = _words(3, "id"), _words(8)
    same = [0.3, -0.2, 0.1, 0.4, 0.0, 0.2, -0.1, 0.5]
    table = {w: (_tok_ids(w), same) for w in (cands[6], cands[1], cands[4])}        # three candidates with the same feature
    net = _StubNet(table)
    words, d = mine_negative_labels(_args(neg_count=8, neg_groups=8), net, ids, cands)
    want_w, want_d, _, _ = _brute_force(net, ids, cands, 0.95, 8, 8)
    assert words == want_w
    pos = [words.index(cands[i]) for i in (1, 4, 6)]
    assert pos == [pos[0], pos[0] + 1, pos[0] + 2] and d[pos[0]] == d[pos[1]] == d[pos[2]]   # equal d: index order, adjacent


def test_refusals():
    from mcm_amd.detection import get_neglabel_score, mine_negative_labels

    net = _StubNet()
    with pytest.raises(ValueError, match="1024"):                                    # k = K - floor(0.0 x 1099) = 1100
        mine_negative_labels(_args(neg_quantile=0.0), net, _words(1100, "id"), _words(5))
    with pytest.raises(ValueError, match="candidate"):                               # nothing is left after cleaning
        mine_negative_labels(_args(), net, ["a", "b"], ["A", " b ", ""])
    with pytest.raises(ValueError, match="kept"):                                    # round(0.01 x 5) = 0
        mine_negative_labels(_args(neg_frac=0.01), net, ["a", "b"], _words(5))
    with pytest.raises(TypeError, match="knn_scores"):
        mine_negative_labels(_args(), types.SimpleNamespace(), ["a"], _words(5))
    with pytest.raises(TypeError, match="neglabel_scores"):
        get_neglabel_score(_args(), types.SimpleNamespace(), _loader(3, 900), {"bank": torch.zeros(2, P), "K": 1, "G": 1, "gs": 1})


def _direct(n_test, ids, cands, a):
    net = _StubNet()
    words, _, G, gs = _brute_force(net, ids, cands, a.neg_quantile, a.neg_count, a.neg_groups)
    bank = torch.cat([_text(net, ids), _text(net, words)])
    f = torch.cat([_unit(net.get_image_features(x)) for x, _ in _loader(n_test, 900)])
    return bank, words, net.neglabel_scores(f, bank, len(ids), G, gs, T=a.neg_T).numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


IDS, CANDS = _words(6, "id"), _words(3, "only") + _words(50)


@pytest.mark.parametrize("n_cand,n_test", [(3, 3), (53, 21)])
def test_single_process_equals_the_direct_computation(n_cand, n_test):
    from mcm_amd.detection import get_neglabel_bank, get_neglabel_score

    a = _args(neg_count=min(n_cand, 20), neg_groups=4)
    net = _StubNet()
    info = get_neglabel_bank(a, net, IDS, CANDS[:n_cand])
    want_bank, want_words, want = _direct(n_test, IDS, CANDS[:n_cand], a)
    assert info["words"] == want_words and info["bank"].dtype == torch.float32
    assert np.array_equal(_bits(info["bank"].numpy()), _bits(want_bank.numpy()))
    got = get_neglabel_score(a, net, _loader(n_test, 900), info)
    assert got.dtype == np.float32 and got.shape == (n_test,) and np.array_equal(_bits(got), _bits(want))


# ---- gloo ---------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, ws, port, n_cand, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank))
    warnings.simplefilter("ignore", RuntimeWarning)
    import torch.distributed as dist

    from mcm_amd.detection import get_neglabel_bank, get_neglabel_score

    dist.init_process_group("gloo", rank=rank, world_size=ws)
    a = _args(neg_count=min(n_cand, 20), neg_groups=4)
    net = _StubNet()
    info = get_neglabel_bank(a, net, IDS, CANDS[:n_cand])
    scores = {n: get_neglabel_score(a, net, _loader(n, 900), info) for n in (3, 21)}
    q.put((rank, info["bank"].numpy(), info["words"], scores[3], scores[21]))
    dist.destroy_process_group()


@pytest.mark.parametrize("ws,n_cand", [(2, 3), (3, 3), (2, 53), (3, 53)])
def test_gloo_shards_equal_single_process(ws, n_cand):
    """3 candidates on three ranks: shards of one word, on two ranks 2 + 1; a test set of 3 leaves a rank of a 21 / 3 split
    ragged batches (and, on two ranks of 2 + 1, 3 samples on three ranks of 1); 53 candidates: 27 + 26 and 18 + 18 + 17.  The
    bank is the same bits on every rank and at every world size, the scores equal the single-process run bit for bit."""
    a = _args(neg_count=min(n_cand, 20), neg_groups=4)
    want_bank, want_words, want3 = _direct(3, IDS, CANDS[:n_cand], a)
    _, _, want21 = _direct(21, IDS, CANDS[:n_cand], a)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, ws, port, n_cand, q)) for r in range(ws)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, bank, words, s3, s21 in got:
        assert words == want_words, rank
        assert np.array_equal(_bits(bank), _bits(want_bank.numpy())), rank
        assert np.array_equal(_bits(s3), _bits(want3)) and np.array_equal(_bits(s21), _bits(want21)), rank


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_switches_and_refusals(tmp_path, monkeypatch):
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    base = ["--in_dataset", "ImageNet10", "--score", "neglabel", "--neg-words", "words.txt"]
    a = cli.process_args(base)
    assert a.score == "neglabel" and a.neg_words == "words.txt"
    assert (a.neg_count, a.neg_frac, a.neg_quantile, a.neg_groups, a.neg_T) == (0, 0.15, 0.95, 100, 0.01)
    a = cli.process_args(base + ["--neg-count", "300", "--neg-frac", "0.5", "--neg-quantile", "0.9", "--neg-groups", "7", "--neg-T",
                                 "0.05", "--T", "3"])
    assert (a.neg_count, a.neg_frac, a.neg_quantile, a.neg_groups, a.neg_T, a.T) == (300, 0.5, 0.9, 7, 0.05, 3)
    assert cli.process_args(base + ["--refine-threshold", "auto"]).score == "neglabel"
    assert cli.process_args(["--in_dataset", "ImageNet10"]).neg_T == 0.01            # the flags exist for every score
    for bad in (["--predict"], ["--refine-threshold", "on"], ["--refine-threshold", "exact"], ["--neg-groups", "0"],
                ["--neg-groups", "1025"], ["--neg-T", "0"], ["--neg-T", "-1"], ["--neg-T", "inf"], ["--neg-frac", "0"],
                ["--neg-frac", "1.5"], ["--neg-quantile", "1.1"], ["--neg-count", "-1"]):
        with pytest.raises(SystemExit):
            cli.process_args(base + bad)
    with pytest.raises(SystemExit):                                                  # --neg-words is required with this score
        cli.process_args(["--in_dataset", "ImageNet10", "--score", "neglabel"])
