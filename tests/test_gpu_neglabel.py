"""The NegLabel score on a real MI355X: mcm_neglabel_score_features (neglabel.hip) against the fp64 reference and the derived
budget of tests/neglabel_budget.py — the arithmetic term plus one ulp on lattice inputs (every similarity exact in fp32), the
full budget on unit inputs — its determinism, NaN and refusal contract, the method's own size, and mining, bank, scoring and the
CLI end to end.  Budget cases print "BUDGET neglabel <worst ratio> ..." (run with -s to collect them)."""
import ctypes
import types

import numpy as np
import pytest

from tests import gpu_scaffold  # (not "as gs": gs is the group size here)
from tests import neglabel_budget as nb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_dev = gpu_scaffold.dev
_bits = gpu_scaffold.bits

WIDTHS = [64, 512, 768, 1024]
# (B, K, G, gs).  (1,1,1,1): two rows, so five of seven splits are empty; (3,300,1,1): the ID range across the tile edge at 256
# and a one-row group behind it; (64,37,7,100): several ranges inside a tile, groups across both tile edges; (65,256,2,256): every
# range ends on a tile edge; (130,257,100,3): the ID range one row past the edge, 86 ranges inside a tile, a ragged third query
# tile; (65,1000,3,301): ranges of several tiles.  With 2 and 7 splits the ID range and groups also lie across split boundaries.
SHAPES = [(1, 1, 1, 1), (3, 300, 1, 1), (64, 37, 7, 100), (65, 256, 2, 256), (130, 257, 100, 3), (65, 1000, 3, 301)]
SPLITS = [1, 2, 7, 0]
TEMPS = [0.01, 1.0]


@pytest.fixture(scope="module")
def neg_nets():
    yield from gpu_scaffold.net_cache()


def _run(net, f, bank, K, G, gs, T, splits=0):
    s, g = net.neglabel_scores(f, bank, K, G, gs, T=T, splits=splits, return_groups=True)
    return s.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("P", WIDTHS)
def test_lattice_inputs_within_the_arithmetic_term(neg_nets, P):
    net = neg_nets(P)
    worst, cases = 0.0, 0
    for B, K, G, gs in SHAPES:
        f, bank = nb.lattice_case(B, K, G, gs, P, seed=B + K + G)
        fd, bd = _dev(f), _dev(bank)
        for T in TEMPS:
            S, score, _ = nb.reference(f, bank, K, G, gs, T)
            bS, bs = nb.budgets(f, bank, K, G, gs, T, exact=True)
            for splits in SPLITS:
                s, g = _run(net, fd, bd, K, G, gs, T, splits)
                rS, rs = nb.ratio(g, S, bS), nb.ratio(s, score, bs)
                worst, cases = max(worst, rS, rs), cases + 1
                assert rS <= 1.0 and rs <= 1.0, (P, B, K, G, gs, T, splits, rS, rs)
    print(f"BUDGET neglabel {worst:.3f} lattice (arithmetic term + one ulp) P={P}: {cases} cases")


@pytest.mark.parametrize("P", [64, 512])
def test_unit_inputs_within_budget(neg_nets, P):
    net = neg_nets(P)
    B, K, G, gs = 65, 37, 7, 100
    f, bank = nb.unit_case(B, K, G, gs, P, seed=P)
    fd, bd = _dev(f), _dev(bank)
    for T in TEMPS:
        S, score, _ = nb.reference(f, bank, K, G, gs, T)
        bS, bs = nb.budgets(f, bank, K, G, gs, T)
        per_split = {}
        for splits in SPLITS:
            s, g = _run(net, fd, bd, K, G, gs, T, splits)
            rS, rs = nb.ratio(g, S, bS), nb.ratio(s, score, bs)
            print(f"BUDGET neglabel {max(rS, rs):.3f} (groups {rS:.3f}, scores {rs:.3f}) unit P={P} B=65 K=37 G=7 gs=100 T={T} "
                  f"splits={splits}; S in [{S.min():.2e}, {S.max():.6f}]")
            assert rS <= 1.0 and rs <= 1.0, (P, T, splits, rS, rs)
            # the score is the fp64 mean of the group values that were written, within one ulp
            mean = -g.astype(np.float64).mean(axis=1)
            assert (np.abs(s.astype(np.float64) - mean) <= np.spacing(np.abs(mean).astype(np.float32))).all(), (P, T, splits)
            per_split[splits] = (s, g)
        # across splits the similarities are the same bits and only the sums are associated differently: two results differ
        # by at most twice the arithmetic term plus one ulp
        xS, xs = nb.budgets(f, bank, K, G, gs, T, exact=True)
        for a in (2, 7):
            assert (np.abs(per_split[a][0].astype(np.float64) - per_split[1][0]) <= 2 * xs).all(), (P, T, a)
            assert (np.abs(per_split[a][1].astype(np.float64) - per_split[1][1]) <= 2 * xS).all(), (P, T, a)


def test_same_bits_over_runs_query_cuts_and_row_positions(neg_nets):
    net = neg_nets(512)
    B, K, G, gs = 130, 257, 100, 3
    f, bank = nb.unit_case(B, K, G, gs, 512, seed=5)
    fd, bd = _dev(f), _dev(bank)
    for splits in (1, 2, 7):
        s1, g1 = _run(net, fd, bd, K, G, gs, 0.01, splits)
        for _ in range(2):                                                              # three runs in all
            s, g = _run(net, fd, bd, K, G, gs, 0.01, splits)
            assert np.array_equal(_bits(s), _bits(s1)) and np.array_equal(_bits(g), _bits(g1)), splits
        parts = [_run(net, fd[a:a + n], bd, K, G, gs, 0.01, splits) for a, n in ((0, 64), (64, 65), (129, 1))]
        assert np.array_equal(_bits(np.concatenate([p[0] for p in parts])), _bits(s1)), splits
        assert np.array_equal(_bits(np.concatenate([p[1] for p in parts])), _bits(g1)), splits
        perm = np.random.default_rng(splits).permutation(B)
        s, g = _run(net, _dev(f[perm]), bd, K, G, gs, 0.01, splits)
        assert np.array_equal(_bits(s), _bits(s1[perm])) and np.array_equal(_bits(g), _bits(g1[perm])), splits


def test_a_nan_query_row_gives_a_nan_score_for_that_row_only(neg_nets):
    net = neg_nets(64)
    B, K, G, gs = 5, 37, 7, 100
    f, bank = nb.unit_case(B, K, G, gs, 64, seed=3)
    fq = f.copy()
    fq[2, 7] = np.nan
    for splits in (1, 3):
        s0, g0 = _run(net, _dev(f), _dev(bank), K, G, gs, 0.01, splits)
        s, g = _run(net, _dev(fq), _dev(bank), K, G, gs, 0.01, splits)
        keep = [0, 1, 3, 4]
        assert np.isnan(s[2]) and np.isnan(g[2]).all()
        assert np.array_equal(_bits(s[keep]), _bits(s0[keep])) and np.array_equal(_bits(g[keep]), _bits(g0[keep]))
    bn = bank.copy()
    bn[K + 2 * gs + 5, 0] = np.nan                                                      # one NaN bank row, in group 2
    s, g = _run(net, _dev(f), _dev(bn), K, G, gs, 0.01, 2)
    assert np.isnan(s).all() and np.isnan(g[:, 2]).all() and np.isfinite(np.delete(g, 2, axis=1)).all()


def test_refused_calls_launch_nothing(neg_nets):
    from mcm_amd.engine import _stream_ptr

    net, P = neg_nets(64), 64
    B, K, G, gs = 5, 37, 7, 100
    f, bank = nb.unit_case(B, K, G, gs, P, seed=3)
    fd, bd = _dev(f), _dev(bank)
    work = torch.full((32 * B * (G + 1) * 2,), 7.5, device="cuda")
    out = torch.full((B,), -2.5, device="cuda")
    grp = torch.full((B, G), -3.5, device="cuda")
    call, sp = net._lib.mcm_neglabel_score_features, _stream_ptr
    wb = work.numel() * 4

    def go(h=net._h, fp=fd.data_ptr(), B=B, bp=bd.data_ptr(), K=K, G=G, gs=gs, T=0.01, splits=2, wp=work.data_ptr(), nbytes=wb,
           op=out.data_ptr(), gp=grp.data_ptr()):
        return call(h, fp, B, bp, K, G, gs, T, splits, wp, nbytes, op, gp, sp())

    assert go(h=None) == -1
    assert go(fp=None) == -1 and go(bp=None) == -1 and go(wp=None) == -1 and go(op=None) == -1
    assert go(B=0) == -1 and go(B=-1) == -1 and go(K=0) == -1 and go(K=-3) == -1
    assert go(G=0) == -1 and go(G=1025) == -1 and go(gs=0) == -1 and go(gs=-1) == -1
    assert go(T=0.0) == -1 and go(T=-0.01) == -1 and go(T=float("inf")) == -1 and go(T=float("nan")) == -1
    assert go(splits=-1) == -1 and go(splits=33) == -1
    assert go(nbytes=2 * B * (G + 1) * 8 - 1) == -1
    assert go(fp=fd.data_ptr() + 4) == -1 and go(bp=bd.data_ptr() + 8) == -1            # rows are read 16 bytes at a time
    assert go(K=2 ** 31 - 1 - 699) == -1 and go(G=1024, gs=2 ** 21) == -1               # K + G gs = 2^31 and 2^31 + 37
    need = ctypes.c_int64(-1)
    wbytes = net._lib.mcm_neglabel_workspace_bytes
    assert wbytes(net._h, B, K, G, gs, 33, ctypes.byref(need)) == -1 and wbytes(net._h, B, K, 0, gs, 1, ctypes.byref(need)) == -1
    assert wbytes(None, B, K, G, gs, 1, ctypes.byref(need)) == -1 and wbytes(net._h, B, K, G, gs, 1, None) == -1
    assert wbytes(net._h, B, K, 1024, 2 ** 21, 1, ctypes.byref(need)) == -1
    assert need.value == -1
    assert wbytes(net._h, B, K, G, gs, 2, ctypes.byref(need)) == 0 and need.value == 2 * B * (G + 1) * 8
    assert wbytes(net._h, B, K, G, gs, 0, ctypes.byref(need)) == 0 and need.value % (B * (G + 1) * 8) == 0
    assert 1 <= need.value // (B * (G + 1) * 8) <= 32
    torch.cuda.synchronize()
    assert (work == 7.5).all() and (out == -2.5).all() and (grp == -3.5).all()
    with pytest.raises(ValueError):
        net.neglabel_scores(fd, bd, K, G, gs + 1)                                       # the bank does not hold K + G gs rows
    with pytest.raises(ValueError):
        net.neglabel_scores(fd, bd, K, G, gs, T=0.0)
    with pytest.raises(ValueError):
        net.neglabel_scores(fd[:, :60], bd, K, G, gs)
    assert go(gp=None) == 0                                                             # group_dev is optional
    torch.cuda.synchronize()
    assert (out != -2.5).all() and (grp == -3.5).all()
    first = out.clone()
    assert go() == 0                                                                    # the same buffers take a good call
    torch.cuda.synchronize()
    assert torch.equal(out, first) and (grp != -3.5).all()
    # no word of the workspace is read before it is written: a NaN-filled one gives the same bits (7 splits of 106 rows:
    # most (split, range) slots are never written)
    for fill in (float("nan"), 3.0e38):
        work.fill_(fill)
        assert go(splits=7) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and torch.isfinite(grp).all()
        s7, g7 = _run(net, fd, bd, K, G, gs, 0.01, 7)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(s7)) and np.array_equal(_bits(grp.cpu().numpy()), _bits(g7))


def test_the_methods_own_size_against_torch_fp64():
    """B = 512, K = 1000, G = 100, gs = 100 (N = 11 000), P = 512, T = 0.01, the library choosing the splits: the fp64
    similarities and eps come from torch on the device."""
    net = gpu_scaffold.widened_net(512)
    B, K, G, gs, T = 512, 1000, 100, 100, 0.01
    f, bank = nb.unit_case(B, K, G, gs, 512, seed=1)
    fd, bd = _dev(f), _dev(bank)
    s64 = (fd.double() @ bd.double().T).cpu().numpy()
    gamma = 512 * nb.U / (1.0 - 512 * nb.U)
    eps = gamma * (fd.double().abs() @ bd.double().abs().T).max(dim=1).values.cpu().numpy()
    S, score, _ = nb.reference_from_similarities(s64, K, G, gs, T)
    bS, bs = nb.budgets_from_similarities(s64, eps, K, G, gs, T)
    s, g = _run(net, fd, bd, K, G, gs, T, 0)
    rS, rs = nb.ratio(g, S, bS), nb.ratio(s, score, bs)
    print(f"BUDGET neglabel {max(rS, rs):.3f} (groups {rS:.3f}, scores {rs:.3f}) unit P=512 B=512 K=1000 G=100 gs=100 T=0.01 splits=0")
    net.close()
    assert rS <= 1.0 and rs <= 1.0, (rS, rs)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _tiny(precision):
    from mcm_amd.config import TEST_GEOMETRIES
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = TEST_GEOMETRIES["tiny"]
    return NativeCLIP(geo, synth_state_dict(geo, seed=0), precision=precision, max_batch=64, max_prompt_tokens=64 * 16)


def _generated_words(n):
    rng = np.random.default_rng(12)
    return ["".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz"), size=int(rng.integers(3, 9)))) + f"{i}" for i in range(n)]


def test_end_to_end_against_torch():
    """Mining, bank and scores through detection.py on the tiny geometry's fp32 arm against a torch fp64 restatement on the
    same fp32 features: the same words in the same order, the scores inside the budget."""
    import warnings

    from mcm_amd.detection import PROMPT, get_neglabel_bank, get_neglabel_score, load_tokenizer
    from mcm_amd.synth import make_pixels

    bs, q, M, G, T = 64, 0.95, 45, 6, 0.01
    ids = [f"class{i}" for i in range(10)]
    words = _generated_words(120) + ["Class3", " ", "class7"]                           # two ID names and a blank among them
    args = types.SimpleNamespace(model="CLIP", normalize=False, batch_size=bs, ckpt="", weights=None, neg_count=M, neg_frac=0.15,
                                 neg_quantile=q, neg_groups=G, neg_T=T)
    net = _tiny("fp32")
    geo = net.geo

    class DS:
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

    class Loader:
        def __init__(self, n, ood, seed):
            self.dataset, self.ood, self.seed = DS(n), ood, seed

        def __iter__(self):
            for s in range(0, self.dataset.n, bs):
                n = min(bs, self.dataset.n - s)
                px, lab = make_pixels(n, geo.image_size, 10, ood=self.ood, seed=self.seed, start=s)
                yield torch.from_numpy(px), torch.from_numpy(lab)

    sets = {"id": Loader(70, False, 1), "ood": Loader(64, True, 2)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                                 # the hash tokenizer's stand-in ids
        info = get_neglabel_bank(args, net, ids, words)
        got = {w: get_neglabel_score(args, net, ld, info) for w, ld in sets.items()}
        tok = load_tokenizer("", allow_hash=True)
    K, gs = 10, M // G
    assert (info["K"], info["C"], info["M"], info["G"], info["gs"]) == (K, 120, M, G, gs)
    assert info["bank"].shape == (K + G * gs, geo.proj_dim) and info["bank"].is_cuda
    # the restatement: the same text features, torch.quantile in fp64, the definition in fp64
    cands = words[:120]
    with torch.no_grad():
        ti = tok([PROMPT.format(c=c) for c in ids], padding=True, return_tensors="pt")
        tc = tok([PROMPT.format(c=c) for c in cands], padding=True, return_tensors="pt")
        id_f = net.get_text_features(input_ids=ti["input_ids"], attention_mask=ti["attention_mask"], normalize=True)
        cand_f = net.get_text_features(input_ids=tc["input_ids"], attention_mask=tc["attention_mask"], normalize=True)
        d = torch.quantile(cand_f.double() @ id_f.double().T, q, dim=1).cpu().numpy()
        order = sorted(range(120), key=lambda i: (d[i], i))[:M][:G * gs]
        assert info["words"] == [cands[i] for i in order]
        np.testing.assert_allclose(info["d"], d[order], rtol=0, atol=2 * float(nb.eps_rows(cand_f.cpu().numpy(), id_f.cpu().numpy()).max()))
        bank = torch.cat([id_f, cand_f[order]]).cpu().numpy()
        assert np.array_equal(_bits(info["bank"].cpu().numpy()), _bits(bank))
        for w, ld in sets.items():
            f = torch.cat([net.get_image_features(pixel_values=px).float() for px, _ in ld])
            f = (f / f.norm(dim=-1, keepdim=True)).cpu().numpy()
            _, score, _ = nb.reference(f, bank, K, G, gs, T)
            _, bs_ = nb.budgets(f, bank, K, G, gs, T)
            r = nb.ratio(got[w], score, bs_)
            print(f"BUDGET neglabel {r:.3f} end to end, {w}: {len(score)} scored, K={K} G={G} gs={gs} P={geo.proj_dim} T={T}; scores in "
                  f"[{score.min():.4f}, {score.max():.4f}]")
            assert got[w].shape == score.shape and r <= 1.0, (w, r)
    net.close()


def test_cli_neglabel(tmp_path, monkeypatch):
    import pandas as pd

    import eval_ood_detection as cli
    from mcm_amd.metrics import get_measures

    monkeypatch.chdir(tmp_path)
    (tmp_path / "words.txt").write_text("\n".join(_generated_words(200) + ["", "  "]) + "\n")
    res = cli.main(["--in_dataset", "ImageNet10", "--CLIP_ckpt", "ViT-B/32", "-b", "64", "--score", "neglabel", "--synthetic",
                    "--synthetic-n", "128", "--neg-words", "words.txt", "--neg-count", "60", "--neg-groups", "7", "--name", "n",
                    "--dtype", "fp16"])
    logdir = tmp_path / "results" / "ImageNet10" / "neglabel" / "CLIP_ViT-B/32_T_1_ID_n"
    log = open(logdir / "ood_eval_info.log").read()
    assert "K = 10 ID labels, C = 200 candidate words" in log and "M = 60 kept, G = 7 groups of gs = 8" in log
    assert "--T 1 is ignored" in log and "--neg-T 0.01" in log
    df = pd.read_csv(logdir / "n.csv", index_col=0)
    assert list(df.index) == ["ImageNet20", "AVG"] and np.isfinite(df.values).all()
    ins, outs = res["in_score"], res["out_scores"]["ImageNet20"]
    assert ins.shape == (128,) and outs.shape == (128,) and np.isfinite(ins).all() and np.isfinite(outs).all()
    assert (ins <= 0).all() and (ins >= -1).all()                                       # minus a mean of masses
    auroc, aupr, fpr = get_measures(-ins, -outs)
    assert res["measures"]["ImageNet20"] == (auroc, aupr, fpr)
    np.testing.assert_allclose(df.loc["ImageNet20"].values, np.round([100 * fpr, 100 * auroc, 100 * aupr], 2), atol=1e-9)
