"""The ViM score on a real MI355X: mcm_vim_score_features (vim.hip) against the fp64 reference and the derived budget of
tests/vim_budget.py — the arithmetic term plus one ulp on lattice inputs (every similarity exact in fp32), the full budget on
unit inputs — its off / parts / determinism / NaN / refusal contract, and fit, scoring and the CLI end to end.  Budget cases
print "BUDGET vim <worst ratio> ..." (run with -s to collect them)."""
import ctypes
import types

import numpy as np
import pytest

from tests import gpu_scaffold as gs
from tests import vim_budget as vb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_dev = gs.dev
_bits = gs.bits

WIDTHS = [4, 36, 64, 512, 1024]   # 36: not a multiple of the walk's 32-column chunk
# (B, K, R), N = K + R.  (1,1,1): two rows, with 32 splits thirty of them are empty; (3,300,1): the prompts across the tile edge
# and one basis row behind them, 32 splits of 10 rows: a boundary exactly at K, the last split empty; (64,255,2): the cut at K
# inside the first tile, one row before its edge; (65,256,256): the cut on the tile edge, two splits of 256: the split boundary
# exactly at K; (130,257,3): one prompt past the edge, a ragged third query tile, two splits of 130: the boundary inside the
# prompts; (64,1,300): one prompt, the basis across the edge, two splits of 151: the boundary inside the basis; (65,1000,256):
# ranges of several tiles, three splits of 419: both boundaries inside the prompts, 32 of 40: one exactly at K, six inside the basis
SHAPES = [(1, 1, 1), (3, 300, 1), (64, 255, 2), (65, 256, 256), (130, 257, 3), (64, 1, 300), (65, 1000, 256)]
SPLITS = [1, 2, 3, 32]
ALPHA = 1.75


@pytest.fixture(scope="module")
def vim_nets():
    yield from gs.net_cache()


def _run(net, f, bank, K, off=None, T=0.01, alpha=ALPHA, splits=0):
    o = None if off is None else torch.from_numpy(np.ascontiguousarray(off, dtype=np.float64)).cuda()
    s, p = net.vim_scores(f, bank, K, T=T, alpha=alpha, off=o, splits=splits, return_parts=True)
    p = p.cpu().numpy()
    return {"score": s.cpu().numpy(), "resid": p[:, 0].copy(), "lse": p[:, 1].copy(), "maxlogit": p[:, 2].copy()}


def _same_bits(a, b, rows=slice(None)):
    return gs.same_bits(a, b, rows, vb.OUTPUTS)


@pytest.mark.parametrize("P", WIDTHS)
def test_lattice_inputs_within_the_arithmetic_term(vim_nets, P):
    net = vim_nets(P)
    worst, cases = 0.0, 0
    for B, K, R in SHAPES:
        f, bank = vb.lattice_case(B, K, R, P, seed=B + K + R)
        fd, bd = _dev(f), _dev(bank)
        for off in (None, vb.lattice_off(R, seed=R)):
            for T in (0.01, 1.0):
                ref = vb.reference(f, bank, K, off, T, ALPHA)
                bud = vb.budgets(f, bank, K, off, T, ALPHA, exact=True)
                for splits in SPLITS + [0]:
                    r = vb.worst_ratio(_run(net, fd, bd, K, off, T, ALPHA, splits), ref, bud)
                    worst, cases = max(worst, r), cases + 1
                    assert r <= 1.0, (P, B, K, R, off is not None, T, splits, r)
    print(f"BUDGET vim {worst:.3f} lattice (arithmetic term + one ulp) P={P}: {cases} cases")


@pytest.mark.parametrize("P", [64, 512])
def test_unit_inputs_within_budget(vim_nets, P):
    net = vim_nets(P)
    for B, K, R in SHAPES:
        f, bank = vb.unit_case(B, K, R, P, seed=P + K)
        fd, bd = _dev(f), _dev(bank)
        off = vb.similarities(f[-1:], bank[K:])[0]                                      # the projections of the last query
        for o in (None, off):
            ref = vb.reference(f, bank, K, o, 0.01, ALPHA)
            bud = vb.budgets(f, bank, K, o, 0.01, ALPHA)
            xbud = vb.budgets(f, bank, K, o, 0.01, ALPHA, exact=True)
            per_split, worst = {}, 0.0
            for splits in SPLITS:
                got = per_split[splits] = _run(net, fd, bd, K, o, 0.01, ALPHA, splits)
                r = vb.worst_ratio(got, ref, bud)
                worst = max(worst, r)
                assert r <= 1.0, (P, B, K, R, o is not None, splits, r)
                if o is None and R <= 4 and B >= 2:
                    assert (got["resid"][:2] == 0.0).all()                              # the rows exactly in the principal space
            print(f"BUDGET vim {worst:.3f} unit P={P} B={B} K={K} R={R} off={'given' if o is not None else 'NULL'} T=0.01 "
                  f"splits={SPLITS}; resid in [{ref['resid'].min():.3e}, {ref['resid'].max():.4f}]")
            # across splits the similarities are the same bits and only the sums are associated differently: two results differ
            # by at most twice the arithmetic term plus one ulp
            for a in SPLITS[1:]:
                for k in vb.OUTPUTS:
                    assert (np.abs(per_split[a][k].astype(np.float64) - per_split[1][k]) <= 2 * xbud[k]).all(), (P, B, K, R, a, k)


def test_off_of_a_querys_own_projections_gives_resid_zero(vim_nets):
    """Lattice inputs: the similarities are exact in fp32, so off = the fp64 projections of query 5 are the values the kernel
    subtracts them from, bit for bit: its resid is exactly 0 and its score the rounded -lse."""
    net = vim_nets(64)
    B, K, R = 65, 256, 256
    f, bank = vb.lattice_case(B, K, R, 64, seed=11)
    off = vb.similarities(f[5:6], bank[K:])[0]
    for splits in SPLITS:
        got = _run(net, _dev(f), _dev(bank), K, off, 0.01, ALPHA, splits)
        none = _run(net, _dev(f), _dev(bank), K, None, 0.01, ALPHA, splits)
        assert got["resid"][5] == 0.0 and none["resid"][5] > 0.0
        assert np.array_equal(_bits(got["score"][5:6]), _bits(-got["lse"][5:6]))
        assert np.array_equal(_bits(got["lse"]), _bits(none["lse"])) and np.array_equal(_bits(got["maxlogit"]), _bits(none["maxlogit"]))
        assert (np.delete(got["resid"], 5) > 0.0).all()


def test_parts_are_consistent_with_the_scores(vim_nets):
    net = vim_nets(512)
    B, K, R = 65, 1000, 256
    f, bank = vb.unit_case(B, K, R, 512, seed=9)
    fd, bd = _dev(f), _dev(bank)
    for alpha in (ALPHA, -3.0, 1e-3):
        got = _run(net, fd, bd, K, None, 0.01, alpha, 3)
        a = vb.a_double(alpha)
        want = a * got["resid"].astype(np.float64) - got["lse"].astype(np.float64)
        # the score is formed from the fp64 parts: each stored part is within half an fp32 ulp of its own, the score of its
        room = (abs(a) * 0.5 * np.spacing(got["resid"]).astype(np.float64) + 0.5 * np.spacing(np.abs(got["lse"])).astype(np.float64)
                + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
        assert (np.abs(got["score"].astype(np.float64) - want) <= room).all(), alpha
    zero = _run(net, fd, bd, K, None, 0.01, 0.0, 3)
    assert np.array_equal(_bits(zero["score"]), _bits(-zero["lse"]))
    assert (zero["maxlogit"] <= zero["lse"]).all() and (zero["resid"] > 0).all()
    only = net.vim_scores(fd, bd, K, T=0.01, alpha=0.0, splits=3)                        # parts_dev is optional
    assert np.array_equal(_bits(only.cpu().numpy()), _bits(zero["score"]))


def test_same_bits_over_runs_query_cuts_and_row_positions(vim_nets):
    net = vim_nets(512)
    B, K, R = 130, 257, 259
    f, bank = vb.unit_case(B, K, R, 512, seed=5)
    off = vb.similarities(f[-1:], bank[K:])[0]
    fd, bd = _dev(f), _dev(bank)
    for splits in SPLITS:
        first = _run(net, fd, bd, K, off, 0.01, ALPHA, splits)
        assert _same_bits(_run(net, fd, bd, K, off, 0.01, ALPHA, splits), first), splits
        parts = [_run(net, fd[a:a + n], bd, K, off, 0.01, ALPHA, splits) for a, n in ((0, 1), (1, 64), (65, 65))]
        joined = {k: np.concatenate([p[k] for p in parts]) for k in vb.OUTPUTS}
        assert _same_bits(joined, first), splits
        perm = np.random.default_rng(splits).permutation(B)
        moved = _run(net, _dev(f[perm]), bd, K, off, 0.01, ALPHA, splits)
        assert _same_bits(moved, {k: first[k][perm] for k in vb.OUTPUTS}), splits


def test_a_nan_stays_in_its_row_and_a_nan_basis_row_reaches_every_score(vim_nets):
    net = vim_nets(64)
    B, K, R = 5, 300, 40
    f, bank = vb.unit_case(B, K, R, 64, seed=3)
    fq = f.copy()
    fq[2, 7] = np.nan
    keep = [0, 1, 3, 4]
    for splits in (1, 3):
        clean = _run(net, _dev(f), _dev(bank), K, None, 0.01, ALPHA, splits)
        got = _run(net, _dev(fq), _dev(bank), K, None, 0.01, ALPHA, splits)
        assert np.isnan(got["score"][2]) and np.isnan(got["resid"][2]) and np.isnan(got["lse"][2])
        assert _same_bits(got, clean, keep)
        bn = bank.copy()
        bn[K + 17, 3] = np.nan                                                          # one NaN basis row
        got = _run(net, _dev(f), _dev(bn), K, None, 0.01, ALPHA, splits)
        assert np.isnan(got["score"]).all() and np.isnan(got["resid"]).all()
        assert np.array_equal(_bits(got["lse"]), _bits(clean["lse"]))                   # the prompts did not see it
        bn = bank.copy()
        bn[K - 1, 3] = np.nan                                                           # one NaN prompt row
        got = _run(net, _dev(f), _dev(bn), K, None, 0.01, ALPHA, splits)
        assert np.isnan(got["score"]).all() and np.isnan(got["lse"]).all()
        assert np.array_equal(_bits(got["resid"]), _bits(clean["resid"]))


def test_refused_calls_launch_nothing(vim_nets):
    """Every refusal of the header but proj_dim % 4 != 0, which mcm_create refuses before a handle exists."""
    from mcm_amd.engine import _stream_ptr

    net, P = vim_nets(64), 64
    B, K, R = 5, 300, 40
    f, bank = vb.unit_case(B, K, R, P, seed=3)
    fd, bd = _dev(f), _dev(bank)
    od = torch.zeros(R + 1, dtype=torch.float64, device="cuda")
    work = torch.full((32 * B * 4,), 7.5, device="cuda")
    out = torch.full((B,), -2.5, device="cuda")
    parts = torch.full((B, 3), -3.5, device="cuda")
    call, sp = net._lib.mcm_vim_score_features, _stream_ptr
    wb = work.numel() * 4

    def go(h=net._h, fp=fd.data_ptr(), B=B, bp=bd.data_ptr(), K=K, R=R, offp=None, T=0.01, alpha=ALPHA, splits=2,
           wp=work.data_ptr(), nbytes=wb, op=out.data_ptr(), pp=parts.data_ptr()):
        return call(h, fp, B, bp, K, R, offp, T, alpha, splits, wp, nbytes, op, pp, sp())

    assert go(h=None) == -1
    assert go(fp=None) == -1 and go(bp=None) == -1 and go(wp=None) == -1 and go(op=None) == -1
    assert go(B=0) == -1 and go(B=-1) == -1 and go(K=0) == -1 and go(K=-3) == -1 and go(R=0) == -1 and go(R=-1) == -1
    assert go(K=2 ** 31 - 1, R=1) == -1 and go(K=2 ** 31 - 40, R=R) == -1               # K + R = 2^31
    assert go(T=0.0) == -1 and go(T=-0.01) == -1 and go(T=float("inf")) == -1 and go(T=float("nan")) == -1
    assert go(alpha=float("inf")) == -1 and go(alpha=float("-inf")) == -1 and go(alpha=float("nan")) == -1
    assert go(splits=-1) == -1 and go(splits=33) == -1
    assert go(nbytes=2 * B * 16 - 1) == -1
    assert go(fp=fd.data_ptr() + 4) == -1 and go(bp=bd.data_ptr() + 8) == -1            # rows are read 16 bytes at a time
    assert go(offp=od.data_ptr() + 4) == -1                                             # off is read as doubles
    need = ctypes.c_int64(-1)
    wbytes = net._lib.mcm_vim_workspace_bytes
    assert wbytes(net._h, B, K, R, 33, ctypes.byref(need)) == -1 and wbytes(net._h, B, K, 0, 1, ctypes.byref(need)) == -1
    assert wbytes(net._h, 0, K, R, 1, ctypes.byref(need)) == -1 and wbytes(net._h, B, 0, R, 1, ctypes.byref(need)) == -1
    assert wbytes(None, B, K, R, 1, ctypes.byref(need)) == -1 and wbytes(net._h, B, K, R, 1, None) == -1
    assert wbytes(net._h, B, 2 ** 31 - 1, 1, 1, ctypes.byref(need)) == -1
    assert need.value == -1
    assert wbytes(net._h, B, K, R, 2, ctypes.byref(need)) == 0 and need.value == 2 * B * 16
    assert wbytes(net._h, B, K, R, 0, ctypes.byref(need)) == 0 and need.value % (B * 16) == 0
    assert 1 <= need.value // (B * 16) <= 32
    torch.cuda.synchronize()
    assert (work == 7.5).all() and (out == -2.5).all() and (parts == -3.5).all()
    with pytest.raises(ValueError, match="n_id"):
        net.vim_scores(fd, bd, K + R)                                                   # no basis row is left
    with pytest.raises(ValueError, match="T="):
        net.vim_scores(fd, bd, K, T=0.0)
    with pytest.raises(ValueError, match="alpha="):
        net.vim_scores(fd, bd, K, alpha=float("nan"))
    with pytest.raises(ValueError, match="splits="):
        net.vim_scores(fd, bd, K, splits=33)
    with pytest.raises(ValueError, match="off"):
        net.vim_scores(fd, bd, K, off=od)                                               # R + 1 values
    with pytest.raises(ValueError):
        net.vim_scores(fd[:, :60], bd, K)
    assert go(pp=None) == 0                                                             # parts_dev is optional
    torch.cuda.synchronize()
    assert (out != -2.5).all() and (parts == -3.5).all()
    first = out.clone()
    assert go(offp=od.data_ptr()) == 0                                                  # off = 0 is NULL; the same buffers take a good call
    torch.cuda.synchronize()
    assert torch.equal(out, first) and (parts != -3.5).all()
    # no word of the workspace is read before it is written: a NaN-filled one gives the same bits (32 splits of 11 rows: the
    # last is empty)
    for fill in (float("nan"), 3.0e38):
        work.fill_(fill)
        assert go(splits=32) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and torch.isfinite(parts).all()
        want = _run(net, fd, bd, K, None, 0.01, ALPHA, 32)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want["score"]))
        assert np.array_equal(_bits(parts.cpu().numpy()[:, 0]), _bits(want["resid"]))


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_end_to_end_fit_and_scores_against_numpy():
    """get_vim_fit and get_vim_score through detection.py on the tiny geometry's fp32 arm (proj_dim 64, D = 32) against a numpy
    fp64 recomputation from the same fp32 features and fit["bank"].  The fit is checked without leaning on an eigen-gap: NS
    orthonormal, and the spectrum of NS (G / n) NS^T equal to the R smallest eigenvalues of G / n."""
    import warnings

    from mcm_amd.config import TEST_GEOMETRIES
    from mcm_amd.detection import get_vim_fit, get_vim_score
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.synth import make_pixels
    from mcm_amd.weights import synth_state_dict

    bs, T = 64, 0.01
    ids = [f"class{i}" for i in range(10)]
    args = types.SimpleNamespace(model="CLIP", normalize=False, batch_size=bs, ckpt="", weights=None, vim_dim=0, vim_T=T)
    geo = TEST_GEOMETRIES["tiny"]
    net = NativeCLIP(geo, synth_state_dict(geo, seed=0), precision="fp32", max_batch=64, max_prompt_tokens=64 * 16)

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

    def features(ld):
        with torch.no_grad():
            f = torch.cat([net.get_image_features(pixel_values=px).float() for px, _ in ld])
        return (f / f.norm(dim=-1, keepdim=True)).cpu().numpy()

    train, sets = Loader(150, False, 7), {"id": Loader(70, False, 1), "ood": Loader(64, True, 2)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                                 # the hash tokenizer's stand-in ids
        fit = get_vim_fit(args, net, train, ids)
        got = {w: get_vim_score(args, net, ld, fit) for w, ld in sets.items()}
    P, K, D, R = geo.proj_dim, 10, 32, 32
    assert (fit["K"], fit["D"], fit["R"], fit["n"], fit["T"]) == (K, D, R, 150, T)
    assert fit["bank"].shape == (K + R, P) and fit["bank"].is_cuda and fit["bank"].dtype == torch.float32
    bank = fit["bank"].cpu().numpy()
    ns = bank[K:].astype(np.float64)
    assert np.abs(ns @ ns.T - np.eye(R)).max() <= 1e-6
    x = features(train).astype(np.float64)
    M = x.T @ x / 150.0
    lam = np.linalg.eigvalsh(M)
    assert np.abs(np.linalg.eigvalsh(ns @ M @ ns.T) - lam[:R]).max() <= 1e-10 * lam[-1]
    assert np.abs(fit["eigenvalues"] - lam).max() <= 1e-10 * lam[-1]
    tr = vb.reference(x.astype(np.float32), bank, K, None, T, 0.0)
    alpha = tr["maxlogit"].sum() / tr["resid"].sum()
    assert abs(fit["alpha"] - alpha) <= 1e-6 * abs(alpha), (fit["alpha"], alpha)
    for w, ld in sets.items():
        f = features(ld)
        ref = vb.reference(f, bank, K, None, T, fit["alpha"])
        bud = vb.budgets(f, bank, K, None, T, fit["alpha"])
        r = vb.ratio(got[w], ref["score"], bud["score"])
        print(f"BUDGET vim {r:.3f} end to end, {w}: {len(f)} scored, K={K} D={D} R={R} P={P} T={T} alpha={fit['alpha']:.4f}; scores in "
              f"[{ref['score'].min():.4f}, {ref['score'].max():.4f}]")
        assert got[w].dtype == np.float32 and got[w].shape == ref["score"].shape and r <= 1.0, (w, r)
    net.close()


def test_cli_vim(tmp_path, monkeypatch):
    import re

    import pandas as pd

    import eval_ood_detection as cli
    from mcm_amd.metrics import get_measures

    monkeypatch.chdir(tmp_path)
    res = cli.main(["--in_dataset", "ImageNet10", "--CLIP_ckpt", "ViT-B/32", "-b", "64", "--score", "vim", "--synthetic",
                    "--synthetic-n", "128", "--vim-dim", "32", "--name", "v", "--dtype", "fp16"])
    logdir = tmp_path / "results" / "ImageNet10" / "vim" / "CLIP_ViT-B/32_T_1_ID_v"
    log = open(logdir / "ood_eval_info.log").read()
    assert "--T 1 is ignored" in log and "--vim-T 0.01" in log
    m = re.search(r"--score vim: D = 32, R = 480, n = 128 unit-norm training features \(synthetic\), alpha = (\S+), lambda_D = (\S+), "
                  r"lambda_\(D\+1\) = (\S+), lambda_max = (\S+)", log)
    assert m, log
    alpha, lam_d, lam_d1, lam_max = (float(g.rstrip(",")) for g in m.groups())
    assert np.isfinite(alpha) and alpha != 0.0 and lam_max >= lam_d > lam_d1 >= -1e-12
    df = pd.read_csv(logdir / "v.csv", index_col=0)
    assert list(df.index) == ["ImageNet20", "AVG"] and np.isfinite(df.values).all()
    ins, outs = res["in_score"], res["out_scores"]["ImageNet20"]
    assert ins.shape == (128,) and outs.shape == (128,) and np.isfinite(ins).all() and np.isfinite(outs).all()
    auroc, aupr, fpr = get_measures(-ins, -outs)
    assert res["measures"]["ImageNet20"] == (auroc, aupr, fpr)
    np.testing.assert_allclose(df.loc["ImageNet20"].values, np.round([100 * fpr, 100 * auroc, 100 * aupr], 2), atol=1e-9)
