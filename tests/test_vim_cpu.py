"""The host side of `--score vim` on the CPU: the CLI's switches and refusals, the dimension rule, `vim_null_space` against numpy
on a planted spectrum and its gap refusal, and `get_vim_fit` / `get_vim_score` through a stand-in net (features a function of the
pixels / token ids, the Mahalanobis running sums and `vim_scores` the definitions in fp64) in one process and under gloo at world
sizes 2 and 3, ragged and empty shards included."""
import os
import socket
import types
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

P, BS = 8, 8
SUPPORTS = [(0, 1, 4, 5), (2, 3, 6, 7), (4, 5, 6, 7), (0, 2, 4, 6)]


class _Set(torch.utils.data.Dataset):
    """Images whose first P values hold four entries +-1 and four zeros: the unit-norm feature has entries +-0.5 and 0, so the
    Gram matrix is a sum of multiples of 0.25 — exact in fp64 however the rows are cut into shards and batches.  Three rows of
    four live on columns 0 .. 3 (the principal space at D = 4), the fourth on one of SUPPORTS."""

    def __init__(self, n, seed):
        self.n, self.seed = n, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed + int(i))
        x = torch.zeros(3 * 4 * 4)
        sup = (0, 1, 2, 3) if int(i) % 4 != 3 else SUPPORTS[(int(i) // 4) % len(SUPPORTS)]
        sign = torch.randint(0, 2, (4,), generator=g).float() * 2.0 - 1.0
        x[list(sup)] = sign
        return x.reshape(3, 4, 4), int(i) % 3


def _cols(t):
    """sum over the last axis, column after column: the same bits for a row whatever batch it comes in."""
    acc = t[..., 0].clone()
    for j in range(1, t.shape[-1]):
        acc = acc + t[..., j]
    return acc


class _StubNet:
    """Text features = a function of the unpadded token ids (not unit: the routines must normalise); image features = the first
    P pixel values; maha_fit_* = the running sums in fp64, row after row; vim_scores = the definition in fp64, every sum taken
    column after column, returned as fp32 like the device's."""

    def get_text_features(self, input_ids, attention_mask=None):
        ids = input_ids.double() * attention_mask.double()
        freq = torch.arange(1, P + 1, dtype=torch.float64) * 0.37
        return (torch.sin(ids[:, :, None] * freq[None, None, :] * 1e-3).sum(dim=1) + 0.05).float()

    def get_image_features(self, pixel_values):
        return pixel_values.reshape(pixel_values.shape[0], -1)[:, :P].float()

    def maha_fit_state(self, shift=None):
        assert shift is None                                       # ViM's origin is 0
        return {"gram": torch.zeros(P, P, dtype=torch.float64), "sum": torch.zeros(P, dtype=torch.float64),
                "shift": torch.zeros(P), "n": 0}

    def maha_fit_accumulate(self, features, state):
        for row in features.double():
            state["gram"] += torch.outer(row, row)
            state["sum"] += row
        state["n"] += int(features.shape[0])
        return state

    def vim_scores(self, features, bank, n_id, T=0.01, alpha=1.0, off=None, splits=0, return_parts=False):
        s = _cols(features.double()[:, None, :] * bank.double()[None, :, :])
        logit = s[:, :n_id] / float(np.float32(T))
        m = logit.max(dim=1).values
        lse = m + torch.log(_cols(torch.exp(logit - m[:, None])))
        v = s[:, n_id:] - (0.0 if off is None else off.double()[None, :])
        resid = torch.sqrt(_cols(v * v))
        score = (float(np.float32(alpha)) * resid - lse).float()
        return (score, torch.stack([resid, lse, m], dim=1).float()) if return_parts else score


IDS = [f"id{i:03d}x" for i in range(6)]


def _args(**kw):
    base = dict(model="CLIP", normalize=False, feat_dim=P, batch_size=BS, ckpt="", weights=None, vim_dim=0, vim_T=0.01)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _loader(n, seed):
    return torch.utils.data.DataLoader(_Set(n, seed), batch_size=BS, shuffle=False)


# (training rows, --vim-dim): 21 rows: 11 + 10 and 7 + 7 + 7 with batches of 8 (ragged everywhere); 4 rows at D = 2: 2 + 2 and
# 2 + 2 + 0, an empty shard in the fit
FITS = [(21, 0), (4, 2)]
TESTS = [3, 21]                                                    # 3 samples: 2 + 1 and 1 + 1 + 1; on the 4-row fit's ranks too


def _fit_and_score():
    from mcm_amd.detection import get_vim_fit, get_vim_score

    out = []
    for n_train, D in FITS:
        a, net = _args(vim_dim=D), _StubNet()
        fit = get_vim_fit(a, net, _loader(n_train, 100), IDS)
        out.append((fit, [get_vim_score(a, net, _loader(n, 900), fit) for n in TESTS]))
    return out


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)            # the hash tokenizer says that its ids are stand-ins
        yield


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_switches_and_refusals(tmp_path, monkeypatch):
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    base = ["--in_dataset", "ImageNet10", "--score", "vim"]
    a = cli.process_args(base)
    assert a.score == "vim" and (a.vim_dim, a.vim_T) == (0, 0.01)
    assert a.refine_threshold == "off"                             # auto resolves to off
    assert cli.process_args(base + ["--refine-threshold", "off"]).refine_threshold == "off"
    a = cli.process_args(base + ["--vim-dim", "300", "--vim-T", "0.05", "--T", "3"])
    assert (a.vim_dim, a.vim_T, a.T) == (300, 0.05, 3)
    a = cli.process_args(["--in_dataset", "ImageNet10"])           # the flags exist for every score, and change nothing there
    assert (a.vim_dim, a.vim_T, a.refine_threshold) == (0, 0.01, "auto")
    for bad in (["--predict"], ["--refine-threshold", "on"], ["--refine-threshold", "exact"], ["--vim-T", "0"], ["--vim-T", "-1"],
                ["--vim-T", "inf"], ["--vim-T", "nan"], ["--vim-dim", "-1"]):
        with pytest.raises(SystemExit):
            cli.process_args(base + bad)


# ---- the dimension rule and the null space --------------------------------------------------------------------------------
def test_principal_dim_rule():
    from mcm_amd.detection import vim_principal_dim

    assert [vim_principal_dim(p) for p in (64, 512, 768, 1024, 2048)] == [32, 256, 512, 512, 1000]
    assert vim_principal_dim(767) == 383 and vim_principal_dim(2047) == 512 and vim_principal_dim(4) == 2
    assert vim_principal_dim(512, 0) == 256 and vim_principal_dim(512, 1) == 1 and vim_principal_dim(512, 511) == 511
    for p, d in ((512, 512), (512, 600), (512, -1), (1, 0), (768, 768)):
        with pytest.raises(ValueError, match="--vim-dim D: D must be 0 or 1..proj_dim - 1"):
            vim_principal_dim(p, d)


@pytest.mark.parametrize("Pw,D", [(16, 8), (16, 1), (16, 15), (64, 32)])
def test_null_space_equals_numpys_on_a_planted_spectrum(Pw, D):
    from mcm_amd.detection import vim_null_space

    rng = np.random.default_rng(Pw + D)
    q, _ = np.linalg.qr(rng.standard_normal((Pw, Pw)))
    lam = np.concatenate([np.linspace(1.0, 0.5, D), np.linspace(0.1, 0.01, Pw - D)])       # descending; 0.5 / 0.1 across the cut
    assert lam[D - 1] / lam[D] >= 4.0
    n = 1000
    gram = n * (q * lam[None, :]) @ q.T
    gram = (gram + gram.T) / 2.0
    ns, spec = vim_null_space(torch.from_numpy(gram), n, D)
    assert ns.dtype == torch.float32 and ns.shape == (Pw - D, Pw) and spec.dtype == torch.float64 and spec.shape == (Pw,)
    np.testing.assert_allclose(spec.numpy()[::-1], lam, rtol=0, atol=1e-12)
    w, v = np.linalg.eigh(gram / n)
    want = v[:, :Pw - D] @ v[:, :Pw - D].T
    got = ns.double().numpy().T @ ns.double().numpy()
    assert np.abs(got - want).max() <= 1e-6
    assert np.abs(ns.double().numpy() @ ns.double().numpy().T - np.eye(Pw - D)).max() <= 1e-6
    ns2, _ = vim_null_space(gram, n, D)                            # an ndarray is taken too, and gives the same bits
    assert torch.equal(ns, ns2)


def test_null_space_refuses_an_undetermined_subspace():
    from mcm_amd.detection import vim_null_space

    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 8))                                # n = 3 < D = 4 rows: lambda_4 = lambda_5 = 0 up to rounding
    with pytest.raises(ValueError, match="not determined"):
        vim_null_space(x.T @ x, 3, 4)
    vim_null_space(x.T @ x, 3, 2)                                  # ... D = 2 of rank 3 is determined
    with pytest.raises(ValueError, match="not determined"):        # a flat spectrum
        vim_null_space(100.0 * np.eye(8), 100, 4)
    for gram, n, D in ((np.eye(8), 0, 4), (np.eye(8), 10, 0), (np.eye(8), 10, 8), (np.ones((8, 7)), 10, 4)):
        with pytest.raises(ValueError):
            vim_null_space(gram, n, D)


# ---- fit and scores ---------------------------------------------------------------------------------------------------------
def test_single_process_equals_the_direct_computation():
    from mcm_amd.detection import get_vim_fit, get_vim_score, prompt_bank

    a, net = _args(), _StubNet()
    fit = get_vim_fit(a, net, _loader(21, 100), IDS)
    assert (fit["K"], fit["D"], fit["R"], fit["n"], fit["T"]) == (6, 4, 4, 21, 0.01)
    x = torch.stack([_Set(21, 100)[i][0].reshape(-1)[:P] for i in range(21)]).double() / 2.0   # the unit rows: entries +-0.5
    M = (x.T @ x / 21.0).numpy()
    lam, vec = np.linalg.eigh(M)
    np.testing.assert_allclose(fit["eigenvalues"], lam, rtol=0, atol=1e-14)
    assert lam[4] - lam[3] > 1e-3                                  # a gap at D = 4: both eigensolvers see one subspace
    bank = fit["bank"]
    assert bank.dtype == torch.float32 and bank.shape == (6 + 4, P)
    assert torch.equal(bank[:6], prompt_bank(a, net, IDS).float())
    ns = bank[6:].double().numpy()
    assert np.abs(ns.T @ ns - vec[:, :4] @ vec[:, :4].T).max() <= 1e-6
    _, parts = net.vim_scores(x.float(), bank, 6, T=0.01, alpha=0.0, return_parts=True)
    alpha = float(parts[:, 2].double().sum()) / float(parts[:, 0].double().sum())
    assert abs(fit["alpha"] - alpha) <= 1e-12 * abs(alpha)
    got = get_vim_score(a, net, _loader(21, 900), fit)
    f = torch.stack([_Set(21, 900)[i][0].reshape(-1)[:P] for i in range(21)]) / 2.0
    want = net.vim_scores(f, bank, 6, T=0.01, alpha=fit["alpha"]).numpy()
    assert got.dtype == np.float32 and got.shape == (21,) and np.array_equal(_bits(got), _bits(want))
    assert len(set(np.round(got, 3))) > 5                          # the residual term differs between rows


def test_refusals():
    from mcm_amd.detection import get_vim_fit, get_vim_score

    with pytest.raises(TypeError, match="vim_scores"):
        get_vim_fit(_args(), types.SimpleNamespace(), _loader(21, 100), IDS)
    with pytest.raises(TypeError, match="vim_scores"):
        get_vim_score(_args(), types.SimpleNamespace(), _loader(3, 900), {"bank": torch.zeros(2, P), "K": 1, "T": 0.01, "alpha": 1.0})
    with pytest.raises(ValueError, match="not determined"):        # 3 training rows, D = 4
        get_vim_fit(_args(), _StubNet(), _loader(3, 100), IDS)
    with pytest.raises(ValueError, match="--vim-dim"):
        get_vim_fit(_args(vim_dim=8), _StubNet(), _loader(21, 100), IDS)

    class NoResidual(_StubNet):                                    # every training row inside the principal space
        def vim_scores(self, *args, **kw):
            score, parts = super().vim_scores(*args, **kw)
            parts[:, 0] = 0.0
            return score, parts

    with pytest.raises(ValueError, match="alpha"):
        get_vim_fit(_args(), NoResidual(), _loader(21, 100), IDS)


# ---- gloo ---------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, ws, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank))
    warnings.simplefilter("ignore", RuntimeWarning)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=ws)
    res = [(fit["bank"].numpy(), fit["alpha"], fit["n"], fit["D"], fit["R"], fit["eigenvalues"], scores) for fit, scores in _fit_and_score()]
    q.put((rank, res))
    dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 3])
def test_gloo_shards_equal_single_process(ws):
    """The Gram matrix is exact in fp64 (see _Set), so every rank computes the basis from the same bits as the single-process
    run: the bank is equal bit for bit, alpha to the rounding of the two all-reduced fp64 sums, the scores bit for bit."""
    want = _fit_and_score()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, ws, port, q)) for r in range(ws)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, res in got:
        for (fit, scores), (bank, alpha, n, D, R, lam, sc) in zip(want, res):
            assert (n, D, R) == (fit["n"], fit["D"], fit["R"]), rank
            assert np.array_equal(lam, fit["eigenvalues"]), rank
            assert np.array_equal(_bits(bank), _bits(fit["bank"].numpy())), rank
            assert abs(alpha - fit["alpha"]) <= 1e-12 * abs(fit["alpha"]), (rank, alpha, fit["alpha"])
            for a, b in zip(sc, scores):
                assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), rank
