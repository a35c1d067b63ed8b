"""`get_mean_prec_device` on the CPU, through a stub net whose `maha_fit_accumulate` is torch fp64: against the host route
`get_mean_prec` in one process, and under gloo at world sizes 2 and 3 with empty and ragged shards; the CLI switch."""
import os
import socket
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

from tests import maha_fit_budget as fb  # noqa: E402

N_CLS, BS = 3, 8


class _FitSet(torch.utils.data.Dataset):
    """Map-style set: image i is a function of i alone; labels cycle through 0 .. 4, so two of five are >= n_cls = 3
    (`big`: what those two are replaced by)."""

    def __init__(self, n, big=None):
        self.n, self.big = n, big

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(500 + int(i))
        lab = int(i) % 5
        return torch.randn(3, 8, 8, generator=g) * 0.7 + 5.0, (self.big if (lab >= N_CLS and self.big is not None) else lab)


class _StubFitNet:
    """Features = the first P pixel values, column c scaled by 1 + c / 4; the fit's running sums in torch fp64."""

    def __init__(self, P):
        self.P = P

    def get_image_features(self, pixel_values):
        f = pixel_values.reshape(pixel_values.shape[0], -1)[:, :self.P].float()
        return f * (1.0 + torch.arange(self.P, dtype=torch.float32) / 4)

    def maha_fit_state(self, shift=None):
        sh = torch.zeros(self.P) if shift is None else shift.float().clone()
        return {"gram": torch.zeros(self.P, self.P, dtype=torch.float64), "sum": torch.zeros(self.P, dtype=torch.float64),
                "shift": sh, "n": 0}

    def maha_fit_accumulate(self, features, state):
        x = features.double() - state["shift"].double()
        for row in x:                                   # row after row, as the kernel does
            state["gram"] += torch.outer(row, row)
            state["sum"] += row
        state["n"] += int(x.shape[0])
        return state


def _args(P, tdir, normalize=False):
    return types.SimpleNamespace(n_cls=N_CLS, feat_dim=P, model="CLIP", normalize=normalize, template_dir=str(tdir),
                                 in_dataset="ImageNet10", max_count=250, batch_size=BS)


def _loader(n, big=None):
    return torch.utils.data.DataLoader(_FitSet(n, big), batch_size=BS, shuffle=False)


def _width(n):
    return 2 if n < 8 else 6   # (three samples span two dimensions: a wider covariance would be singular)


def _all_features(net, n, normalize=False):
    f = torch.cat([net.get_image_features(x) for x, _ in _loader(n)])
    return (f / f.norm(dim=-1, keepdim=True)) if normalize else f


def _bits(t):
    return np.ascontiguousarray(t.numpy()).view(np.int32)


def _files(tdir):
    return sorted(os.listdir(tdir)) if os.path.isdir(tdir) else []


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n", [3, 70])
def test_single_process_equals_host_route(n, normalize, tmp_path):
    from mcm_amd.detection import get_mean_prec, get_mean_prec_device

    P = _width(n)
    net = _StubFitNet(P)
    mean_h, prec_h = get_mean_prec(_args(P, tmp_path / "host", normalize), net, _loader(n))
    mean_d, prec_d, cov = get_mean_prec_device(_args(P, tmp_path / "dev", normalize), net, _loader(n), return_cov=True)
    assert np.array_equal(_bits(mean_d), _bits(mean_h))                       # bit for bit, NaN rows (empty classes) included
    assert cov.dtype == torch.float64 and prec_d.dtype == torch.float32
    F = _all_features(net, n, normalize).numpy()
    r, i = fb.cov_ratio(cov.numpy(), F, F[:BS].mean(axis=0, dtype=np.float32))
    print(f"BUDGET maha-fit stub {r:.3f} n={n} normalize={normalize}")
    assert r <= 1.0, (r, i)
    assert _files(tmp_path / "dev") == _files(tmp_path / "host") and len(_files(tmp_path / "dev")) == 2
    assert torch.equal(torch.load(tmp_path / "dev" / f"CLIP_precision_ImageNet10_250_{normalize}.pt"), prec_d)
    assert torch.equal(torch.load(tmp_path / "dev" / f"CLIP_classwise_mean_ImageNet10_250_{normalize}.pt").isnan(),
                       mean_d.isnan())
    if n == 70:   # a well-conditioned case: the two routes' precisions agree to fp32 round-off of the inverse
        np.testing.assert_allclose(prec_d.numpy(), prec_h.numpy(), rtol=1e-5, atol=1e-6 * float(prec_h.abs().max()))
    assert get_mean_prec_device(_args(P, "", normalize), net, _loader(n))[1].shape == (P, P)   # two values without return_cov


def test_labels_beyond_n_cls_are_ignored(tmp_path):
    from mcm_amd.detection import get_mean_prec_device

    net = _StubFitNet(6)
    a = get_mean_prec_device(_args(6, tmp_path), net, _loader(70))
    b = get_mean_prec_device(_args(6, tmp_path), net, _loader(70, big=99))
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])
    assert torch.isfinite(a[0]).all()


def test_a_net_without_the_fit_is_refused(tmp_path):
    from mcm_amd.detection import get_mean_prec_device

    net = types.SimpleNamespace(get_image_features=lambda pixel_values: pixel_values)
    with pytest.raises(TypeError, match="maha_fit"):
        get_mean_prec_device(_args(6, tmp_path), net, _loader(9))


def test_unshardable_loader_is_refused(tmp_path, monkeypatch):
    """world_size 2 and an opaque iterable: the TypeError of get_Mahalanobis_score, raised before anything is computed."""
    from mcm_amd import dist as mdist
    from mcm_amd.detection import get_mean_prec_device

    base = _loader(20)

    class Plain:
        dataset = base.dataset

        def __iter__(self):
            raise AssertionError("nothing may be iterated")

    monkeypatch.setattr(mdist, "world", lambda: (1, 2))
    with pytest.raises(TypeError, match="sharded by index"):
        get_mean_prec_device(_args(6, tmp_path), _StubFitNet(6), Plain())


# ---- gloo ---------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, ws, port, n, tdir, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from mcm_amd.detection import get_mean_prec_device

    dist.init_process_group("gloo", rank=rank, world_size=ws)
    P = _width(n)
    mine = os.path.join(tdir, f"rank{rank}")
    mean, prec, cov = get_mean_prec_device(_args(P, mine), _StubFitNet(P), _loader(n), return_cov=True)
    q.put((rank, mean.numpy(), prec.numpy(), cov.numpy(), _files(mine)))
    dist.destroy_process_group()


@pytest.mark.parametrize("ws,n", [(2, 3), (3, 3), (2, 70), (3, 70)])
def test_gloo_shards_equal_single_process(ws, n, tmp_path):
    """n = 3 on three ranks of batch 8: shards of one sample, on two ranks 2 + 1; n = 70: 35 + 35 and 24 + 24 + 22, the
    last batch of every shard ragged, the rows of the class-mean rule (the first 1 or 9 samples) all in rank 0's shard."""
    from mcm_amd.detection import get_mean_prec_device
    from mcm_amd.dist import shard_range

    P = _width(n)
    net = _StubFitNet(P)
    mean1, prec1, cov1 = get_mean_prec_device(_args(P, tmp_path / "one"), net, _loader(n), return_cov=True)
    F = _all_features(net, n).numpy()
    shift = F[:min(BS, shard_range(n, 0, ws)[1])].mean(axis=0, dtype=np.float32)   # rank 0's first batch
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, ws, port, n, str(tmp_path), q)) for r in range(ws)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, mean, prec, cov, files in got:
        assert np.array_equal(mean.view(np.int32), _bits(mean1)), rank
        r, i = fb.cov_ratio(cov, F, shift)
        print(f"BUDGET maha-fit gloo {r:.3f} ws={ws} n={n} rank={rank}")
        assert r <= 1.0, (rank, r, i)
        assert np.array_equal(cov, got[0][3]) and np.array_equal(prec, got[0][2])   # every rank returns the same statistics
        assert len(files) == (2 if rank == 0 else 0), (rank, files)


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_switch(tmp_path, monkeypatch):
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    assert cli.process_args(["--in_dataset", "ImageNet10"]).maha_fit == "host"
    assert cli.process_args(["--in_dataset", "ImageNet10", "--score", "maha", "--maha-fit", "device"]).maha_fit == "device"
    with pytest.raises(SystemExit):
        cli.process_args(["--in_dataset", "ImageNet10", "--maha-fit", "device"])
    with pytest.raises(SystemExit):
        cli.process_args(["--in_dataset", "ImageNet10", "--score", "maha", "--maha-fit", "elsewhere"])
