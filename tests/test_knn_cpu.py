"""`get_knn_bank` / `get_knn_score` on the CPU, through a stub net whose features are a function of the pixels and whose
`knn_scores` is torch top-k in fp64: against the direct computation in one process, under gloo at world sizes 2 and 3 with
empty and ragged shards, the refusals, `knn_auto_k` and the CLI switch."""
import os
import socket
import types

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


class _StubKnnNet:
    """Features = the first P pixel values plus 0.5 (not unit: the routines must normalise); knn_scores = fp64 top-k."""

    def get_image_features(self, pixel_values):
        return pixel_values.reshape(pixel_values.shape[0], -1)[:, :P].float() + 0.5

    def knn_scores(self, features, bank, k, splits=0, return_values=False):
        v = torch.topk(features.double() @ bank.double().T, int(k), dim=1).values
        s = torch.sqrt(torch.clamp(2.0 - 2.0 * v[:, -1], min=0.0)).float()
        return (s, v.float()) if return_values else s


def _args():
    return types.SimpleNamespace(model="CLIP", normalize=False, feat_dim=P, batch_size=BS)


def _loader(n, seed):
    return torch.utils.data.DataLoader(_Set(n, seed), batch_size=BS, shuffle=False)


def _direct(n_train, n_test, k):
    net = _StubKnnNet()
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)  # noqa: E731
    bank = torch.cat([unit(net.get_image_features(x)) for x, _ in _loader(n_train, 100)])
    f = torch.cat([unit(net.get_image_features(x)) for x, _ in _loader(n_test, 900)])
    return bank, net.knn_scores(f, bank, k).numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


@pytest.mark.parametrize("n_train,n_test,k", [(3, 3, 2), (70, 21, 5), (70, 3, 70)])
def test_single_process_equals_the_direct_computation(n_train, n_test, k):
    from mcm_amd.detection import get_knn_bank, get_knn_score

    net = _StubKnnNet()
    bank = get_knn_bank(_args(), net, _loader(n_train, 100))
    want_bank, want = _direct(n_train, n_test, k)
    assert bank.shape == (n_train, P) and bank.dtype == torch.float32
    assert np.array_equal(_bits(bank.numpy()), _bits(want_bank.numpy()))
    np.testing.assert_allclose(bank.norm(dim=-1).numpy(), 1.0, rtol=1e-6)            # unit rows although args.normalize is False
    got = get_knn_score(_args(), net, _loader(n_test, 900), bank, k)
    assert got.dtype == np.float32 and got.shape == (n_test,)                         # every sample, the ragged last batch too
    assert np.array_equal(_bits(got), _bits(want))


def test_refusals(monkeypatch):
    from mcm_amd import dist as mdist
    from mcm_amd.detection import get_knn_bank, get_knn_score

    net = _StubKnnNet()
    bank = get_knn_bank(_args(), net, _loader(9, 100))
    with pytest.raises(ValueError, match="k = 10"):
        get_knn_score(_args(), net, _loader(5, 900), bank, 10)                         # k > n_train
    with pytest.raises(ValueError):
        get_knn_score(_args(), net, _loader(5, 900), bank, 0)
    with pytest.raises(TypeError, match="knn_scores"):
        get_knn_bank(_args(), types.SimpleNamespace(get_image_features=lambda pixel_values: pixel_values), _loader(9, 100))
    base = _loader(20, 100)

    class Plain:
        dataset = base.dataset

        def __iter__(self):
            raise AssertionError("nothing may be iterated")

    monkeypatch.setattr(mdist, "world", lambda: (1, 2))
    with pytest.raises(TypeError, match="sharded by index"):
        get_knn_bank(_args(), net, Plain())
    with pytest.raises(TypeError, match="sharded by index"):
        get_knn_score(_args(), net, Plain(), bank, 3)


def test_knn_auto_k():
    from mcm_amd.detection import knn_auto_k

    assert knn_auto_k(1_281_167) == 1000
    assert knn_auto_k(12_812) == 10
    assert knn_auto_k(5) == 1
    assert knn_auto_k(10 ** 7) == 1024


# ---- gloo ---------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, ws, port, n_train, k, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from mcm_amd.detection import get_knn_bank, get_knn_score

    dist.init_process_group("gloo", rank=rank, world_size=ws)
    net = _StubKnnNet()
    bank = get_knn_bank(_args(), net, _loader(n_train, 100))
    scores = {n: get_knn_score(_args(), net, _loader(n, 900), bank, k) for n in (3, 21)}
    q.put((rank, bank.numpy(), scores[3], scores[21]))
    dist.destroy_process_group()


@pytest.mark.parametrize("ws,n_train", [(2, 3), (3, 3), (2, 70), (3, 70)])
def test_gloo_shards_equal_single_process(ws, n_train):
    """n = 3 on three ranks: shards of one sample, on two ranks 2 + 1 (and a test set of 3 leaves a rank of a 21 / 3 split
    ragged batches); n_train = 70: 35 + 35 and 24 + 24 + 22.  The bank is the same bits in dataset order on every rank, the
    scores equal the single-process run bit for bit."""
    k = 2 if n_train == 3 else 5
    want_bank, want3 = _direct(n_train, 3, k)
    _, want21 = _direct(n_train, 21, k)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, ws, port, n_train, k, q)) for r in range(ws)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, bank, s3, s21 in got:
        assert np.array_equal(_bits(bank), _bits(want_bank.numpy())), rank
        assert np.array_equal(_bits(s3), _bits(want3)) and np.array_equal(_bits(s21), _bits(want21)), rank


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_switch(tmp_path, monkeypatch):
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    a = cli.process_args(["--in_dataset", "ImageNet10", "--score", "knn"])
    assert a.score == "knn" and a.knn_k == 0
    assert cli.process_args(["--in_dataset", "ImageNet10", "--score", "knn", "--knn-k", "7"]).knn_k == 7
    assert cli.process_args(["--in_dataset", "ImageNet10", "--score", "knn", "--refine-threshold", "auto"]).score == "knn"
    for bad in (["--predict"], ["--refine-threshold", "on"], ["--refine-threshold", "exact"], ["--knn-k", "1025"],
                ["--knn-k", "-1"]):
        with pytest.raises(SystemExit):
            cli.process_args(["--in_dataset", "ImageNet10", "--score", "knn"] + bad)
