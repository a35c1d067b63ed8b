"""`get_glmcm_scores` on the CPU, through a stub net whose global and local features are functions of the pixels and whose
`score_images_glmcm` is the definition in fp64: against the direct computation in one process, under gloo at world sizes 2
and 3 with empty and ragged shards, the refusal of a net without the method, the re-export and the CLI switch."""
import os
import socket
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

P, R, BS = 4, 5, 8
LABELS = ["cat", "dog", "tree"]


class _Set(torch.utils.data.Dataset):
    def __init__(self, n, seed):
        self.n, self.seed = n, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed + int(i))
        return torch.randn(3, 4, 4, generator=g), int(i) % 3


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


class _StubGlNet:
    """Global feature = the first P pixel values, local rows = the next R P; the score is the definition in fp64."""

    def __init__(self):
        self.calls = []

    def get_text_features(self, input_ids, attention_mask):
        k = input_ids.shape[0]
        return torch.cos(torch.arange(k * P, dtype=torch.float32).reshape(k, P) + 1.0)

    def score_images_glmcm(self, images, text, T, lam):
        self.calls.append((int(images.shape[0]), float(T), float(lam)))
        flat = images.reshape(images.shape[0], -1).double()
        g, loc = _unit(flat[:, :P]), _unit(flat[:, P:P + R * P].reshape(-1, R, P))
        t = text.double()
        s_g = torch.softmax(g @ t.T / T, dim=-1).max(dim=-1).values
        s_l = torch.softmax(loc @ t.T / T, dim=-1).max(dim=-1).values.max(dim=-1).values
        return (-(s_g + lam * s_l)).float()


def _args(lam=None, T=1):
    a = types.SimpleNamespace(ckpt="x", model="CLIP", score="GL-MCM", T=T)
    if lam is not None:
        a.gl_lambda = lam
    return a


def _loader(n, seed=900):
    return torch.utils.data.DataLoader(_Set(n, seed), batch_size=BS, shuffle=False)


def _direct(n, lam, T=1):
    from mcm_amd.detection import prompt_bank

    net = _StubGlNet()
    text = prompt_bank(_args(), net, LABELS)
    images = torch.stack([_Set(n, 900)[i][0] for i in range(n)])
    return net.score_images_glmcm(images, text, float(T), lam).numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


@pytest.mark.parametrize("n", [1, 3, 21])
@pytest.mark.parametrize("lam", [None, 0.5])
def test_single_process_equals_the_direct_computation(n, lam):
    from mcm_amd.detection import get_glmcm_scores

    net = _StubGlNet()
    got = get_glmcm_scores(_args(lam), net, _loader(n), LABELS)
    assert got.dtype == np.float32 and got.shape == (n,)                              # every sample, the ragged last batch too
    assert np.array_equal(_bits(got), _bits(_direct(n, 1.0 if lam is None else lam)))
    assert sum(c[0] for c in net.calls) == n
    assert {c[2] for c in net.calls} == {1.0 if lam is None else lam}                 # --gl-lambda reaches the net; 1 by default
    dev = get_glmcm_scores(_args(lam), net, _loader(n), LABELS, device_out=True)
    assert isinstance(dev, torch.Tensor) and np.array_equal(_bits(dev.numpy()), _bits(got))


def test_refusal_and_reexport():
    from mcm_amd.detection import get_glmcm_scores
    from utils import detection_util

    assert detection_util.get_glmcm_scores is get_glmcm_scores
    plain = types.SimpleNamespace(score_images=lambda *a: None)
    with pytest.raises(TypeError, match="score_images_glmcm"):
        get_glmcm_scores(_args(), plain, _loader(3), LABELS)


# ---- gloo ---------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, ws, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from mcm_amd.detection import get_glmcm_scores

    dist.init_process_group("gloo", rank=rank, world_size=ws)
    net = _StubGlNet()
    scores = {n: get_glmcm_scores(_args(0.5), net, _loader(n), LABELS) for n in (1, 3, 21)}
    q.put((rank, scores[1], scores[3], scores[21], sum(c[0] for c in net.calls)))
    dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 3])
def test_gloo_shards_equal_single_process(ws):
    """n = 1: every rank but one has an empty shard; n = 3: shards of one sample (2 + 1 on two ranks); n = 21: 11 + 10 and
    7 + 7 + 7, ragged batches of the loader's 8.  Every rank ends with the single-process scores, bit for bit, and the ranks
    together scored every sample once."""
    want = {n: _direct(n, 0.5) for n in (1, 3, 21)}
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
    for rank, s1, s3, s21, _seen in got:
        for n, s in ((1, s1), (3, s3), (21, s21)):
            assert s.shape == (n,) and np.array_equal(_bits(s), _bits(want[n])), (rank, n)
    assert sum(t[4] for t in got) == 1 + 3 + 21


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_switch(tmp_path, monkeypatch):
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    base = ["--in_dataset", "ImageNet10", "--score", "GL-MCM"]
    a = cli.process_args(base)
    assert a.score == "GL-MCM" and a.gl_lambda == 1.0
    assert a.refine_threshold == "off"                                                # auto resolves to off
    assert cli.process_args(base + ["--gl-lambda", "0.25"]).gl_lambda == 0.25
    assert cli.process_args(base + ["--refine-threshold", "off", "--dtype", "bf16"]).dtype == "bf16"
    for bad in (["--refine-threshold", "on"], ["--refine-threshold", "exact"], ["--dtype", "fp16x2"], ["--gl-lambda", "nan"],
                ["--gl-lambda", "inf"]):
        with pytest.raises(SystemExit):
            cli.process_args(base + bad)
    assert cli.process_args(["--in_dataset", "ImageNet10"]).gl_lambda == 1.0         # the switch exists for every score
    from mcm_amd.config import SCORE_KINDS

    assert "GL-MCM" not in SCORE_KINDS                                                # the fused tail's kinds are what they were
