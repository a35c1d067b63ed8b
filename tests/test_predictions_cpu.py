"""Host side of the top-k predictions, on the CPU: `zero_shot_accuracy` from its definition, `get_ood_predictions_clip`
with a torch stand-in for the fused call (order, shapes, a ragged last batch), the same under gloo at world sizes 2 and 3
(an empty shard included), and the CLI's `--predict` flag."""
import os
import socket
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

K_BANK = 7


class _TopkNet:
    """`score_images(..., topk=)` in torch on CPU tensors: similarities of the first four pixel values against a fixed bank,
    so every image has its own score, order and probabilities and a shard mix-up is visible."""

    def get_text_features(self, input_ids, attention_mask):
        g = torch.Generator().manual_seed(3)
        return torch.randn(input_ids.shape[0], 4, generator=g)

    def score_images(self, images, text, T, score, topk=0):
        sim = images.reshape(images.shape[0], -1)[:, :4].double() @ text.double().T
        p = torch.softmax(sim / T, dim=1)
        s = -p.max(dim=1).values.float()
        if not topk:
            return s
        order = torch.argsort(-sim, dim=1, stable=True)[:, :topk]
        prob = torch.gather(p, 1, order).float()
        idx = order.to(torch.int32)
        if topk > sim.shape[1]:
            pad = topk - sim.shape[1]
            idx = torch.cat([idx, torch.full((idx.shape[0], pad), -1, dtype=torch.int32)], dim=1)
            prob = torch.cat([prob, torch.full((idx.shape[0], pad), float("nan"))], dim=1)
        return s, idx, prob


def _args():
    return types.SimpleNamespace(ckpt="x", model="CLIP", score="MCM", T=1)


def _single(n, bs, topk):
    from mcm_amd.detection import get_ood_predictions_clip
    from mcm_amd.synth import SyntheticImageSet, SyntheticLoader, class_names

    ds = SyntheticImageSet(n, 8, 3, ood=False, seed=1)
    return get_ood_predictions_clip(_args(), _TopkNet(), SyntheticLoader(ds, bs), class_names(K_BANK), topk=topk)


# ---- zero_shot_accuracy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_zero_shot_accuracy_from_the_definition(dtype):
    from mcm_amd.detection import zero_shot_accuracy

    idx = np.array([[2, 0, 1],      # label 2: hit at 1
                    [0, 1, 2],      # label 1: hit at 2
                    [1, 2, 0],      # label 0: hit at 3
                    [1, -1, -1],    # label 2: no hit
                    [-1, -1, -1]],  # label -1: a -1 slot never matches, not even a -1 label
                   dtype=dtype)
    labels = np.array([2, 1, 0, 2, -1], dtype=dtype)
    acc = zero_shot_accuracy(idx, labels, ks=(1, 2, 3))
    assert acc == {1: 1 / 5, 2: 2 / 5, 3: 3 / 5}
    assert zero_shot_accuracy(torch.from_numpy(idx), torch.from_numpy(labels), ks=(1,)) == {1: 1 / 5}
    assert zero_shot_accuracy(idx, labels.astype(np.int64 if dtype == np.int32 else np.int32), ks=(3,)) == {3: 3 / 5}
    with pytest.raises(ValueError):
        zero_shot_accuracy(idx, labels, ks=(1, 5))        # k beyond the topk the indices hold
    with pytest.raises(ValueError):
        zero_shot_accuracy(idx, labels, ks=(0,))
    with pytest.raises(ValueError):
        zero_shot_accuracy(idx, labels[:3])
    with pytest.raises(ValueError):
        zero_shot_accuracy(idx, labels)                   # default ks = (1, 5) on topk = 3


# ---- get_ood_predictions_clip, one process ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bs,topk", [(37, 5, 5), (16, 8, 1), (3, 4, 8)])
def test_predictions_order_and_shapes(n, bs, topk):
    """A ragged last batch (37 = 7 x 5 + 2), a single short batch, and topk beyond the bank (-1 / NaN slots pass through):
    sample i of every array belongs to image i of the loader, and the scores are `get_ood_scores_clip`'s."""
    from mcm_amd.detection import get_ood_predictions_clip, get_ood_scores_clip, prompt_bank, zero_shot_accuracy
    from mcm_amd.synth import SyntheticImageSet, SyntheticLoader, class_names

    ds = SyntheticImageSet(n, 8, 3, ood=False, seed=1)
    net = _TopkNet()
    scores, idx, prob, labels = get_ood_predictions_clip(_args(), net, SyntheticLoader(ds, bs), class_names(K_BANK), topk=topk)
    assert scores.shape == (n,) and scores.dtype == np.float32
    assert idx.shape == (n, topk) and idx.dtype == np.int32
    assert prob.shape == (n, topk) and prob.dtype == np.float32
    assert labels.shape == (n,) and labels.dtype == np.int64
    np.testing.assert_array_equal(scores, get_ood_scores_clip(_args(), net, SyntheticLoader(ds, bs), class_names(K_BANK)))
    # image by image, straight from the stand-in on the whole set at once
    px = torch.cat([x for x, _ in SyntheticLoader(ds, n)])
    want_lab = torch.cat([y for _, y in SyntheticLoader(ds, n)]).numpy()
    bank = prompt_bank(_args(), net, class_names(K_BANK))
    ws, wi, wp = net.score_images(px, bank, 1.0, "MCM", topk=topk)
    np.testing.assert_array_equal(scores, ws.numpy())
    np.testing.assert_array_equal(idx, wi.numpy())
    np.testing.assert_array_equal(prob, wp.numpy())
    np.testing.assert_array_equal(labels, want_lab)
    if topk > K_BANK:
        assert (idx[:, K_BANK:] == -1).all() and np.isnan(prob[:, K_BANK:]).all()
    assert 0.0 <= zero_shot_accuracy(idx, labels, ks=(1,))[1] <= 1.0
    dev = get_ood_predictions_clip(_args(), net, SyntheticLoader(ds, bs), class_names(K_BANK), topk=topk, device_out=True)
    assert all(isinstance(t, torch.Tensor) for t in dev) and len(dev) == 4
    np.testing.assert_array_equal(dev[1].numpy(), idx)


def test_predictions_refuse_what_the_scores_refuse():
    from mcm_amd.detection import get_ood_predictions_clip
    from mcm_amd.synth import SyntheticImageSet, SyntheticLoader, class_names

    loader = SyntheticLoader(SyntheticImageSet(4, 8, 3, ood=False, seed=1), 4)
    bad = _args()
    bad.score = "maha"
    with pytest.raises(ValueError):
        get_ood_predictions_clip(bad, _TopkNet(), loader, class_names(3))
    with pytest.raises(TypeError):
        get_ood_predictions_clip(_args(), object(), loader, class_names(3))


# ---- the same under gloo ------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, ws, port, n, bs, topk, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=ws)
    q.put((rank,) + _single(n, bs, topk))
    dist.destroy_process_group()


@pytest.mark.parametrize("ws,n,bs", [(2, 37, 5), (3, 40, 12), (3, 2, 4), (2, 1, 4)])
def test_gathered_predictions_equal_single_process(ws, n, bs):
    """World sizes 2 and 3: ragged shards, and sets smaller than the world (n = 2 on 3 ranks, n = 1 on 2: a rank with an
    EMPTY shard still takes part in every collective).  Every rank ends with the one-process arrays, dtype and order kept."""
    topk = 5
    want = _single(n, bs, topk)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, ws, port, n, bs, topk, q)) for r in range(ws)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(g[0] for g in got) == list(range(ws))
    for g in got:
        for have, ref in zip(g[1:], want):
            assert have.dtype == ref.dtype and have.shape == ref.shape
            np.testing.assert_array_equal(have, ref)


def test_all_gather_rows_without_a_group_is_the_identity():
    from mcm_amd.dist import all_gather_rows

    t = torch.arange(6, dtype=torch.int32).reshape(3, 2)
    assert all_gather_rows(t, 3) is t


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_predict_flag(tmp_path, monkeypatch, capsys):
    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)   # (process_args creates the log directory under the working directory)
    base = ["--in_dataset", "ImageNet10", "--data-dir", os.path.join(os.path.dirname(cli.__file__), "data")]
    assert cli.process_args(base).predict == 0                       # default: off
    assert cli.process_args(base + ["--predict"]).predict == 5       # without a value: 5
    assert cli.process_args(base + ["--predict", "3"]).predict == 3
    assert cli.process_args(base + ["--predict", "--score", "energy"]).predict == 5
    for bad in (["--predict", "--score", "maha"], ["--predict", "9"], ["--predict", "-1"]):
        with pytest.raises(SystemExit):
            cli.process_args(base + bad)
    assert "maha" in capsys.readouterr().err
