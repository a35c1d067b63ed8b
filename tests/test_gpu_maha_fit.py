"""The device Mahalanobis fit on a real MI355X: mcm_maha_fit_accumulate (score.hip maha_fit_kernel) against longdouble sums
under tests/maha_fit_budget.py, its determinism / symmetry / refusal contract, and get_mean_prec_device end to end against the
host route, the reference's own outputs (tests/golden/maha_tiny.npz) and through the CLI.  Each kernel case prints
"BUDGET maha-fit fp64 <max |got - ref| / budget> ..." (run with -s to collect them)."""
import os
import types

import numpy as np
import pytest

from tests import gpu_scaffold as gs
from tests import maha_fit_budget as fb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_dev = gs.dev

# proj_dim must be a multiple of 4 (mcm_create); the kernel's tile is 64 wide: 64 is one tile, 100 one full and one ragged,
# 1024 sixteen (136 workgroups); the Mahalanobis widths of tests/test_gpu_eval_tail.py, and 1024
WIDTHS = [64, 100, 512, 768, 1024]


@pytest.fixture(scope="module")
def fit_nets():
    yield from gs.net_cache(lambda P: gs.widened_net(P, max_batch=512 if P == 512 else 72))


def _run(net, x, splits, shift):
    """Accumulate the rows of x in calls of the given sizes; (gram, sum) as numpy, n checked."""
    state = net.maha_fit_state(None if shift is None else _dev(shift))
    xd, s = _dev(x), 0
    for b in splits:
        net.maha_fit_accumulate(xd[s:s + b], state)
        s += b
    assert s == x.shape[0] and state["n"] == s
    assert state["gram"].dtype == torch.float64 and state["sum"].dtype == torch.float64 and state["shift"].dtype == torch.float32
    return state["gram"].cpu().numpy(), state["sum"].cpu().numpy()


@pytest.mark.parametrize("P", WIDTHS)
def test_kernel_within_budget(fit_nets, P):
    """B = 1, 17 (less than one staged step), 65 + 64 + 3 (three calls, the steps' edge on both sides, a ragged last one)
    and, at P = 512, one call of 512; with no shift and with the first call's column mean.  gram against the first budget
    term, sum against the second one's source, entry by entry; gram symmetric bit for bit."""
    net = fit_nets(P)
    assert net.geo.proj_dim == P
    for splits in [(1,), (17,), (65, 64, 3)] + ([(512,)] if P == 512 else []):
        n = sum(splits)
        x = fb.fit_case(n, P, 20.0, seed=len(splits), offset_kind="randn")
        for use_shift in (False, True):
            shift = fb.first_batch_shift(x, splits[0]) if use_shift else None
            gram, fsum = _run(net, x, splits, shift)
            xs = fb.shifted(x, shift)
            gref, sref, gown, sown = fb.gram_sum_reference(xs)
            rg, ig = fb.entry_ratio(gram, gref, fb.gram_budget(xs) + gown)
            rs, isum = fb.entry_ratio(fsum, sref, fb.sum_budget(xs) + sown)
            print(f"BUDGET maha-fit fp64 {rg:.3f} gram {rs:.3f} sum P={P} B={splits} shift={use_shift}")
            assert np.isfinite(gram).all() and np.isfinite(fsum).all()
            assert np.array_equal(gram, gram.T), (P, splits, use_shift)
            assert rg <= 1.0, (P, splits, use_shift, rg, gram.flat[ig], gref.flat[ig])
            assert rs <= 1.0, (P, splits, use_shift, rs, fsum[isum], sref[isum])


@pytest.mark.parametrize("P", [100, 512])
def test_kernel_is_deterministic_and_accumulates(fit_nets, P):
    net = fit_nets(P)
    x = fb.fit_case(132, P, 20.0, seed=9, offset_kind="randn")
    shift = fb.first_batch_shift(x, 65)
    a = _run(net, x, (65, 64, 3), shift)
    b = _run(net, x, (65, 64, 3), shift)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])          # the same bits on a second run
    assert np.array_equal(a[0], a[0].T)
    one = _run(net, x, (132,), shift)
    assert np.array_equal(a[0], one[0]) and np.array_equal(a[1], one[1])      # ... and for any split of the rows into calls
    last = _run(net, x[129:], (3,), shift)                                     # the last call alone: the calls before it count
    assert not np.array_equal(a[0], last[0]) and not np.array_equal(a[1], last[1])
    first = _run(net, x[:65], (65,), shift)
    assert (np.diag(a[0]) > np.diag(first[0])).all()                           # sums of squares only grow


def test_refused_calls_touch_nothing(fit_nets):
    from mcm_amd.engine import _stream_ptr

    net = fit_nets(100)
    P = 100
    f = _dev(fb.fit_case(8, P, 0.0))
    gram = torch.full((P, P), 3.25, device="cuda", dtype=torch.float64)
    fsum = torch.full((P,), -1.5, device="cuda", dtype=torch.float64)
    call = net._lib.mcm_maha_fit_accumulate
    assert call(net._h, f.data_ptr(), 0, None, gram.data_ptr(), fsum.data_ptr(), _stream_ptr()) == -1      # B = 0
    assert call(net._h, f.data_ptr(), -3, None, gram.data_ptr(), fsum.data_ptr(), _stream_ptr()) == -1
    assert call(net._h, f.data_ptr(), 8, None, None, fsum.data_ptr(), _stream_ptr()) == -1                 # NULL outputs
    assert call(net._h, f.data_ptr(), 8, None, gram.data_ptr(), None, _stream_ptr()) == -1
    assert call(net._h, None, 8, None, gram.data_ptr(), fsum.data_ptr(), _stream_ptr()) == -1
    assert call(None, f.data_ptr(), 8, None, gram.data_ptr(), fsum.data_ptr(), _stream_ptr()) == -1
    torch.cuda.synchronize()
    assert (gram == 3.25).all() and (fsum == -1.5).all()
    with pytest.raises(RuntimeError):
        net.maha_fit_accumulate(torch.empty((0, P), device="cuda"), net.maha_fit_state())
    with pytest.raises(ValueError):
        net.maha_fit_accumulate(torch.zeros((2, P + 4), device="cuda"), net.maha_fit_state())
    # a good call on the same buffers adds to what they hold (the lower triangle is the upper one's mirror)
    assert call(net._h, f.data_ptr(), 8, None, gram.data_ptr(), fsum.data_ptr(), _stream_ptr()) == 0
    torch.cuda.synchronize()
    x = f.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(gram.cpu().numpy(), 3.25 + x.T @ x, rtol=1e-13)
    np.testing.assert_allclose(fsum.cpu().numpy(), -1.5 + x.sum(axis=0), rtol=1e-13)


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net32():
    from mcm_amd.config import TEST_GEOMETRIES
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = TEST_GEOMETRIES["tiny"]
    n = NativeCLIP(geo, synth_state_dict(geo, seed=0), precision="fp32", max_batch=64, max_prompt_tokens=64 * 16)
    yield n
    n.close()


def test_end_to_end_vs_host_route_and_reference(net32, golden_dir, tmp_path):
    """The loaders and sizes of tests/test_gpu_maha.py::test_end_to_end_vs_reference: get_mean_prec_device against
    get_mean_prec on the same net, and against the reference's own run on HF."""
    from mcm_amd.detection import get_Mahalanobis_score, get_mean_prec, get_mean_prec_device
    from mcm_amd.synth import make_pixels

    net = net32
    g = np.load(os.path.join(golden_dir, "maha_tiny.npz"))
    n_cls, bs, geo = int(g["n_cls"]), int(g["batch"]), net.geo

    class DS:
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

    class Loader:
        def __init__(self, n, ood, seed):
            self.dataset, self.ood, self.seed = DS(n), ood, seed

        def __len__(self):
            return -(-self.dataset.n // bs)

        def __iter__(self):
            for s in range(0, self.dataset.n, bs):
                n = min(bs, self.dataset.n - s)
                px, lab = make_pixels(n, geo.image_size, n_cls, ood=self.ood, seed=self.seed, start=s)
                yield torch.from_numpy(px), torch.from_numpy(lab)

    n_train = int(g["n_train"])
    for normalize, tag in ((False, "raw"), (True, "norm")):
        def args(sub):
            return types.SimpleNamespace(n_cls=n_cls, feat_dim=geo.proj_dim, model="CLIP", normalize=normalize,
                                         template_dir=str(tmp_path / sub), in_dataset="ImageNet10", max_count=250, batch_size=bs)

        mean_h, prec_h = get_mean_prec(args("host"), net, Loader(n_train, False, 7))
        mean_d, prec_d, cov = get_mean_prec_device(args("dev"), net, Loader(n_train, False, 7), return_cov=True)
        assert np.array_equal(mean_d.numpy().view(np.int32), mean_h.numpy().view(np.int32))
        with torch.no_grad():
            F = torch.cat([net.get_image_features(pixel_values=px).float() for px, _ in Loader(n_train, False, 7)])
            if normalize:
                F = F / F.norm(dim=-1, keepdim=True)
            shift = F[:bs].mean(dim=0).cpu().numpy()
        F = F.cpu().numpy()
        ref, own = fb.cov_reference(F)
        bud = fb.cov_budget(F, shift) + own
        r, i = fb.cov_ratio(cov.numpy(), F, shift)
        prec_ref, bound = fb.precision_bound(ref, bud)
        rp = float((np.abs(prec_d.numpy().astype(np.float64) - prec_ref) / bound).max())
        print(f"BUDGET maha-fit fp64 {r:.3f} covariance {rp:.3f} precision (bound / max|precision| "
              f"{float(bound.max() / np.abs(prec_ref).max()):.1e}) n={n_train} P={geo.proj_dim} {tag}")
        assert r <= 1.0, (tag, r, i)
        assert rp <= 1.0, (tag, rp)
        np.testing.assert_allclose(mean_d.numpy(), g[f"mean_{tag}"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(prec_d.numpy(), g[f"prec_{tag}"], rtol=2e-3, atol=2e-3 * np.abs(g[f"prec_{tag}"]).max())
        for what in ("classwise_mean", "precision"):
            assert os.path.exists(tmp_path / "dev" / f"CLIP_{what}_ImageNet10_250_{normalize}.pt")
        s_h = get_Mahalanobis_score(args("host"), net, Loader(int(g["n_id"]), False, 1), mean_h, prec_h, in_dist=True)
        s_d = get_Mahalanobis_score(args("dev"), net, Loader(int(g["n_id"]), False, 1), mean_d, prec_d, in_dist=True)
        print(f"maha scores, device fit vs host fit: max |d| {float(np.abs(s_d - s_h).max()):.3e} "
              f"(scores up to {float(np.abs(s_h).max()):.3e}) {tag}")


def test_cli_maha_device_fit(tmp_path, monkeypatch):
    import pandas as pd

    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    cli.main(["--in_dataset", "ImageNet10", "--CLIP_ckpt", "ViT-B/32", "-b", "64", "--synthetic-n", "640",
              "--score", "maha", "--maha-fit", "device", "--name", "m", "--dtype", "fp16"])
    df = pd.read_csv(tmp_path / "results" / "ImageNet10" / "maha" / "CLIP_ViT-B/32_T_1_ID_m" / "m.csv", index_col=0)
    assert list(df.index) == ["ImageNet20", "AVG"] and np.isfinite(df.values).all()
    for what in ("classwise_mean", "precision"):
        assert os.path.exists(tmp_path / "img_templates" / f"CLIP_{what}_ImageNet10_250_False.pt")
