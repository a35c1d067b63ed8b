"""The k-nearest-neighbour score on a real MI355X: mcm_knn_score_features (knn.hip) against the fp64 reference of
tests/knn_budget.py — value for value on lattice inputs (every similarity exact in fp32), inside the derived budget on unit
inputs — its invariance, edge and refusal contract, a bank beyond 4 GiB, and get_knn_bank / get_knn_score / the CLI end to end.
Budget cases print "BUDGET knn fp32 <worst ratio> ..." (run with -s to collect them)."""
import ctypes
import types

import numpy as np
import pytest

from tests import gpu_scaffold as gs
from tests import knn_budget as kb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_dev = gs.dev

WIDTHS = [64, 512, 768, 1024]
# one row; 63 / 65 and 255 / 257 rows: either side of a wave's 64 candidates and of the 256-row tile; 65 and 130 queries: a
# ragged second and third query tile; 3001 rows: twelve tiles, the last one ragged
SHAPES = [(1, 1), (3, 63), (3, 65), (65, 255), (65, 257), (130, 3001)]
KS = [1, 2, 63, 64, 65, 1000, 1024]
SPLITS = [1, 2, 7]


@pytest.fixture(scope="module")
def knn_nets():
    yield from gs.net_cache()


def _run(net, f, bank, k, splits=0):
    s, v = net.knn_scores(f, bank, k, splits=splits, return_values=True)
    return s.cpu().numpy(), v.cpu().numpy()


def _score32(vk):
    return kb.score_of(vk).astype(np.float32)


def _check_exact(got_s, got_v, ref_full, k, what):
    ref = ref_full[:, :k]
    assert got_v.shape == ref.shape, what
    assert np.array_equal(got_v.astype(np.float64), ref), (what, np.argwhere(got_v.astype(np.float64) != ref)[:4])
    want = _score32(ref[:, k - 1])
    fin = np.isfinite(want)
    assert np.array_equal(got_s[~fin], want[~fin]), what
    assert (np.abs(got_s[fin].astype(np.float64) - want[fin]) <= np.spacing(want[fin])).all(), what
    return int((got_s.view(np.int32) != want.view(np.int32)).sum())


@pytest.mark.parametrize("P", WIDTHS)
def test_exact_selection_on_lattice_inputs(knn_nets, P):
    net = knn_nets(P)
    off, cases = 0, 0
    for B, N in SHAPES:
        f, bank = kb.lattice_case(B, N, P, seed=B + N)
        ref_full = kb.top_from_similarities(kb.similarities(f, bank), max(KS))
        fd, bd = _dev(f), _dev(bank)
        for k in KS:
            for splits in SPLITS:
                s, v = _run(net, fd, bd, k, splits)
                off += _check_exact(s, v, ref_full, k, (P, B, N, k, splits))
                cases += 1
    print(f"EXACT knn lattice P={P}: {cases} cases, lists equal in every slot; {off} score(s) not bit-equal to float32(sqrt(2 - 2 v)) "
          "(all within one fp32 ulp)")


def test_exact_selection_with_the_library_choosing_the_splits(knn_nets):
    net = knn_nets(512)
    f, bank = kb.lattice_case(130, 20000, 512, seed=11)
    ref_full = kb.top_from_similarities(kb.similarities(f, bank), 200)
    s, v = _run(net, _dev(f), _dev(bank), 200, 0)
    off = _check_exact(s, v, ref_full, 200, "splits=0")
    print(f"EXACT knn lattice splits=0 N=20000 B=130 k=200: {off} score(s) not bit-equal")


@pytest.mark.parametrize("P", WIDTHS)
def test_unit_inputs_within_budget(knn_nets, P):
    net = knn_nets(P)
    f, bank = kb.unit_case(65, 3001, P, seed=P)
    eps = kb.eps_rows(f, bank)
    ref_full = kb.top_from_similarities(kb.similarities(f, bank), 1000)
    fd, bd = _dev(f), _dev(bank)
    for k in [1, 10, 200, 1000]:
        s, v = _run(net, fd, bd, k)
        ref = ref_full[:, :k]
        rl, rs = kb.list_ratio(v, ref, eps), kb.score_ratio(s, ref[:, k - 1], eps)
        print(f"BUDGET knn fp32 {max(rl, rs):.3f} (lists {rl:.3f}, scores {rs:.3f}) P={P} B=65 N=3001 k={k}")
        assert (np.diff(v, axis=1) <= 0).all()                                          # sorted, descending
        assert rl <= 1.0 and rs <= 1.0, (P, k, rl, rs)


@pytest.mark.parametrize("k", [10, 1000])
def test_outputs_are_a_pure_function_of_the_inputs(knn_nets, k):
    net = knn_nets(512)
    f, bank = kb.unit_case(65, 3001, 512, seed=7)
    fd, bd = _dev(f), _dev(bank)
    s1, v1 = _run(net, fd, bd, k, 1)
    for splits in (2, 7, 0, 1):                                                         # ... and a second run of splits = 1
        s, v = _run(net, fd, bd, k, splits)
        assert np.array_equal(s.view(np.int32), s1.view(np.int32)) and np.array_equal(v.view(np.int32), v1.view(np.int32)), splits
    for cut in ((1, 64), (33, 32)):                                                     # the queries in two calls
        parts = [_run(net, fd[a:a + n], bd, k, 2) for a, n in zip((0, cut[0]), cut)]
        assert np.array_equal(np.concatenate([p[0] for p in parts]).view(np.int32), s1.view(np.int32)), cut
        assert np.array_equal(np.concatenate([p[1] for p in parts]).view(np.int32), v1.view(np.int32)), cut
    perm = np.random.default_rng(0).permutation(65)                                     # a query's row position does not matter
    s, v = _run(net, _dev(f[perm]), bd, k, 7)
    assert np.array_equal(s.view(np.int32), s1[perm].view(np.int32)) and np.array_equal(v.view(np.int32), v1[perm].view(np.int32))


def test_edges(knn_nets):
    from mcm_amd.engine import _stream_ptr

    net, P = knn_nets(64), 64
    f, bank = kb.unit_case(5, 300, P, seed=3)
    bank = bank.copy()
    bank[5] = np.nan                                                                    # a NaN bank row is never selected
    ref = kb.top_from_similarities(kb.similarities(f, bank), 300)
    eps = kb.eps_rows(f, np.delete(bank, 5, axis=0))
    for splits in (1, 3):
        s, v = _run(net, _dev(f), _dev(bank), 300, splits)
        assert not np.isnan(v).any() and np.isneginf(v[:, 299]).all() and np.isfinite(v[:, :299]).all()
        assert kb.list_ratio(v, ref, eps) <= 1.0 and np.isposinf(s).all()
    fq = f.copy()
    fq[2] = np.nan                                                                      # an all-NaN query row
    s, v = _run(net, _dev(fq), _dev(bank), 4, 2)
    assert np.isneginf(v[2]).all() and np.isposinf(s[2]) and np.isfinite(v[[0, 1, 3, 4]]).all()
    # s == 1 exactly gives 0; s == 1.25 clamps to 0
    e0 = np.zeros((1, P), np.float32)
    e0[0, 0] = 1.0
    plant = np.zeros((260, P), np.float32)
    plant[:, 1] = 1.0
    plant[258, :2] = (1.0, 0.0)
    s, v = _run(net, _dev(e0), _dev(plant), 1, 2)
    assert v[0, 0] == 1.0 and s[0] == 0.0
    s, v = _run(net, _dev(e0), _dev(plant), 2, 2)
    assert list(v[0]) == [1.0, 0.0] and s[0] == np.float32(np.sqrt(2.0))
    plant[3, 0] = 1.25
    s, v = _run(net, _dev(e0), _dev(plant), 1, 1)
    assert v[0, 0] == 1.25 and s[0] == 0.0
    # duplicates on either side of a split boundary both appear: 10 rows in 2 splits of 5, rows 4 and 5 the same bits
    fl, bl = kb.lattice_case(3, 10, P, seed=9)
    bl = bl.copy()
    bl[4] = bl[5] = fl[0] * 3.0                                                         # (multiples of 2^-11 still: exact)
    ref = kb.top_from_similarities(kb.similarities(fl, bl), 10)
    s, v = _run(net, _dev(fl), _dev(bl), 2, 2)
    assert np.array_equal(v.astype(np.float64), ref[:, :2]) and v[0, 0] == v[0, 1]
    # topv_dev = NULL: the same scores
    fd, bd = _dev(f), _dev(kb.unit_case(5, 300, P, seed=3)[1])
    s1, _ = _run(net, fd, bd, 7, 2)
    need = ctypes.c_int64(0)
    assert net._lib.mcm_knn_workspace_bytes(net._h, 5, 300, 7, 2, ctypes.byref(need)) == 0 and need.value == 2 * 5 * 7 * 4
    work = torch.empty(need.value // 4, device="cuda")
    out = torch.empty(5, device="cuda")
    assert net._lib.mcm_knn_score_features(net._h, fd.data_ptr(), 5, bd.data_ptr(), 300, 7, 2, work.data_ptr(), need.value,
                                           out.data_ptr(), None, _stream_ptr()) == 0
    assert np.array_equal(out.cpu().numpy().view(np.int32), s1.view(np.int32))


def test_refused_calls_launch_nothing(knn_nets):
    from mcm_amd.engine import _stream_ptr

    net, P = knn_nets(64), 64
    f, bank = kb.unit_case(5, 300, P, seed=3)
    fd, bd = _dev(f), _dev(bank)
    work = torch.full((32 * 5 * 8,), 7.5, device="cuda")
    out = torch.full((5,), -2.5, device="cuda")
    topv = torch.full((5, 8), -3.5, device="cuda")
    call, sp = net._lib.mcm_knn_score_features, _stream_ptr
    wb = work.numel() * 4

    def go(h=net._h, fp=fd.data_ptr(), B=5, bp=bd.data_ptr(), N=300, k=8, splits=2, wp=work.data_ptr(), nbytes=wb, op=out.data_ptr()):
        return call(h, fp, B, bp, N, k, splits, wp, nbytes, op, topv.data_ptr(), sp())

    assert go(h=None) == -1
    assert go(fp=None) == -1 and go(bp=None) == -1 and go(wp=None) == -1 and go(op=None) == -1
    assert go(B=0) == -1 and go(B=-1) == -1 and go(N=0) == -1 and go(N=-5) == -1
    assert go(k=0) == -1 and go(k=1025) == -1 and go(splits=-1) == -1 and go(splits=33) == -1
    assert go(nbytes=2 * 5 * 8 * 4 - 1) == -1
    assert go(fp=fd.data_ptr() + 4) == -1                                               # rows are read 16 bytes at a time
    need = ctypes.c_int64(-1)
    wbytes = net._lib.mcm_knn_workspace_bytes
    assert wbytes(net._h, 5, 300, 8, 33, ctypes.byref(need)) == -1 and wbytes(net._h, 5, 300, 0, 1, ctypes.byref(need)) == -1
    assert wbytes(None, 5, 300, 8, 1, ctypes.byref(need)) == -1 and wbytes(net._h, 5, 300, 8, 1, None) == -1
    assert need.value == -1
    assert wbytes(net._h, 5, 300, 8, 0, ctypes.byref(need)) == 0 and need.value % (5 * 8 * 4) == 0 and 1 <= need.value // 160 <= 32
    torch.cuda.synchronize()
    assert (work == 7.5).all() and (out == -2.5).all() and (topv == -3.5).all()
    with pytest.raises(ValueError):
        net.knn_scores(fd, bd, 2000)
    with pytest.raises(ValueError):
        net.knn_scores(fd[:, :60], bd, 3)
    assert go() == 0                                                                    # the same buffers take a good call
    torch.cuda.synchronize()
    assert (out != -2.5).all() and (topv != -3.5).all()


def test_bank_beyond_4_gib(knn_nets):
    """N = 1 100 000 rows of 1024 floats (4.5 GB): lattice rows planted at row 0, on either side of byte offset 2^32 (rows
    1 048 575 and 1 048 576) and at the last row, zeros elsewhere: the four largest similarities of every query are known."""
    net, P, N = knn_nets(1024), 1024, 1_100_000
    f, rows = kb.lattice_case(3, 4, P, seed=21)
    at = [0, (1 << 32) // (4 * P) - 1, (1 << 32) // (4 * P), N - 1]
    bank = torch.zeros((N, P), device="cuda", dtype=torch.float32)
    bank[at] = _dev(rows)
    sims = kb.similarities(f, rows)
    ref = kb.top_from_similarities(np.concatenate([sims, np.zeros((3, 4))], axis=1), 4)
    assert (np.abs(sims) > 0).all()
    for splits in (0, 3):
        s, v = _run(net, _dev(f), bank, 4, splits)
        _check_exact(s, v, ref, 4, ("4GiB", splits))
    # every planted row alone must be seen: k = N's worth is not needed, the largest of each query names its row
    s, v = _run(net, _dev(f), bank, 1, 0)
    assert np.array_equal(v[:, 0].astype(np.float64), np.maximum(sims.max(axis=1), 0.0))
    del bank
    torch.cuda.empty_cache()


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _tiny(precision):
    from mcm_amd.config import TEST_GEOMETRIES
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = TEST_GEOMETRIES["tiny"]
    return NativeCLIP(geo, synth_state_dict(geo, seed=0), precision=precision, max_batch=64, max_prompt_tokens=64 * 16)


def test_end_to_end_against_torch():
    from mcm_amd.detection import get_knn_bank, get_knn_score
    from mcm_amd.synth import make_pixels

    bs, k = 64, 5
    args = types.SimpleNamespace(model="CLIP", normalize=False, batch_size=bs)
    out = {}
    for precision in ("fp32", "fp16"):
        net = _tiny(precision)
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

        train, sets = Loader(192, False, 7), {"id": Loader(64, False, 1), "ood": Loader(64, True, 2)}
        bank = get_knn_bank(args, net, train)
        assert bank.shape == (192, geo.proj_dim) and bank.is_cuda
        got = {w: get_knn_score(args, net, ld, bank, k) for w, ld in sets.items()}
        out[precision] = got
        if precision == "fp32":
            with torch.no_grad():
                ref_bank = torch.cat([net.get_image_features(px, normalize=True) for px, _ in train]).cpu().numpy()
                for w, ld in sets.items():
                    fr = torch.cat([net.get_image_features(px, normalize=True) for px, _ in ld]).cpu().numpy()
                    eps = kb.eps_rows(fr, ref_bank)
                    ref, _ = kb.knn_reference(fr, ref_bank, k)
                    r = kb.score_ratio(got[w], ref[:, k - 1], eps)
                    print(f"BUDGET knn fp32 {r:.3f} end to end, {w}: 192 training images, 64 scored, k={k}, P={geo.proj_dim}")
                    assert got[w].shape == (64,) and np.isfinite(got[w]).all()
                    assert r <= 1.0, (w, r)
        net.close()
    for w in ("id", "ood"):
        print(f"knn scores, fp16 arm vs fp32 arm, {w}: max |d| {float(np.abs(out['fp16'][w] - out['fp32'][w]).max()):.3e} "
              f"(scores up to {float(out['fp32'][w].max()):.3e}); recorded, no bar")


def test_cli_knn(tmp_path, monkeypatch):
    import pandas as pd

    import eval_ood_detection as cli

    monkeypatch.chdir(tmp_path)
    res = cli.main(["--in_dataset", "ImageNet10", "--CLIP_ckpt", "ViT-B/32", "-b", "64", "--score", "knn", "--synthetic",
                    "--synthetic-n", "128", "--knn-k", "5", "--name", "n", "--dtype", "fp16"])
    logdir = tmp_path / "results" / "ImageNet10" / "knn" / "CLIP_ViT-B/32_T_1_ID_n"
    log = open(logdir / "ood_eval_info.log").read()
    assert "k = 5" in log and "bank of 128" in log
    df = pd.read_csv(logdir / "n.csv", index_col=0)
    assert list(df.index) == ["ImageNet20", "AVG"] and np.isfinite(df.values).all()
    assert set(res["measures"]) == {"ImageNet20"} and res["in_score"].shape == (128,) and np.isfinite(res["in_score"]).all()
