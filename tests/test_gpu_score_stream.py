"""The streamed tail of the MCM family on a real MI355X: mcm_score_features_stream (score_stream.hip) against the fp64 reference and
the derived budget of tests/score_stream_budget.py — the arithmetic term plus one ulp on lattice inputs (every similarity exact
in fp32), the full budget on unit inputs — against the LDS tail, its top-k order, determinism, NaN and refusal contract, and the
engine's routing past the LDS tail's bank size.  Budget cases print "BUDGET score_stream <worst ratio> ..." (run with -s)."""
import ctypes
import types

import numpy as np
import pytest

from tests import error_budget as eb
from tests import gpu_scaffold as gs
from tests import score_stream_budget as sb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
_dev = gs.dev
_bits = gs.bits

WIDTHS = [4, 36, 64, 512, 1024]   # 36: not a multiple of the walk's 32-column chunk
# (B, K).  (1,1): one row, with 32 splits thirty-one of them are empty; (3,300): the bank across the tile edge, 32 splits of 10
# rows, the last two empty; (64,255): one row short of a tile; (65,256): exactly a tile, a second query tile of one row;
# (130,257): one row past the edge, a ragged third query tile; (65,1000): splits of several tiles, three of 334: both boundaries
# inside a tile
SHAPES = [(1, 1), (3, 300), (64, 255), (65, 256), (130, 257), (65, 1000)]
SPLITS = [1, 2, 3, 32]
TEMPS = [0.01, 1.0]
K_CAP, P_CAP = 38337, 64          # the first K the LDS tail refuses at P = 64: (64 + 38337) * 4 = 150 KiB + 4


@pytest.fixture(scope="module")
def nets():
    yield from gs.net_cache()


def _run(net, fd, bd, T, splits, kind="MCM", topk=0):
    """{kind: [B]} from parts, "scores" [B], and with topk "idx" / "prob"."""
    res = net.score_features(fd, bd, T, kind, topk=topk, tail="stream", splits=splits, return_parts=True)
    parts = res[-1].cpu().numpy()
    out = {k: parts[:, i].copy() for i, k in enumerate(sb.KINDS)}
    out["scores"] = res[0].cpu().numpy()
    if topk:
        out["idx"], out["prob"] = res[1].cpu().numpy().astype(np.int64), res[2].cpu().numpy()
    return out


def _same_bits(a, b, rows=slice(None), keys=sb.KINDS):
    return gs.same_bits(a, b, rows, keys)


@pytest.mark.parametrize("P", WIDTHS)
def test_lattice_inputs_within_the_arithmetic_term(nets, P):
    net = nets(P)
    worst, where, cases = 0.0, None, 0
    for B, K in SHAPES:
        f, bank = sb.lattice_case(B, K, P, seed=B + K)
        fd, bd = _dev(f), _dev(bank)
        for T in TEMPS:
            ref = sb.reference(f, bank, T)
            bud = sb.budgets(f, bank, T, exact=True)
            for splits in SPLITS + [0]:
                got = _run(net, fd, bd, T, splits)
                r, k = sb.worst_ratio(got, ref, bud)
                cases += 1
                if r > worst:
                    worst, where = r, (B, K, T, splits, k)
                assert r <= 1.0, (P, B, K, T, splits, k, r)
                assert np.array_equal(_bits(got["scores"]), _bits(got["MCM"]))
                for i, kind in enumerate(sb.KINDS[1:], 1):              # scores is the bits of parts[:, kind]
                    one = net.score_features(fd, bd, T, kind, tail="stream", splits=splits)
                    assert np.array_equal(_bits(one.cpu().numpy()), _bits(got[kind])), (P, B, K, T, splits, kind)
    print(f"BUDGET score_stream {worst:.3f} lattice (arithmetic term + one ulp) P={P}: {cases} cases, worst at "
          f"(B, K, T, splits, kind) = {where}")


@pytest.mark.parametrize("P", [64, 512])
def test_unit_inputs_within_budget(nets, P):
    net = nets(P)
    for B, K in SHAPES:
        f, bank = sb.unit_case(B, K, P, seed=P + K)
        fd, bd = _dev(f), _dev(bank)
        ref = sb.reference(f, bank, 0.01)
        bud = sb.budgets(f, bank, 0.01)
        xbud = sb.budgets(f, bank, 0.01, exact=True)
        per_split, worst, where = {}, 0.0, None
        for splits in SPLITS:
            got = per_split[splits] = _run(net, fd, bd, 0.01, splits)
            r, k = sb.worst_ratio(got, ref, bud)
            if r > worst:
                worst, where = r, (splits, k)
            assert r <= 1.0, (P, B, K, splits, k, r)
        print(f"BUDGET score_stream {worst:.3f} unit P={P} B={B} K={K} T=0.01 splits={SPLITS}, worst at (splits, kind) = {where}")
        # across splits the similarities are the same bits and only the sums are associated differently: two results differ
        # by at most twice the arithmetic term plus one ulp
        for a in SPLITS[1:]:
            for k in sb.KINDS:
                assert (np.abs(per_split[a][k].astype(np.float64) - per_split[1][k]) <= 2 * xbud[k]).all(), (P, B, K, a, k)
            assert np.array_equal(_bits(per_split[a]["max-logit"]), _bits(per_split[1]["max-logit"]))


@pytest.mark.parametrize("T", TEMPS)
def test_against_the_lds_tail_on_lattice_inputs(nets, T):
    """Similarities are exact on both routes.  The LDS tail's budget is tests/error_budget.py's score_budget for the five kinds;
    it has none for prob there, so prob is held to the streamed budget twice."""
    P, topk = 64, 5
    net = nets(P)
    worst = {}
    for B, K in SHAPES:
        f, bank = sb.lattice_case(B, K, P, seed=B + K)
        fd, bd = _dev(f), _dev(bank)
        s64 = sb.similarities(f, bank)
        idx_ref = sb.topk_reference(s64, T, topk)[0]
        bud = sb.budgets(f, bank, T, exact=True, prob_idx=idx_ref)
        for kind_no, kind in enumerate(sb.KINDS):
            lds, lidx, lprob = (t.cpu().numpy() for t in net.score_features(fd, bd, T, kind, topk=topk, tail="lds"))
            got = _run(net, fd, bd, T, 0, kind, topk)
            assert np.array_equal(got["idx"], lidx.astype(np.int64)) and np.array_equal(got["idx"], idx_ref), (B, K, kind)
            if kind == "max-logit":
                assert np.array_equal(_bits(got["scores"]), _bits(lds)), (B, K)
                continue
            room = eb.score_budget(f, bank, T, kind_no)[1] + bud[kind]
            r = float((np.abs(got["scores"].astype(np.float64) - lds) / room).max())
            worst[kind] = max(worst.get(kind, 0.0), r)
            assert r <= 1.0, (B, K, kind, r)
            have = idx_ref >= 0
            rp = float((np.abs(got["prob"].astype(np.float64) - lprob)[have] / (2 * bud["prob"][have])).max())
            worst["prob"] = max(worst.get("prob", 0.0), rp)
            assert np.isnan(got["prob"][~have]).all() and np.isnan(lprob[~have]).all()
    print(f"BUDGET score_stream vs the LDS tail, lattice P={P} T={T}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert worst["prob"] <= 1.0, worst


@pytest.mark.parametrize("topk", [1, 5, 8])
def test_topk_order_is_the_stable_argsort(nets, topk):
    P = 64
    net = nets(P)
    B, K = 65, 1000
    f, bank = sb.lattice_case(B, K, P, seed=3)                          # rows K // 2 and K - 1 are copies of rows 0 and 1
    bank[256] = bank[255]                                               # duplicates on both sides of a tile edge ...
    bank[334] = bank[333]                                               # ... and of the boundary of three splits of 334
    bank[500] = bank[499]                                               # ... and of two splits of 500
    f[:6] = bank[[255, 256, 333, 334, 0, 1]]                            # queries whose best rows are the duplicated ones
    fd, bd = _dev(f), _dev(bank)
    s64 = sb.similarities(f, bank)
    for T in TEMPS:
        idx, prob = sb.topk_reference(s64, T, topk)
        bud = sb.budgets_from_similarities(s64, np.zeros_like(s64), T, prob_idx=idx)
        for splits in SPLITS + [0]:
            got = _run(net, fd, bd, T, splits, "MCM", topk)
            assert np.array_equal(got["idx"], idx), (T, splits)
            assert sb.prob_ratio(got["prob"], prob, bud["prob"]) <= 1.0, (T, splits)
            assert np.array_equal(_bits(got["prob"][:, 0]), _bits(-got["scores"])), (T, splits)
    assert idx[0, :2].tolist() == [255, 256] or topk == 1


def test_topk_zeros_nan_rows_and_more_slots_than_rows(nets):
    """K = 6 < topk = 8: a +0 row and a -0 row (equal similarities: the lower row first), a NaN row (never a candidate; every
    score of every query is NaN, as a softmax over it would be), and slots without a candidate (-1 / NaN)."""
    P = 64
    net = nets(P)
    f, bank = sb.lattice_case(4, 6, P, seed=5)
    bank[2], bank[3] = -0.0, 0.0
    clean = _run(net, _dev(f), _dev(bank), 1.0, 2, "MCM", 8)
    s64 = sb.similarities(f, bank)
    idx, prob = sb.topk_reference(s64, 1.0, 8)
    assert np.array_equal(clean["idx"], idx) and (clean["idx"][:, 6:] == -1).all() and np.isnan(clean["prob"][:, 6:]).all()
    pos2 = np.argmax(idx == 2, axis=1)
    assert (idx[np.arange(4), pos2 + 1] == 3).all()                     # the zero pair: row 2 straight before row 3
    bud = sb.budgets_from_similarities(s64, np.zeros_like(s64), 1.0, prob_idx=idx)
    assert sb.prob_ratio(clean["prob"], prob, bud["prob"]) <= 1.0
    bank[4] = np.nan
    for splits in (1, 2, 32):
        got = _run(net, _dev(f), _dev(bank), 1.0, splits, "MCM", 8)
        want = np.where(idx == 4, -2, idx)                              # the reference order without row 4
        want = np.stack([np.concatenate([r[r != -2], [-1]]) for r in want])
        assert np.array_equal(got["idx"], want), splits
        assert all(np.isnan(got[k]).all() for k in sb.KINDS) and np.isnan(got["prob"]).all()


def test_same_bits_over_runs_query_cuts_and_row_positions(nets):
    net = nets(512)
    B, K = 130, 1000
    f, bank = sb.unit_case(B, K, 512, seed=5)
    fd, bd = _dev(f), _dev(bank)
    keys = sb.KINDS + ("scores", "idx", "prob")
    for splits in SPLITS:
        first = _run(net, fd, bd, 0.01, splits, "entropy", 5)
        assert _same_bits(_run(net, fd, bd, 0.01, splits, "entropy", 5), first, keys=keys), splits
        cuts = [_run(net, fd[a:a + n], bd, 0.01, splits, "entropy", 5) for a, n in ((0, 1), (1, 64), (65, 65))]
        joined = {k: np.concatenate([c[k] for c in cuts]) for k in keys}
        assert _same_bits(joined, first, keys=keys), splits
        perm = np.random.default_rng(splits).permutation(B)
        moved = _run(net, _dev(f[perm]), bd, 0.01, splits, "entropy", 5)
        assert _same_bits(moved, {k: first[k][perm] for k in keys}, keys=keys), splits


def test_a_nan_stays_in_its_row(nets):
    net = nets(64)
    B, K = 5, 300
    f, bank = sb.unit_case(B, K, 64, seed=3)
    fq = f.copy()
    fq[2, 7] = np.nan
    keep = [0, 1, 3, 4]
    keys = sb.KINDS + ("scores", "idx", "prob")
    for splits in (1, 3):
        clean = _run(net, _dev(f), _dev(bank), 0.01, splits, "var", 5)
        got = _run(net, _dev(fq), _dev(bank), 0.01, splits, "var", 5)
        assert all(np.isnan(got[k][2]) for k in sb.KINDS) and np.isnan(got["prob"][2]).all() and (got["idx"][2] == -1).all()
        assert _same_bits(got, clean, keep, keys=keys)


def test_refused_calls_launch_nothing(nets):
    """Every refusal of the header but proj_dim % 4 != 0, which mcm_create refuses before a handle exists."""
    from mcm_amd.engine import _stream_ptr

    net, P = nets(64), 64
    B, K, topk = 5, 300, 5
    f, bank = sb.unit_case(B, K, P, seed=3)
    fd, bd = _dev(f), _dev(bank)
    want = _run(net, fd, bd, 0.01, 2, "energy", topk)                   # (binds the two entries)
    slot = 32 + 8 * topk
    work = torch.full((32 * B * slot // 4,), 7.5, device="cuda")
    out = torch.full((B,), -2.5, device="cuda")
    parts = torch.full((B, 5), -3.5, device="cuda")
    idx = torch.full((B, topk), -7, dtype=torch.int32, device="cuda")
    prob = torch.full((B, topk), -4.5, device="cuda")
    call, sp = net._lib.mcm_score_features_stream, _stream_ptr
    wb = work.numel() * 4

    def go(h=net._h, fp=fd.data_ptr(), B=B, bp=bd.data_ptr(), K=K, T=0.01, kind=2, topk=topk, splits=2, wp=work.data_ptr(),
           nbytes=wb, op=out.data_ptr(), pp=parts.data_ptr(), ip=idx.data_ptr(), qp=prob.data_ptr()):
        return call(h, fp, B, bp, K, T, kind, topk, splits, wp, nbytes, op, pp, ip, qp, sp())

    assert go(h=None) == -1
    assert go(fp=None) == -1 and go(bp=None) == -1 and go(wp=None) == -1 and go(op=None) == -1
    assert go(B=0) == -1 and go(B=-1) == -1 and go(K=0) == -1 and go(K=-3) == -1
    assert go(K=2 ** 31) == -1 and go(K=2 ** 40) == -1                                  # rows are numbered in int32
    assert go(T=0.0) == -1 and go(T=-0.01) == -1 and go(T=float("inf")) == -1 and go(T=float("nan")) == -1
    assert go(kind=-1) == -1 and go(kind=5) == -1
    assert go(topk=-1) == -1 and go(topk=9) == -1 and go(ip=None) == -1
    assert go(splits=-1) == -1 and go(splits=33) == -1
    assert go(nbytes=2 * B * slot - 1) == -1
    assert go(fp=fd.data_ptr() + 4) == -1 and go(bp=bd.data_ptr() + 8) == -1            # rows are read 16 bytes at a time
    assert go(wp=work.data_ptr() + 4) == -1                                             # slots hold doubles
    need = ctypes.c_int64(-1)
    wbytes = net._lib.mcm_score_stream_workspace_bytes
    assert wbytes(net._h, B, K, topk, 33, ctypes.byref(need)) == -1 and wbytes(net._h, B, K, 9, 1, ctypes.byref(need)) == -1
    assert wbytes(net._h, 0, K, topk, 1, ctypes.byref(need)) == -1 and wbytes(net._h, B, 0, topk, 1, ctypes.byref(need)) == -1
    assert wbytes(None, B, K, topk, 1, ctypes.byref(need)) == -1 and wbytes(net._h, B, K, topk, 1, None) == -1
    assert wbytes(net._h, B, 2 ** 31, topk, 1, ctypes.byref(need)) == -1
    assert need.value == -1
    assert wbytes(net._h, B, K, topk, 2, ctypes.byref(need)) == 0 and need.value == 2 * B * slot
    assert wbytes(net._h, B, K, 0, 0, ctypes.byref(need)) == 0 and need.value % (B * 32) == 0 and 1 <= need.value // (B * 32) <= 32
    torch.cuda.synchronize()
    assert (work == 7.5).all() and (out == -2.5).all() and (parts == -3.5).all() and (idx == -7).all() and (prob == -4.5).all()
    with pytest.raises(ValueError, match="T="):
        net.score_features(fd, bd, 0.0, tail="stream")
    with pytest.raises(ValueError, match="splits="):
        net.score_features(fd, bd, 0.01, tail="stream", splits=33)
    with pytest.raises(ValueError, match="topk"):
        net.score_features(fd, bd, 0.01, tail="stream", topk=9)
    with pytest.raises(ValueError, match="tail"):
        net.score_features(fd, bd, 0.01, tail="hbm")
    with pytest.raises(ValueError, match="streamed tail"):
        net.score_features(fd, bd, 0.01, tail="lds", return_parts=True)
    assert go(pp=None, qp=None) == 0                                                    # parts_dev and prob_dev are optional
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want["energy"])) and (parts == -3.5).all() and (prob == -4.5).all()
    assert np.array_equal(idx.cpu().numpy(), want["idx"])
    assert go(topk=0, ip=None, qp=None) == 0                                            # ... and so is idx_dev without topk
    # no word of the workspace is read before it is written: a NaN-filled one gives the same bits (32 splits of 10 rows: the
    # last two are empty)
    for fill in (float("nan"), 3.0e38):
        work.fill_(fill)
        assert go(splits=32) == 0
        torch.cuda.synchronize()
        w32 = _run(net, fd, bd, 0.01, 32, "energy", topk)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(w32["energy"])) and torch.isfinite(parts).all()
        assert np.array_equal(_bits(parts.cpu().numpy()[:, 3]), _bits(w32["entropy"]))
        assert np.array_equal(idx.cpu().numpy(), w32["idx"]) and np.array_equal(_bits(prob.cpu().numpy()), _bits(w32["prob"]))


# ---- past the LDS tail's bank size: what fails on the code before the streamed tail ------------------------------------------
@pytest.fixture(scope="module")
def cap():
    """(net, f, bank, fd, bd, s64): three planted unit queries against a unit bank of K_CAP rows, on tiny's own proj_dim."""
    net = gs.widened_net(P_CAP)
    f, bank = sb.unit_case(3, K_CAP, P_CAP, seed=17)
    yield net, f, bank, _dev(f), _dev(bank), sb.similarities(f, bank)
    net.close()


def test_past_the_cap_auto_streams_and_lds_refuses(cap):
    net, f, bank, fd, bd, s64 = cap
    assert (P_CAP + K_CAP) * 4 > 150 * 1024 >= (P_CAP + K_CAP - 1) * 4
    with pytest.raises(RuntimeError):
        net.score_features(fd, bd, 0.01, "MCM", tail="lds")
    with pytest.raises(RuntimeError):
        net.score_features(fd, bd, 0.01, "MCM", topk=5, tail="lds")
    with pytest.raises(RuntimeError):
        net.score_features(fd, bd, 0.01, "MCM")                                         # this call's default stays the LDS tail
    below = net.score_features(fd, bd[:1000], 0.01, "entropy", tail="auto")             # "auto" below the cap: the LDS tail's bits
    assert torch.equal(below.view(torch.int32), net.score_features(fd, bd[:1000], 0.01, "entropy", tail="lds").view(torch.int32))
    net.score_features(fd, bd[:K_CAP - 1], 0.01, "MCM", tail="lds")                     # the last K the LDS tail takes
    E = sb.eps_elements(f, bank)
    for T in TEMPS:
        ref = sb.reference_from_similarities(s64, T)
        idx, prob = sb.topk_reference(s64, T, 5)
        bud = sb.budgets_from_similarities(s64, E, T, prob_idx=idx)
        got = {}
        for kind in sb.KINDS:
            got[kind] = net.score_features(fd, bd, T, kind, tail="auto").cpu().numpy()
            s5, i5, p5 = (t.cpu().numpy() for t in net.score_features(fd, bd, T, kind, topk=5, tail="auto"))
            assert np.array_equal(_bits(s5), _bits(got[kind])), (T, kind)
            # the order is the reference's wherever the fp32 similarities cannot have swapped two of the best six
            top6 = -np.sort(-s64, axis=1)[:, :6]
            safe = (top6[:, :-1] - top6[:, 1:]).min(axis=1) > 2 * E.max(axis=1)
            assert safe.any() and np.array_equal(i5[safe].astype(np.int64), idx[safe]), (T, kind)
            assert sb.prob_ratio(p5[safe], prob[safe], bud["prob"][safe]) <= 1.0, (T, kind)
        r, k = sb.worst_ratio(got, ref, bud)
        print(f"BUDGET score_stream {r:.3f} past the cap: unit P={P_CAP} B=3 K={K_CAP} T={T} tail=auto, worst at {k}")
        assert r <= 1.0, (T, k, r)
        kinds = net.score_kinds(fd, bd, T).cpu().numpy()
        assert all(np.array_equal(_bits(kinds[:, i]), _bits(got[k])) for i, k in enumerate(sb.KINDS))


def _pixels(net, n, seed):
    from mcm_amd.synth import make_pixels

    return torch.from_numpy(make_pixels(n, net.geo.image_size, 10, ood=False, seed=seed)[0]).cuda()


def test_past_the_cap_images_equal_features_on_the_same_arm(cap):
    net, _f, _bank, _fd, bd, _s = cap
    px = _pixels(net, 3, seed=1)
    for x2 in (False, True):
        feats = (net.get_image_features_x2 if x2 else net.get_image_features)(px, normalize=True)
        score_images = net.score_images_x2 if x2 else net.score_images
        for kind in ("MCM", "entropy"):
            want = net.score_features(feats, bd, 0.01, kind, topk=5, tail="stream")
            got = score_images(px, bd, 0.01, kind, topk=5)
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want)), (x2, kind)
            plain = score_images(px, bd, 0.01, kind)
            assert torch.equal(plain.view(torch.int32), want[0].view(torch.int32)), (x2, kind)
        with pytest.raises(RuntimeError):
            score_images(px, bd, 0.01, "MCM", tail="lds")


def test_past_the_cap_predictions_through_detection(cap):
    from mcm_amd.detection import get_ood_predictions_clip

    net, _f, _bank, _fd, bd, _s = cap
    labels = [f"concept{i}" for i in range(K_CAP)]
    args = types.SimpleNamespace(model="CLIP", score="MCM", T=1, ckpt="", weights=None)
    net._bank_cache = {(tuple(labels), None, ""): bd}                                   # the bank as prompt_bank would keep it
    px = _pixels(net, 6, seed=2)

    class Loader:
        dataset = list(range(6))

        def __iter__(self):
            for s in (0, 4):
                yield px[s:s + 4].cpu(), torch.arange(s, min(s + 4, 6))

    s, i, p, lab = get_ood_predictions_clip(args, net, Loader(), labels, topk=5)
    ws, wi, wp = (t.cpu().numpy() for t in net.score_images(px, bd, 1.0, "MCM", topk=5))
    assert np.array_equal(_bits(s), _bits(ws)) and np.array_equal(i, wi) and np.array_equal(_bits(p), _bits(wp))
    assert lab.tolist() == list(range(6)) and s.shape == (6,) and np.isfinite(s).all() and (i >= 0).all()


def test_past_the_cap_a_captured_graph_replays_the_eager_bits(cap):
    from mcm_amd.engine import GraphedScorer

    net, _f, _bank, _fd, bd, _s = cap
    px = _pixels(net, 3, seed=4)
    eager = net.score_images(px, bd, 0.01, "energy").clone()
    scorer = GraphedScorer(net, batch=3, bank=bd, T=0.01, score="energy")
    for _ in range(2):
        got = scorer(px)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), eager.view(torch.int32))
