"""GL-MCM's local features from the vision tower on a real MI355X (mcm_encode_image_local, mcm_score_glmcm),
with seeded weights, against an fp64 restatement written here from HF `CLIPModel`: the last layer's input from
`output_hidden_states`, then layer_norm1, v_proj, out_proj, post_layernorm and visual_projection applied to the rows and the
rows normalised.

The yardstick is the call's own global rows: their max abs error against the same fp64 model is the parent path's error in
this arm at this geometry, and the local rows may err by at most 8 times that.  (The local path shares the tower up to the
last layer and then does fewer operations than the CLS row; the factor absorbs the maximum being taken over R times as many
components, and post_layernorm of rows with a smaller spread.)  Each case prints "BUDGET glmcm tower ..." with the ratio."""
import warnings

import numpy as np
import pytest

from tests.error_budget import u8_normalise

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FACTOR = 8.0
# (precision, weight_operands)
ARMS = [("fp32", "auto"), ("fp16", "single"), ("bf16", "single"), ("fp16", "split")]
CASES = [("tiny", 1), ("tiny", 3), ("tiny", 8), ("B16-2L", 2)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def models():
    """(geo, state dict, fp64 HF model on the device) per geometry, built once."""
    from mcm_amd.config import geometry
    from mcm_amd.weights import synth_state_dict
    from oracle.hf_reference import HFReference, hf_available

    if hf_available() is not None:
        pytest.fail(f"transformers CLIPModel is needed for the reference: {hf_available()}")
    made = {}

    def get(name):
        if name not in made:
            geo = geometry(name)
            sd = synth_state_dict(geo, 0)
            made[name] = (geo, sd, HFReference(geo, sd, device="cuda").model.double())
        return made[name]

    yield get
    made.clear()


def _net(geo, sd, precision, operands="auto", max_batch=8):
    from mcm_amd.engine import NativeCLIP

    return NativeCLIP(geo, sd, precision=precision, max_batch=max_batch, max_prompt_tokens=256, weight_operands=operands,
                      x2_max_batch=-1 if precision != "fp16x2" else None)


def _pixels(geo, B, seed=1):
    from mcm_amd.synth import make_pixels

    px, _ = make_pixels(B, geo.image_size, 10, ood=False, seed=seed)
    return torch.from_numpy(px).cuda()


def _reference(model, px):
    """(global [B,P], local [B,R,P]) in fp64: unit rows."""
    with torch.no_grad():
        vm = model.vision_model
        out = vm(pixel_values=px.double(), output_hidden_states=True)
        h = out.hidden_states[-2]                      # the residual stream entering the last encoder layer
        layer = vm.encoder.layers[-1]
        o = layer.self_attn.out_proj(layer.self_attn.v_proj(layer.layer_norm1(h)))
        y = model.visual_projection(vm.post_layernorm(o))[:, 1:, :]
        g = model.visual_projection(out.pooler_output)
        return (g / g.norm(dim=-1, keepdim=True)).cpu().numpy(), (y / y.norm(dim=-1, keepdim=True)).cpu().numpy()


def _check_case(models, name, B, precision, operands):
    geo, sd, model = models(name)
    net = _net(geo, sd, precision, operands)
    try:
        px = _pixels(geo, B)
        g_ref, l_ref = _reference(model, px)
        before = net.get_image_features(px, normalize=True).cpu().numpy()
        g, loc = net.get_local_features(px)
        g, loc = g.cpu().numpy(), loc.cpu().numpy()
        after = net.get_image_features(px, normalize=True).cpu().numpy()
        R = (geo.image_size // geo.patch_size) ** 2
        assert loc.shape == (B, R, geo.proj_dim) and np.isfinite(loc).all()
        assert np.array_equal(_bits(g), _bits(before)) and np.array_equal(_bits(after), _bits(before))
        np.testing.assert_allclose(np.linalg.norm(loc.astype(np.float64), axis=-1), 1.0, atol=1e-6)
        e_g = float(np.abs(g - g_ref).max())
        e_l = float(np.abs(loc - l_ref).max())
        print(f"BUDGET glmcm tower {e_l / e_g:.3f} of {FACTOR:g} ({name} B={B} {precision} weights={operands}: local max abs error "
              f"{e_l:.3e}, global {e_g:.3e}, split={net.split_weights})")
        assert net.saturation_count() == 0
        assert e_l <= FACTOR * e_g, (name, B, precision, operands, e_l, e_g)
    finally:
        net.close()


@pytest.mark.parametrize("precision,operands", ARMS)
@pytest.mark.parametrize("name,B", CASES)
def test_local_rows_against_the_fp64_model(models, name, B, precision, operands):
    _check_case(models, name, B, precision, operands)


def test_local_rows_h14(models):
    """1280 columns (the wide LayerNorm and GEMM routes), P = 1024, 257 tokens: fp16 only."""
    _check_case(models, "H14-2L", 2, "fp16", "auto")


@pytest.mark.parametrize("precision,operands", ARMS)
def test_the_score_is_its_parts(models, precision, operands):
    """mcm_score_glmcm's parts are mcm_score's and mcm_local_score_features' bits on mcm_encode_image_local's rows, the
    combination is the fp64 one rounded once, and a plain score before and after is untouched.  B = 3: a ragged batch."""
    geo, sd, _model = models("tiny")
    net = _net(geo, sd, precision, operands)
    try:
        B, K, T, lam = 3, 10, 0.5, 0.75
        px = _pixels(geo, B, seed=4)
        text = torch.randn(K, geo.proj_dim, generator=torch.Generator().manual_seed(1))
        text = (text / text.norm(dim=-1, keepdim=True)).cuda()
        plain = net.score_images(px, text, T, "MCM").cpu().numpy()
        score, gs, ls, patch = [t.cpu().numpy() for t in net.score_images_glmcm(px, text, T, lam, return_parts=True)]
        only = net.score_images_glmcm(px, text, T, lam).cpu().numpy()               # the parts left in the workspace
        again = net.score_images(px, text, T, "MCM").cpu().numpy()
        assert np.array_equal(_bits(plain), _bits(again)) and np.array_equal(_bits(gs), _bits(plain))
        _g, loc = net.get_local_features(px)
        ls2, patch2 = [t.cpu().numpy() for t in net.local_scores(loc, text, T, return_patches=True)]
        assert np.array_equal(_bits(ls), _bits(ls2)) and np.array_equal(_bits(patch), _bits(patch2))
        assert np.array_equal(_bits(only), _bits(score))
        want = gs.astype(np.float64) + float(np.float32(lam)) * ls.astype(np.float64)
        assert (np.abs(score.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
        assert (score < 0).all() and (ls < 0).all() and (ls >= -1).all()
        assert net.saturation_count() == 0
        if precision == "fp16":   # uint8 ingest gives the bits of the fp32 pixels it decodes to
            u8 = torch.randint(0, 256, (B, geo.image_size, geo.image_size, 3), dtype=torch.uint8,
                               generator=torch.Generator().manual_seed(2))
            pf = torch.from_numpy(u8_normalise(u8.numpy())).cuda()
            a = [t.cpu().numpy() for t in net.get_local_features(u8.cuda())]
            b = [t.cpu().numpy() for t in net.get_local_features(pf)]
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
            sa = net.score_images_glmcm(u8.cuda(), text, T, lam).cpu().numpy()
            sb = net.score_images_glmcm(pf, text, T, lam).cpu().numpy()
            assert np.array_equal(_bits(sa), _bits(sb))
    finally:
        net.close()


def test_chunks_of_max_batch_and_refusals(models):
    """More images than max_batch go through in chunks with the same bits; the split-activation arm and bad arguments are
    refused."""
    from mcm_amd.engine import _stream_ptr

    geo, sd, _model = models("tiny")
    net = _net(geo, sd, "fp16", max_batch=4)
    try:
        px = _pixels(geo, 6, seed=7)
        g, loc = net.get_local_features(px)
        g2, loc2 = net.get_local_features(px[4:])
        assert torch.equal(g[4:], g2) and torch.equal(loc[4:], loc2)
        text = torch.randn(5, geo.proj_dim, generator=torch.Generator().manual_seed(1))
        text = (text / text.norm(dim=-1, keepdim=True)).cuda()
        R, P = net.local_rows, geo.proj_dim
        gl = torch.full((2, P), -2.5, device="cuda")
        lo = torch.full((2, R, P), -3.5, device="cuda")
        enc, sc, sp = net._lib.mcm_encode_image_local, net._lib.mcm_score_glmcm, _stream_ptr
        p2 = px[:2].contiguous()
        assert enc(None, p2.data_ptr(), 0, 2, gl.data_ptr(), lo.data_ptr(), sp()) == -1
        assert enc(net._h, None, 0, 2, gl.data_ptr(), lo.data_ptr(), sp()) == -1
        assert enc(net._h, p2.data_ptr(), 0, 2, None, lo.data_ptr(), sp()) == -1
        assert enc(net._h, p2.data_ptr(), 0, 2, gl.data_ptr(), None, sp()) == -1
        assert enc(net._h, p2.data_ptr(), 2, 2, gl.data_ptr(), lo.data_ptr(), sp()) == -1       # unknown pixel format
        assert enc(net._h, p2.data_ptr(), 0, 0, gl.data_ptr(), lo.data_ptr(), sp()) != 0
        assert enc(net._h, p2.data_ptr(), 0, 5, gl.data_ptr(), lo.data_ptr(), sp()) != 0        # beyond max_batch
        out = torch.full((2,), -4.5, device="cuda")

        def score(tp=text.data_ptr(), K=5, T=1.0, lam=1.0, op=out.data_ptr()):
            return sc(net._h, p2.data_ptr(), 0, 2, tp, K, T, lam, op, None, None, None, sp())

        assert score(tp=None) == -1 and score(op=None) == -1 and score(K=0) == -1 and score(T=0.0) == -1
        assert score(T=float("nan")) == -1 and score(lam=float("inf")) == -1 and score(lam=float("nan")) == -1
        torch.cuda.synchronize()
        assert (gl == -2.5).all() and (lo == -3.5).all() and (out == -4.5).all()
        assert score() == 0
        torch.cuda.synchronize()
        assert (out != -4.5).all()
    finally:
        net.close()
    x2 = _net(geo, sd, "fp16x2")
    try:
        with pytest.raises(ValueError, match="split-activation"):
            x2.get_local_features(_pixels(geo, 2))
        with pytest.raises(ValueError, match="split-activation"):
            x2.score_images_glmcm(_pixels(geo, 2), text, 1.0)
    finally:
        x2.close()


def test_cli_glmcm(tmp_path, monkeypatch):
    import pandas as pd

    import eval_ood_detection as cli
    from mcm_amd.metrics import get_measures

    monkeypatch.chdir(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        res = cli.main(["--in_dataset", "ImageNet10", "--CLIP_ckpt", "ViT-B/32", "-b", "64", "--score", "GL-MCM", "--synthetic",
                        "--synthetic-n", "128", "--gl-lambda", "0.5", "--name", "g", "--dtype", "fp16"])
    logdir = tmp_path / "results" / "ImageNet10" / "GL-MCM" / "CLIP_ViT-B/32_T_1_ID_g"
    log = open(logdir / "ood_eval_info.log").read()
    assert "--score GL-MCM: -(S_G + 0.5 S_L) at T = 1, 49 patch rows per image" in log
    df = pd.read_csv(logdir / "g.csv", index_col=0)
    assert list(df.index) == ["ImageNet20", "AVG"] and np.isfinite(df.values).all()
    ins, outs = res["in_score"], res["out_scores"]["ImageNet20"]
    assert ins.shape == (128,) and outs.shape == (128,) and np.isfinite(ins).all() and np.isfinite(outs).all()
    assert (ins < 0).all() and (ins >= -1.5).all()                                      # -(S_G + 0.5 S_L), both in (0, 1]
    auroc, aupr, fpr = get_measures(-ins, -outs)
    assert res["measures"]["ImageNet20"] == (auroc, aupr, fpr)
    np.testing.assert_allclose(df.loc["ImageNet20"].values, np.round([100 * fpr, 100 * auroc, 100 * aupr], 2), atol=1e-9)
