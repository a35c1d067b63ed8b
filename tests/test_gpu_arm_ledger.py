"""The launch ledger of the A/B arms: every harness switch must change WHICH kernels a forward pass launches.

The tail, ROW64, head-major, chunk and n-split arms give the shipped path's bits (or its bits to round-off) by design,
and the tests that hold them to that (test_gpu_ln_tail.py, test_gpu_ln_row.py, test_gpu_qkv_layout.py, ...) pass just
as well when an edit of the host orchestration silently stops an arm from engaging.  This test closes that gap: one
B/16 handle of three layers, one score_images per switch setting under the library's own profiler, and the launches
per kernel class (engine.KERNEL_CLASSES, mcm_profile_read) compared with a recorded ledger.  Three rows of the shipped
library pin its own launch sequence the same way.

Shape: ViT-B/16 with 3 vision layers (layer 1's layer_norm1 is the one folded into / produced by layer 0's fc2, layer 2
is the row-0-only layer) and 1 text layer, fp16, batch 64 = 12 608 token rows, run as 12 800 = 50 row tiles; 50 x 3 = 150
tiles at N = 768 is more than half of 256 workgroups, so the residual GEMMs take the ping-pong kernel and every arm's
size condition holds.  The ragged batch of 37 is below it.

The ledger was recorded with these very functions on an MI355X from the libraries of the commit BEFORE the arm
orchestration moved out of mcm_api.hip into mcm_api_arms.hpp; the move must not change one number of it."""
import dataclasses

import pytest
import torch

from mcm_amd.config import geometry
from mcm_amd.engine import KERNEL_CLASSES, NativeCLIP
from mcm_amd.synth import make_token_ids
from mcm_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu

BATCH = 64
# setting -> ((switch, value) ..., batch).  A switch is the X of mcm_debug_X; every one is back at OFF behind each row.
OFF = {"ln_fold": 0, "ln_tail": 0, "ln_cluster": 0, "ln_cluster_spin": -1, "ln_row": 0, "qkv_head_major": 0,
       "qkv_chunks": 1, "nsplit": 1, "patch_fold": 1}
SETTINGS = {
    "off": ((), BATCH),
    "ln_fold": ((("ln_fold", 1),), BATCH),
    "ln_tail": ((("ln_tail", 1),), BATCH),
    "ln_cluster_wait": ((("ln_cluster", 1), ("ln_cluster_spin", -1)), BATCH),
    "ln_cluster_defer": ((("ln_cluster", 1), ("ln_cluster_spin", 0)), BATCH),
    "ln_row_1": ((("ln_row", 1),), BATCH),
    "ln_row_2": ((("ln_row", 2),), BATCH),
    "ln_row_3": ((("ln_row", 3),), BATCH),
    "ln_row_4": ((("ln_row", 4),), BATCH),
    "qkv_head_major": ((("qkv_head_major", 1),), BATCH),
    "qkv_chunks_2": ((("qkv_chunks", 2),), BATCH),
    "nsplit_2": ((("nsplit", 2),), BATCH),
    "nsplit_3": ((("nsplit", 3),), BATCH),
    "nsplit_4": ((("nsplit", 4),), BATCH),
    "patch_fold_0": ((("patch_fold", 0),), BATCH),
    "ragged_37_off": ((), 37),
}
# Settings whose scores existing tests hold bit-identical to the all-off run (test_gpu_ln_tail.py, test_gpu_qkv_layout.py,
# test_gpu_model.py's patch route) — and the two a column's / a sequence's independence makes so by construction: a column
# block of a GEMM (n-split) or a chunk of the batch (qkv_chunks) computes each output element with the same K-sum in the same
# order.  The fold, the cluster and the full-row tiles sum LayerNorm statistics in another order: close, not equal.
BIT_IDENTICAL = ("ln_tail", "qkv_head_major", "qkv_chunks_2", "nsplit_2", "nsplit_3", "nsplit_4", "patch_fold_0")
# Two arms launch, class for class, as many kernels as the all-off run: the fold puts one fold_stats launch where each LayerNorm
# launch was, and the cluster's defer form four clean-up launches where the cluster saved four LayerNorms.  Both sum the
# LayerNorm statistics in another order than the LayerNorm kernel, so there it is the scores that must differ from the
# all-off run's.  (Head-major qkv also keeps the ledger — the same kernels write and read h->qkv in another order — and
# keeps the bits: this test cannot see that switch engage.)
LEDGER_OF_OFF = ("ln_fold", "ln_cluster_defer")
# these need the per-XCD counters, which mcm_create allocates only on a device that deals workgroups to XCDs round-robin
NEEDS_XCD_ROUND_ROBIN = ("ln_tail", "ln_cluster_wait", "ln_cluster_defer")

# KERNEL_CLASSES: patchify gemm layernorm attention pool_project score embed gemm_qkv gemm_outproj gemm_fc1 gemm_fc2
EXPECTED_HARNESS = {
    "off": (0, 14, 6, 3, 1, 1, 0, 3, 2, 2, 2),
    "ln_fold": (0, 14, 6, 3, 1, 1, 0, 3, 2, 2, 2),
    "ln_tail": (0, 14, 2, 3, 1, 1, 0, 3, 2, 2, 2),
    "ln_cluster_wait": (0, 14, 2, 3, 1, 1, 0, 3, 2, 2, 2),
    "ln_cluster_defer": (0, 14, 6, 3, 1, 1, 0, 3, 2, 2, 2),
    "ln_row_1": (0, 14, 2, 3, 1, 1, 0, 3, 2, 2, 2),
    "ln_row_2": (0, 14, 2, 3, 1, 1, 0, 3, 2, 2, 2),
    "ln_row_3": (0, 14, 2, 3, 1, 1, 0, 3, 2, 2, 2),
    "ln_row_4": (0, 14, 2, 3, 1, 1, 0, 3, 2, 2, 2),
    "qkv_head_major": (0, 14, 6, 3, 1, 1, 0, 3, 2, 2, 2),
    "qkv_chunks_2": (0, 16, 6, 5, 1, 1, 0, 5, 2, 2, 2),
    "nsplit_2": (0, 16, 6, 3, 1, 1, 0, 3, 2, 4, 2),
    "nsplit_3": (0, 22, 6, 3, 1, 1, 0, 7, 2, 6, 2),
    "nsplit_4": (0, 20, 6, 3, 1, 1, 0, 3, 2, 8, 2),
    "patch_fold_0": (1, 14, 6, 3, 1, 1, 0, 3, 2, 2, 2),
    "ragged_37_off": (1, 14, 6, 3, 1, 1, 0, 3, 2, 2, 2),
}
EXPECTED_SHIPPED = {
    "score_images": (0, 14, 6, 3, 1, 1, 0, 3, 2, 2, 2),
    "score_images_x2": (1, 14, 6, 3, 1, 1, 0, 3, 2, 2, 2),
    "get_text_features_40": (0, 4, 2, 1, 1, 0, 1, 0, 0, 0, 0),
}


def _geo():
    return dataclasses.replace(geometry("ViT-B/16"), name="B16-3L", v_layers=3, t_layers=1)


def _net(harness):
    geo = _geo()
    return NativeCLIP(geo, synth_state_dict(geo, 0), device=0, precision="fp16", max_batch=BATCH, max_prompt_tokens=40 * 20,
                      harness=harness, weight_operands="single")


def _inputs(net):
    ids, _ = make_token_ids(40, seed=2)
    ids = torch.from_numpy(ids)
    g = torch.Generator(device="cuda").manual_seed(17)
    px = torch.randn((BATCH, 3, net.geo.image_size, net.geo.image_size), generator=g, device="cuda")
    return ids, px


def _launches(net):
    prof = net.profile_read()  # (one read: it also resets the counters)
    return tuple(prof[k]["launches"] for k in KERNEL_CLASSES)


def _set(lib, switches):
    for name, value in switches.items():
        assert getattr(lib, "mcm_debug_" + name)(value) == 0, name


def harness_rows():
    """{setting: (launches per KERNEL_CLASSES entry, scores)} of one harness handle"""
    net = _net(True)
    rows = {}
    try:
        ids, px = _inputs(net)
        txt = net.get_text_features(input_ids=ids, normalize=True)
        _set(net._lib, OFF)
        net.profile(True)
        net.profile_read()
        for name, (switches, batch) in SETTINGS.items():
            try:
                _set(net._lib, dict(switches))
                scores = net.score_images(px[:batch], txt, 1.0, "MCM").clone()
                rows[name] = (_launches(net), scores)
            finally:
                _set(net._lib, OFF)
    finally:
        _set(net._lib, OFF)
        net.close()
    return rows


def shipped_rows():
    """{call: launches per KERNEL_CLASSES entry} of one handle of the shipped library"""
    net = _net(False)
    rows = {}
    try:
        ids, px = _inputs(net)
        txt = net.get_text_features(input_ids=ids, normalize=True)
        net.profile(True)
        net.profile_read()
        net.score_images(px, txt, 1.0, "MCM")
        rows["score_images"] = _launches(net)
        net.score_images_x2(px, txt, 1.0, "MCM")
        rows["score_images_x2"] = _launches(net)
        net.get_text_features(input_ids=ids, normalize=True)
        rows["get_text_features_40"] = _launches(net)
    finally:
        net.close()
    return rows


def _need_256_cus():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the ledger is that of 256 CUs (the persistent kernels' grid and the size policy); this device reports {cus}")


@pytest.fixture(scope="module")
def rows():
    _need_256_cus()
    return harness_rows()


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_switch_engages(rows, setting):
    got, scores = rows[setting]
    off, off_scores = rows["off"]
    print(f"{setting}: " + " ".join(f"{k}={n}" for k, n in zip(KERNEL_CLASSES, got)))
    if setting in NEEDS_XCD_ROUND_ROBIN and all(rows[s][0] == off for s in NEEDS_XCD_ROUND_ROBIN):
        pytest.skip("ln_tail and ln_cluster launch what the all-off run launches: the device failed the XCD round-robin probe "
                    "of mcm_create, so the handle has no counters for them")
    assert torch.isfinite(scores).all()
    assert got == EXPECTED_HARNESS[setting]
    if setting in BIT_IDENTICAL:
        assert torch.equal(scores, off_scores)
    if setting == "ln_cluster_defer":  # test_gpu_ln_cluster.py: the defer form gives the waiting form's bits
        assert torch.equal(scores, rows["ln_cluster_wait"][1])
    if setting in LEDGER_OF_OFF:
        assert got == off and not torch.equal(scores, off_scores), "the switch did nothing"


def test_shipped_library_ledger():
    _need_256_cus()
    got = shipped_rows()
    for name, n in got.items():
        print(f"{name}: " + " ".join(f"{k}={v}" for k, v in zip(KERNEL_CLASSES, n)))
    assert got == EXPECTED_SHIPPED
