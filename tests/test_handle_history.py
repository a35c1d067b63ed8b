"""The pieces of the handle-history tests that need no GPU (tests/handle_history.py): the schedule covers every ordered pair and
never changes, the catalogue names every route for the handle kind it is given, the comparator says what differed and where, and
the extension reader of mcm_amd/abi.py takes an #ifdef MCM_HARNESS block."""
import collections
import ctypes
import os

import numpy as np
import pytest

from tests import handle_history as hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_the_schedule_covers_every_ordered_pair_and_is_fixed(precision):
    names = [e.name for e in hh.catalogue(precision)]
    n = len(names)
    walk = hh.schedule(names)
    assert len(walk) == n * n + 1 and walk[0] == walk[-1]
    pairs = collections.Counter(zip(walk, walk[1:]))
    assert set(pairs) == {(a, b) for a in names for b in names} and set(pairs.values()) == {1}
    assert walk == hh.schedule(list(names))                       # the same list on every run
    assert hh.schedule(["a", "b"]) == ["a", "a", "b", "b", "a"]   # ... written out for the smallest case
    assert hh.schedule(["a"]) == ["a", "a"]
    for pair in hh.REGRESSIONS:
        assert set(pair) <= set(hh._RUN), pair


def test_the_catalogue_names_every_route_for_its_handle_kind():
    any_, fp16 = hh.ROUTES["any"], hh.ROUTES["fp16"]
    assert [e.name for e in hh.catalogue("fp16")] == any_ + fp16
    for precision in ("bf16", "fp32"):   # the split-activation arm and the saturation watch exist on fp16 handles only
        assert [e.name for e in hh.catalogue(precision)] == any_
    assert len(set(any_ + fp16)) == len(any_ + fp16) and set(any_ + fp16) == set(hh._RUN)
    assert all(callable(e.run) for e in hh.catalogue("fp16"))
    # every kind of route the property is about has an entry: both text entries and the pass shapes, every pixel form and batch
    # class, the three fused tails, the split arm, the local pass, a captured graph, a staging ring, the two operator calls
    for word in ("text_k1", "three_passes", "ragged_pass", "text_ctx", "b1_raw", "f32_b3", "u8_b3", "max_batch", "two_chunks",
                 "score_u8_mcm", "topk5", "stream", "score_x2", "image_x2", "local_features", "glmcm", "graph_replay",
                 "resize_crop", "op_layernorm", "op_linear_saturating"):
        assert sum(word in name for name in any_ + fp16) == 1, word
    assert "control_vision_front" not in hh._RUN and callable(hh.control_vision_front)   # the control is no catalogue entry


def test_the_inputs_are_the_same_bits_on_every_run():
    from mcm_amd.config import geometry

    a, b = hh.make_inputs(geometry("tiny")), hh.make_inputs(geometry("tiny"))
    assert sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)
    assert a["ids_k5"].shape == (5, 77) and a["ids_s31"].shape == (6, 31) and a["px"].shape[0] == hh.MAX_BATCH + 1
    assert hh.MAX_PROMPT_TOKENS // 77 == 2 and hh.MAX_PROMPT_TOKENS // 31 == 4            # three passes; four prompts, then two
    for ids in (a["ids_k1"], a["ids_k5"], a["ids_s31"], a["ctx_ids"]):
        assert ids.min() >= 0 and ids.max() == hh.EOS and (ids[:, 0] == hh.BOS).all()
    assert a["ctx_slots"].max() == a["ctx"].shape[0] - 1 and a["ctx_slots"].min() == -1
    assert a["raw_a"].shape != a["raw_b"].shape and min(a["raw_a"].shape[:2] + a["raw_b"].shape[:2]) >= 64


def test_the_comparator_names_entry_predecessor_output_and_first_index():
    want = {"scores": np.arange(6, dtype=np.float32).reshape(2, 3), "idx": np.arange(4, dtype=np.int32)}
    same = {k: v.copy() for k, v in want.items()}
    assert hh.first_difference("b", "a", same, want) is None
    same["scores"][0, 0] = -0.0          # +0 and -0 are different bits
    msg = hh.first_difference("b", "a", same, want)
    assert "b after a" in msg and "'scores'" in msg and "flat index 0 (0, 0)" in msg and "0x80000000" in msg and "1 of 6" in msg
    nan = {"scores": np.full((2, 3), np.nan, np.float32), "idx": want["idx"]}
    assert hh.first_difference("b", "a", nan, {k: v.copy() for k, v in nan.items()}) is None   # a NaN equals its own bits
    other = {k: v.copy() for k, v in want.items()}
    other["scores"][1, 1] += 1
    other["scores"][1, 2] += 1
    other["idx"][3] = 9
    msg = hh.first_difference("entry", "pred", other, want, where=" (second parity)")
    assert "entry after pred (second parity)" in msg and "'scores'" in msg and "flat index 4 (1, 1)" in msg and "2 of 6" in msg
    assert list(hh.differing(other["scores"], want["scores"])) == [4, 5]
    half = {"y": np.array([1.0, 2.0], np.float16)}
    msg = hh.first_difference("e", "p", {"y": np.array([1.0, 2.5], np.float16)}, half)
    assert "flat index 1 (1,)" in msg and "0x4100" in msg and "0x4000" in msg
    assert "expected float32[2, 3]" in hh.first_difference("e", "p", {"scores": want["scores"][:1], "idx": want["idx"]}, want)
    assert "outputs ['idx']" in hh.first_difference("e", "p", {"idx": want["idx"]}, want)


EXTENSION = """/* an extension header as include/mcm_debug_workspace.h is written */
#ifndef MCM_X_H
#define MCM_X_H
#include "mcm.h"
#ifdef __cplusplus
extern "C" {
#endif
int mcm_more(const mcm_handle* h, int64_t* out);
#ifdef MCM_HARNESS
int mcm_debug_more(mcm_handle* h, int32_t byte, void* stream);
#endif
%s
#ifdef __cplusplus
}
#endif
#endif
"""


def test_the_extension_reader_takes_a_harness_block_and_refuses_the_rest(tmp_path):
    from mcm_amd import abi

    c = ctypes
    path = tmp_path / "mcm_x.h"
    path.write_text(EXTENSION % "")
    ext = abi.read_extension(str(path))
    assert ext.prototypes == {"mcm_more": (c.c_int, [c.c_void_p, c.c_void_p])}
    assert ext.harness_prototypes == {"mcm_debug_more": (c.c_int, [c.c_void_p, c.c_int32, c.c_void_p])}
    with pytest.raises(ValueError, match=r"mcm_x.h.*declared before.*mcm_more"):
        abi.read_extension(str(path), taken=["mcm_more"])
    with pytest.raises(ValueError, match=r"declared before.*mcm_debug_more"):
        abi.read_extension(str(path), taken=["mcm_debug_more"])
    path.write_text(EXTENSION % "#define MCM_NEW 3")
    with pytest.raises(ValueError, match="new entries and nothing else"):
        abi.read_extension(str(path))
    path.write_text(EXTENSION % "typedef struct mcm_s { int32_t a; } mcm_s;")
    with pytest.raises(ValueError, match="new entries and nothing else"):
        abi.read_extension(str(path))


def test_the_workspace_entries_are_harness_only_and_declared_apart():
    from mcm_amd import abi
    from mcm_amd.engine import HARNESS_LIB_PATH, LIB_PATH

    c = ctypes
    assert abi.EXTENSION_HARNESS_PROTOTYPES == {
        "mcm_debug_workspace_fill": (c.c_int, [c.c_void_p, c.c_int32, c.c_void_p]),
        "mcm_debug_walk_parity": (c.c_int, [c.c_void_p, c.c_int32, c.c_void_p])}
    for table in (abi.PROTOTYPES, abi.HARNESS_PROTOTYPES, abi.EXTENSION_PROTOTYPES):   # the frozen tables do not know them
        assert not set(table) & set(abi.EXTENSION_HARNESS_PROTOTYPES)
    assert sorted(abi.EXTENSION_PROTOTYPES) == ["mcm_score_features_stream", "mcm_score_stream_workspace_bytes"]
    if not os.path.exists(LIB_PATH) or not os.path.exists(HARNESS_LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib, hlib = c.CDLL(LIB_PATH), c.CDLL(HARNESS_LIB_PATH)
    for name in abi.EXTENSION_HARNESS_PROTOTYPES:
        assert not hasattr(lib, name), f"{name} must not be exported by libmcm_hip.so"
    abi.declare(hlib, names=list(abi.EXTENSION_HARNESS_PROTOTYPES))
    # refused before anything touches a device: a NULL handle
    assert hlib.mcm_debug_workspace_fill(None, 0xFF, None) == abi.DEFINES["MCM_EINVAL"]
    assert hlib.mcm_debug_walk_parity(None, -1, None) == abi.DEFINES["MCM_EINVAL"]
