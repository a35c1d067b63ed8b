"""What a handle's results may depend on: the call's arguments, and nothing the handle ran before.  This module holds the
pieces the tests of that property share (tests/test_handle_history.py on the CPU, tests/test_gpu_handle_history.py on the GPU):

    make_inputs(geo)          seeded host inputs, built once per geometry and shared by every handle
    catalogue(precision)      the named compute entries of a handle of that precision: Entry(name, run), run(net, dev) ->
                              {output name: device tensor}, every call made through NativeCLIP as its users make it.  Every
                              route that touches the shared activation workspace, the walk parity or a sticky word is in it
    schedule(names)           a fixed walk of len(names)^2 + 1 calls in which every ordered pair (a, b), a = b included, is adjacent
    REGRESSIONS               (predecessor, entry) pairs that once differed, run by name next to the schedule (REGRESSION_ROUNDS:
                              how often the one that needed a young handle is repeated behind a capture)
    first_difference(...)     the comparator: None, or a message naming the entry, its predecessor, the output and the first
                              differing index
    control_vision_front      the positive control, NOT a catalogue entry: mcm_debug_vision_front(stage = 0) hands out the residual
                              rows behind the patch GEMM, whose CLS rows are by its contract "whatever the workspace held" —
                              an entry that legitimately depends on history, and therefore what proves that the workspace fill
                              reaches the buffers and that the comparator sees a workspace read

Importing this module needs neither torch nor a GPU."""
import collections
import ctypes

import numpy as np

MAX_BATCH, MAX_PROMPT_TOKENS = 8, 154
BOS, EOS = 49406, 49407
Entry = collections.namedtuple("Entry", "name run")
# every route the catalogue has to name, by handle kind ("fp16": the routes only an fp16 handle has)
ROUTES = {
    "any": ["text_k1_s77", "text_k5_s77_three_passes", "text_k6_s31_ragged_pass", "text_ctx",
            "image_f32_b1_raw", "image_f32_b3", "image_u8_b3", "image_f32_max_batch", "image_f32_two_chunks",
            "score_u8_mcm", "score_u8_topk5", "score_u8_stream",
            "local_features_b3", "score_glmcm_b2",
            "graph_replay", "resize_crop_two_sizes", "op_layernorm"],
    "fp16": ["score_x2_b2", "image_x2_b3", "op_linear_saturating"],
}
# (predecessor, entry) pairs that differed when these tests first ran.
# (op_layernorm, graph_replay), fp16 handles, by the saturation count alone (7 ... 112 for a fresh handle's 0; the outputs held).
# Observed, `tiny`, a handle of its own, capture, then (op_layernorm, replay) rounds on the default stream, the workspace read
# back after every call: vision_front zeroed the pad rows of x, ln, att and the MLP hidden with four hipMemsetAsync; behind a
# replay rows 51 ... 255 of att, then of ln, held a 16-byte periodic non-zero pattern (up to 55 136 as fp16) although nothing but
# those memsets writes them; the next replay's fc1 read the ln rows, packed hidden rows 51 ... 255 up to 65 056, and counted.
# From the 2nd round in one run, at the 13th only in another; never in an eager call or a replay on a side stream.  Supposed:
# that the runtime's replayed memset nodes write that pattern — the same sequence counts 0 with one kernel (launch_zero_spans)
# in their place, which is the fix in the product.  test_graph_replay_behind_operator_calls is that sequence.
REGRESSIONS = [("op_layernorm", "graph_replay")]
REGRESSION_ROUNDS = 16   # (op_layernorm, graph_replay) rounds behind a capture: past the 13th, where the count appeared


def _prompts(rng, K, S):
    """[K,S] ids as a padded tokenizer batch: BOS, n tokens, EOS, EOS padding; the longest prompt fills the row."""
    ids = np.full((K, S), EOS, dtype=np.int64)
    for k in range(K):
        n = S - 2 if k == 0 else int(rng.integers(1, S - 1))
        ids[k, 0] = BOS
        ids[k, 1:1 + n] = rng.integers(1, BOS - 1, size=n)
    return ids


def make_inputs(geo, seed=11):
    """Host arrays only; the same bits on every run."""
    from mcm_amd.synth import make_pixels

    rng = np.random.Generator(np.random.Philox(key=seed))
    S, P = geo.image_size, geo.proj_dim
    inp = {"ids_k1": _prompts(rng, 1, 77), "ids_k5": _prompts(rng, 5, 77), "ids_s31": _prompts(rng, 6, 31),
           "ctx_ids": _prompts(rng, 3, 77)}
    slots = np.full((3, 77), -1, dtype=np.int64)
    slots[:, 1:5] = np.arange(4)
    inp["ctx_slots"] = slots
    inp["ctx"] = (rng.standard_normal((4, geo.t_width)) * 0.02).astype(np.float32)
    inp["px"] = make_pixels(MAX_BATCH + 1, S, 11, ood=False, seed=5)[0]
    inp["u8"] = rng.integers(0, 256, (3, S, S, 3), dtype=np.uint8)
    bank = rng.standard_normal((11, P))
    inp["bank"] = (bank / np.linalg.norm(bank, axis=1, keepdims=True)).astype(np.float32)
    inp["raw_a"] = rng.integers(0, 256, (S + 13, S + 40, 3), dtype=np.uint8)
    inp["raw_b"] = rng.integers(0, 256, (2 * S + 5, S + 1, 3), dtype=np.uint8)
    inp["ln_x"] = rng.standard_normal((70, 128)).astype(np.float32)
    inp["ln_g"] = (1.0 + 0.1 * rng.standard_normal(128)).astype(np.float32)
    inp["ln_b"] = (0.1 * rng.standard_normal(128)).astype(np.float32)
    # the operands of test_gpu_kernels.py::test_fp16_outputs_saturate_instead_of_overflowing: row 3 x column 5 = 768 000
    x = rng.standard_normal((70, 64)).astype(np.float16)
    w = (rng.standard_normal((128, 64)) * 0.1).astype(np.float16)
    x[3, :], w[5, :], w[6, :] = 200.0, 60.0, -60.0
    inp["sat_x"], inp["sat_w"], inp["sat_b"] = x, w, np.zeros(128, np.float32)
    return inp


def device_inputs(inp):
    """The arrays the entries hand over as device tensors; token ids and slots stay on the host, as the text entries take them."""
    import torch

    return {k: v if k.startswith(("ids_", "ctx_ids", "ctx_slots")) else torch.from_numpy(v).cuda() for k, v in inp.items()}


def bind(net):
    """Declares the harness entries of include/mcm_debug_workspace.h on the handle's library (the harness one), once."""
    from mcm_amd import abi

    if not getattr(net._lib, "_mcm_debug_workspace", False):
        abi.declare(net._lib, names=list(abi.EXTENSION_HARNESS_PROTOTYPES))
        net._lib._mcm_debug_workspace = True
    return net._lib


def workspace_fill(net, byte):
    from mcm_amd.engine import _stream_ptr

    net._check(bind(net).mcm_debug_workspace_fill(net._h, int(byte), _stream_ptr()))


def walk_parity(net, set_to=-1):
    """The walk parity the handle's next tower launch takes; `set_to` 0 / 1 sets it behind the read."""
    out = ctypes.c_int32(-1)
    net._check(bind(net).mcm_debug_walk_parity(net._h, int(set_to), ctypes.byref(out)))
    return int(out.value)


# ---- the entries ------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _graph(net, d):
    from mcm_amd.engine import GraphedScorer

    scorer = getattr(net, "_history_scorer", None)
    if scorer is None:   # captured once per handle; on a fresh handle the capture is the handle's first compute call
        scorer = net._history_scorer = GraphedScorer(net, 3, d["bank"], uint8=True)
    return {"scores": scorer(d["u8"])}


def _op_layernorm(net, d):
    import torch

    from mcm_amd.config import PREC_BF16, PREC_F16
    from mcm_amd.engine import _stream_ptr

    # the output in the handle's operand type, as the towers ask for it: on an fp16 handle the kernel gets the sticky counter
    dtype = {PREC_F16: torch.float16, PREC_BF16: torch.bfloat16}.get(net.precision, torch.float32)
    y = torch.zeros((70, 128), device="cuda", dtype=dtype)
    net._check(net._lib.mcm_op_layernorm(net._h, net.precision, _ptr(d["ln_x"]), _ptr(d["ln_g"]), _ptr(d["ln_b"]), _ptr(y),
                                         70, 128, 1e-5, 0, _stream_ptr()))
    return {"y": y}


def _op_linear_saturating(net, d):
    import torch

    from mcm_amd.config import PREC_F16
    from mcm_amd.engine import _stream_ptr

    y = torch.zeros((70, 128), device="cuda", dtype=torch.float16)
    net._check(net._lib.mcm_op_linear(net._h, PREC_F16, _ptr(d["sat_x"]), _ptr(d["sat_w"]), _ptr(d["sat_b"]), _ptr(y), None,
                                      70, 128, 64, 0, _stream_ptr()))
    return {"y": y}


def _named(names, values):
    return dict(zip(names, values))


_RUN = {
    "text_k1_s77": lambda n, d: {"text": n.get_text_features(d["ids_k1"])},
    # max_prompt_tokens = 154: two prompts per pass — passes of 2, 2 and 1 prompts, 154 rows (padded to 256) and a 77-row last one
    "text_k5_s77_three_passes": lambda n, d: {"text": n.get_text_features(d["ids_k5"], normalize=True)},
    # S = 31, the ragged band of test_gpu_text_lengths.py: four prompts per pass, then two
    "text_k6_s31_ragged_pass": lambda n, d: {"text": n.get_text_features(d["ids_s31"], normalize=True)},
    "text_ctx": lambda n, d: {"text": n.get_text_features_ctx(d["ctx_ids"], d["ctx_slots"], d["ctx"], normalize=True)},
    "image_f32_b1_raw": lambda n, d: {"feat": n.get_image_features(d["px"][:1], normalize=False)},
    "image_f32_b3": lambda n, d: {"feat": n.get_image_features(d["px"][:3], normalize=True)},
    "image_u8_b3": lambda n, d: {"feat": n.get_image_features(d["u8"], normalize=True)},
    "image_f32_max_batch": lambda n, d: {"feat": n.get_image_features(d["px"][:MAX_BATCH], normalize=True)},
    "image_f32_two_chunks": lambda n, d: {"feat": n.get_image_features(d["px"][:MAX_BATCH + 1], normalize=True)},
    "score_u8_mcm": lambda n, d: {"scores": n.score_images(d["u8"], d["bank"], 1.0, "MCM")},
    "score_u8_topk5": lambda n, d: _named(("scores", "idx", "prob"), n.score_images(d["u8"], d["bank"], 1.0, "MCM", topk=5)),
    "score_u8_stream": lambda n, d: {"scores": n.score_images(d["u8"], d["bank"], 1.0, "MCM", tail="stream")},
    "score_x2_b2": lambda n, d: {"scores": n.score_images_x2(d["px"][:2], d["bank"], 1.0, "MCM")},
    "image_x2_b3": lambda n, d: {"feat": n.get_image_features_x2(d["px"][:3], normalize=True)},
    "local_features_b3": lambda n, d: _named(("global", "local"), n.get_local_features(d["px"][:3])),
    "score_glmcm_b2": lambda n, d: _named(("scores", "global", "local", "patch"),
                                          n.score_images_glmcm(d["px"][:2], d["bank"], 1.0, 1.0, return_parts=True)),
    "graph_replay": _graph,
    "resize_crop_two_sizes": lambda n, d: {"pixels": n.resize_crop([d["raw_a"], d["raw_b"]])},
    # two operator-level calls on the caller's buffers: they leave the workspace and the walk parity alone (mcm_op_* launch with a
    # fixed direction) and only read the handle's switches; the second sets the sticky saturation counter
    "op_layernorm": _op_layernorm,
    "op_linear_saturating": _op_linear_saturating,
}


def catalogue(precision):
    """The entries of a handle of `precision` ("fp16", "bf16" or "fp32"), in a fixed order."""
    names = ROUTES["any"] + (ROUTES["fp16"] if precision == "fp16" else [])
    return [Entry(name, _RUN[name]) for name in names]


def control_vision_front(net, d, B=3):
    """The positive control (see the module's docstring): the residual rows [B ntok, D] behind the patch GEMM."""
    import torch

    from mcm_amd import abi
    from mcm_amd.engine import _stream_ptr

    ntok = net.local_rows + 1
    out = torch.zeros((B * ntok, net.geo.v_width), device="cuda", dtype=torch.float32)
    net._check(net._lib.mcm_debug_vision_front(net._h, _ptr(d["px"]), abi.DEFINES["MCM_PIXELS_F32_NCHW"], 0, B, 0, 0, _ptr(out),
                                               None, _stream_ptr()))
    return {"resid": out}


# ---- the schedule -----------------------------------------------------------------------------------------------------------
def schedule(names):
    """An Eulerian circuit of the complete directed graph on `names`, loops included (Hierholzer, neighbours in list order):
    len(names)^2 + 1 calls, every ordered pair adjacent exactly once, the same list on every run."""
    n = len(names)
    nxt, stack, walk = [0] * n, [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            nxt[v] += 1
            stack.append((v + nxt[v] - 1) % n)
        else:
            walk.append(stack.pop())
    return [names[i] for i in reversed(walk)]


# ---- the comparator ---------------------------------------------------------------------------------------------------------
def host(outs):
    """{name: device tensor} -> {name: host array} (a 16-bit float tensor as its uint16 patterns where numpy has no such type)."""
    import torch

    return {k: (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy() for k, t in outs.items()}


def _patterns(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


def differing(got, want):
    """Flat indices at which two host arrays of one shape and dtype hold different bits."""
    return np.flatnonzero(_patterns(got).ravel() != _patterns(want).ravel())


def first_difference(entry, predecessor, got, want, where=""):
    """None where the outputs `got` hold the bits of `want` under every name; else one line: the entry, the call before it,
    the first output that differs and its first differing index."""
    if sorted(got) != sorted(want):
        return f"{entry} after {predecessor}{where}: outputs {sorted(got)}, expected {sorted(want)}"
    for name in want:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"{entry} after {predecessor}{where}: output {name!r} is {g.dtype}{list(g.shape)}, expected {w.dtype}{list(w.shape)}"
        bad = differing(g, w)
        if bad.size:
            i = int(bad[0])
            idx = tuple(int(v) for v in np.unravel_index(i, w.shape)) if w.ndim else ()
            return (f"{entry} after {predecessor}{where}: output {name!r} differs at {bad.size} of {w.size} elements, first at flat "
                    f"index {i} {idx}: got {g.ravel()[i]!r} (0x{int(_patterns(g).ravel()[i]):x}), expected {w.ravel()[i]!r} "
                    f"(0x{int(_patterns(w).ravel()[i]):x})")
    return None
