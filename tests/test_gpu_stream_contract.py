"""Every exported entry that takes a `stream`, held to the class tests/stream_contract.py gives it.

    replayable     one case per entry (REPLAY_CASES; a variant per pixel format, arm or `splits` where the entry has them): the
                   call is captured into a hipGraph on a side stream and replayed on new input values; every output is, bit for
                   bit, what the eager call writes (tests/gpu_scaffold.py replay_equals_eager).  Inside the capture a launch on the
                   null stream, a host synchronisation or an allocation raises; a launch on some other stream is missing from the
                   replay; a host value baked in shows as stale output.  The criterion is include/mcm.h's "same arguments, same
                   bits": no tolerance.  Accuracy against fp64 is the budget tests' job, not this module's.
    host_staged    cannot be captured.  ORDER_CASES holds them (and a handful of replayable entries) to eager stream order instead:
                   queued behind a few milliseconds of work and an in-place rewrite of their device inputs on the same side stream,
                   with no synchronisation in between, they give what the same call gives after a full synchronise.
    synchronising  mcm_measures and mcm_saturation_count say so and are tested where their results are.

The shapes are the smallest that still take every launch of an entry: the `tiny` geometry (17 tokens, proj_dim 64), 3 images on
handles of max_batch 8 (51 token rows: the pad rows up to 256 exist and are zeroed inside the graph), K = 7 prompts (the LDS
tail), banks of 301 rows cut in 3 (two launches, a short last range; splits = 0 once), top-3 with probabilities, operators at
M = 65, N = 208 and one K-step, LayerNorm at D = 128, attention at 50 tokens and causal at 7.  Calls go to the raw library with
preallocated buffers and the side stream's handle, so torch allocates nothing inside a capture.  Profiling stays off.

Importing this module touches no GPU: the CPU test of the contract table reads REPLAY_CASES and ORDER_CASES from it."""
import ctypes

import numpy as np
import pytest

from tests import gpu_scaffold as gs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P, B, K, NB = 64, 3, 7, 301   # proj_dim, images, prompts, bank rows
F32, U8 = 0, 1                # MCM_PIXELS_*
PREC = {"bf16": 0, "fp32": 1, "fp16": 2}
DT = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}

REPLAY_CASES = {}   # entry -> (builder, variants)
ORDER_CASES = {}    # entry -> builder


def replay_case(entry, *variants):
    def deco(fn):
        assert entry not in REPLAY_CASES
        REPLAY_CASES[entry] = (fn, variants or (None,))
        return fn
    return deco


def order_case(*entries):
    def deco(fn):
        for e in entries:
            assert e not in ORDER_CASES
            ORDER_CASES[e] = fn
        return fn
    return deco


class Case:
    """The buffers of one case: inputs with the rule that refreshes each, outputs, accumulators."""

    def __init__(self, seed=0, watch=None):
        """watch: an fp16 handle whose saturation count a replay must leave as the eager call does (what the pad rows that a ragged
        batch zeroes inside the graph decide: mcm_api.hip vision_front "Pad rows")."""
        self.g = torch.Generator(device="cuda").manual_seed(1000 + seed)
        self.inputs, self.fills, self.outputs, self.inout = [], [], [], []
        self.probe = (lambda: watch.saturation_count(reset=True)) if watch is not None else None

    def _input(self, t, fill):
        self.inputs.append(t)
        self.fills.append(lambda: fill(t))
        fill(t)
        return t

    def normal(self, *shape, dtype=torch.float32, scale=1.0):
        return self._input(torch.empty(shape, dtype=dtype, device="cuda"), lambda t: t.normal_(0.0, scale, generator=self.g))

    def unit(self, *shape):
        def fill(t):
            t.normal_(generator=self.g)
            t.div_(t.norm(dim=-1, keepdim=True))
        return self._input(torch.empty(shape, device="cuda"), fill)

    def u8(self, *shape):
        return self._input(torch.empty(shape, dtype=torch.uint8, device="cuda"), lambda t: t.random_(0, 256, generator=self.g))

    def ascending(self, n):
        return self._input(torch.empty(n, device="cuda"),
                           lambda t: t.copy_(torch.sort(torch.randn(n, generator=self.g, device="cuda"))[0]))

    def pixels(self, fmt, S):
        return self.u8(B, S, S, 3) if fmt == U8 else self.normal(B, 3, S, S)

    def out(self, *shape, dtype=torch.float32):
        t = torch.empty(shape, dtype=dtype, device="cuda")
        self.outputs.append(t)
        return t

    def acc(self, *shape, dtype=torch.float64, zero=False):
        """An accumulator: refresh() re-initialises it (to zero, or to new values)."""
        t = torch.zeros(shape, dtype=dtype, device="cuda")
        self.inout.append(t)
        self.fills.append((lambda: t.zero_()) if zero else (lambda: t.normal_(generator=self.g)))
        return t

    def scratch(self, nbytes):
        return torch.empty((int(nbytes) + 7) // 8, dtype=torch.int64, device="cuda")

    def refresh(self):
        for f in self.fills:
            f()

    def run(self, call):
        """call(stream pointer, outputs..., accumulators...) -> replay_equals_eager."""
        gs.replay_equals_eager(lambda s, bufs: call(s.cuda_stream, *[b.data_ptr() for b in bufs]),
                               self.inputs, self.outputs, self.refresh, inout=self.inout, probe=self.probe)


class Ctx:
    """The handles of the module, one per precision: `tiny`, max_batch 8, fp16 with the split-activation workspace."""

    def __init__(self, get):
        self._get = get

    def net(self, prec="fp16"):
        from mcm_amd import abi

        n = self._get(prec)
        abi.declare(n._lib, names=list(abi.EXTENSION_PROTOTYPES))
        return n

    @staticmethod
    def lib(net, entry, *args):
        rc = getattr(net._lib, entry)(net._h, *args)
        assert rc == 0, f"{entry} rc={rc}: {net._lib.mcm_last_error(net._h).decode()}"

    def need(self, net, entry, *args):
        n = ctypes.c_int64(-1)
        self.lib(net, entry, *args, ctypes.byref(n))
        return n.value


@pytest.fixture(scope="module")
def ctx():
    for get in gs.net_cache(lambda prec: gs.widened_net(precision=prec, max_batch=8)):
        yield Ctx(get)


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- the vision tower ---------------------------------------------------------------------------------------------------------------
@replay_case("mcm_encode_image")
def _(ctx, _v):
    net, c = ctx.net("fp32"), Case()
    px = c.pixels(F32, net.geo.image_size)
    c.out(B, P)
    c.run(lambda s, o: ctx.lib(net, "mcm_encode_image", ptr(px), B, o, s))


@replay_case("mcm_encode_image_raw")
def _(ctx, _v):
    net, c = ctx.net("bf16"), Case(1)
    px = c.pixels(F32, net.geo.image_size)
    c.out(B, P)
    c.run(lambda s, o: ctx.lib(net, "mcm_encode_image_raw", ptr(px), B, o, s))


@replay_case("mcm_encode_image_u8")
def _(ctx, _v):
    net = ctx.net()
    c = Case(2, watch=net)
    px = c.pixels(U8, net.geo.image_size)
    c.out(B, P)
    c.run(lambda s, o: ctx.lib(net, "mcm_encode_image_u8", ptr(px), B, o, s))


@replay_case("mcm_encode_image_ex", F32, U8)
def _(ctx, fmt):
    net = ctx.net()
    c = Case(3, watch=net)
    px = c.pixels(fmt, net.geo.image_size)
    c.out(B, P)
    c.run(lambda s, o: ctx.lib(net, "mcm_encode_image_ex", ptr(px), fmt, B, 1 - fmt, o, s))   # (normalised and raw, once each)


@replay_case("mcm_encode_image_x2", F32, U8)
def _(ctx, fmt):
    net = ctx.net()
    c = Case(4, watch=net)
    px = c.pixels(fmt, net.geo.image_size)
    c.out(B, P)
    c.run(lambda s, o: ctx.lib(net, "mcm_encode_image_x2", ptr(px), fmt, B, 1, o, s))


@replay_case("mcm_encode_image_local", F32, U8)
def _(ctx, fmt):
    net = ctx.net()
    c = Case(5, watch=net)
    px = c.pixels(fmt, net.geo.image_size)
    c.out(B, P), c.out(B, net.local_rows, P)
    c.run(lambda s, g, loc: ctx.lib(net, "mcm_encode_image_local", ptr(px), fmt, B, g, loc, s))


# ---- scores on features -------------------------------------------------------------------------------------------------------------
@replay_case("mcm_score_features", 0, 1, 2, 3, 4)
def _(ctx, kind):
    net, c = ctx.net(), Case(6)
    f, t = c.unit(B, P), c.unit(K, P)
    c.out(B)
    c.run(lambda s, o: ctx.lib(net, "mcm_score_features", ptr(f), B, ptr(t), K, 0.5, kind, o, s))


@replay_case("mcm_score_features_topk")
def _(ctx, _v):
    net, c = ctx.net(), Case(7)
    f, t = c.unit(B, P), c.unit(K, P)
    c.out(B), c.out(B, 3, dtype=torch.int32), c.out(B, 3)
    c.run(lambda s, o, idx, prob: ctx.lib(net, "mcm_score_features_topk", ptr(f), B, ptr(t), K, 0.5, 0, 3, o, idx, prob, s))


@replay_case("mcm_score_features_stream", 3, 0)
def _(ctx, splits):
    net, c = ctx.net(), Case(8)
    f, t = c.unit(B, P), c.unit(NB, P)
    work = c.scratch(ctx.need(net, "mcm_score_stream_workspace_bytes", B, NB, 3, splits))
    c.out(B), c.out(B, 5), c.out(B, 3, dtype=torch.int32), c.out(B, 3)
    c.run(lambda s, o, parts, idx, prob: ctx.lib(net, "mcm_score_features_stream", ptr(f), B, ptr(t), NB, 0.05, 3, 3, splits,
                                                 ptr(work), work.numel() * 8, o, parts, idx, prob, s))


@replay_case("mcm_knn_score_features", 3, 0)
def _(ctx, splits):
    net, c, k = ctx.net(), Case(9), 5
    f, bank = c.unit(B, P), c.unit(NB, P)
    work = c.scratch(ctx.need(net, "mcm_knn_workspace_bytes", B, NB, k, splits))
    c.out(B), c.out(B, k)
    c.run(lambda s, o, topv: ctx.lib(net, "mcm_knn_score_features", ptr(f), B, ptr(bank), NB, k, splits, ptr(work),
                                     work.numel() * 8, o, topv, s))


@replay_case("mcm_neglabel_score_features")
def _(ctx, _v):
    net, c, n_id, G, gsz = ctx.net(), Case(10), 101, 4, 50   # 101 + 4 * 50 = 301 rows in 3 ranges of 101, 101, 99
    f, bank = c.unit(B, P), c.unit(NB, P)
    work = c.scratch(ctx.need(net, "mcm_neglabel_workspace_bytes", B, n_id, G, gsz, 3))
    c.out(B), c.out(B, G)
    c.run(lambda s, o, grp: ctx.lib(net, "mcm_neglabel_score_features", ptr(f), B, ptr(bank), n_id, G, gsz, 0.05, 3, ptr(work),
                                    work.numel() * 8, o, grp, s))


@replay_case("mcm_vim_score_features")
def _(ctx, _v):
    net, c, n_id, R = ctx.net(), Case(11), 261, 40
    f, bank, off = c.unit(B, P), c.unit(NB, P), c.normal(R, dtype=torch.float64, scale=0.1)
    work = c.scratch(ctx.need(net, "mcm_vim_workspace_bytes", B, n_id, R, 3))
    c.out(B), c.out(B, 3)
    c.run(lambda s, o, parts: ctx.lib(net, "mcm_vim_score_features", ptr(f), B, ptr(bank), n_id, R, ptr(off), 0.05, 1.5, 3,
                                      ptr(work), work.numel() * 8, o, parts, s))


@replay_case("mcm_local_score_features")
def _(ctx, _v):
    net, c = ctx.net(), Case(12)
    R = net.local_rows
    loc, t = c.unit(B, R, P), c.unit(K, P)
    work = c.scratch(ctx.need(net, "mcm_local_workspace_bytes", B, R, K))
    c.out(B), c.out(B, R)
    c.run(lambda s, o, patch: ctx.lib(net, "mcm_local_score_features", ptr(loc), B, R, ptr(t), K, 0.5, ptr(work), work.numel() * 8,
                                      o, patch, s))


# ---- one batch of the hot loop ------------------------------------------------------------------------------------------------------
@replay_case("mcm_score")
def _(ctx, _v):
    net, c = ctx.net("bf16"), Case(13)
    px, t = c.pixels(F32, net.geo.image_size), c.unit(K, P)
    c.out(B)
    c.run(lambda s, o: ctx.lib(net, "mcm_score", ptr(px), B, ptr(t), K, 1.0, 0, o, s))


@replay_case("mcm_score_u8")
def _(ctx, _v):
    net = ctx.net()
    c = Case(14, watch=net)
    px, t = c.pixels(U8, net.geo.image_size), c.unit(K, P)
    c.out(B)
    c.run(lambda s, o: ctx.lib(net, "mcm_score_u8", ptr(px), B, ptr(t), K, 1.0, 2, o, s))


@replay_case("mcm_score_x2", F32, U8)
def _(ctx, fmt):
    net = ctx.net()
    c = Case(15, watch=net)
    px, t = c.pixels(fmt, net.geo.image_size), c.unit(K, P)
    c.out(B)
    c.run(lambda s, o: ctx.lib(net, "mcm_score_x2", ptr(px), fmt, B, ptr(t), K, 1.0, 0, o, s))


@replay_case("mcm_score_topk", (F32, 0), (U8, 0), (F32, 1), (U8, 1))
def _(ctx, v):
    fmt, x2 = v
    net = ctx.net()
    c = Case(16, watch=net)
    px, t = c.pixels(fmt, net.geo.image_size), c.unit(K, P)
    c.out(B), c.out(B, 3, dtype=torch.int32), c.out(B, 3)
    c.run(lambda s, o, idx, prob: ctx.lib(net, "mcm_score_topk", ptr(px), fmt, x2, B, ptr(t), K, 1.0, 0, 3, o, idx, prob, s))


@replay_case("mcm_score_glmcm", (F32, True), (U8, False))
def _(ctx, v):
    fmt, parts = v   # parts: the optional outputs given, or NULL (the handle's workspace then holds them)
    net = ctx.net()
    c = Case(17, watch=net)
    px, t = c.pixels(fmt, net.geo.image_size), c.unit(K, P)
    c.out(B)
    if parts:
        c.out(B), c.out(B), c.out(B, net.local_rows)
    c.run(lambda s, o, g=None, l=None, patch=None: ctx.lib(net, "mcm_score_glmcm", ptr(px), fmt, B, ptr(t), K, 1.0, 0.5, o, g, l,
                                                           patch, s))


# ---- banks, metrics, Mahalanobis ----------------------------------------------------------------------------------------------------
@replay_case("mcm_reduce_bank")
def _(ctx, _v):
    net, c, T = ctx.net(), Case(18), 3
    f = c.unit(K * T, P)
    c.out(K, P)
    c.run(lambda s, o: ctx.lib(net, "mcm_reduce_bank", ptr(f), K, T, o, s))


@replay_case("mcm_score_histogram")
def _(ctx, _v):
    net, c, n, nb = ctx.net(), Case(19), 1000, 16   # 1000 scores: four workgroups add into the counts
    x, e = c.normal(n), c.ascending(nb + 1)
    c.out(nb, dtype=torch.int64)
    c.run(lambda s, o: ctx.lib(net, "mcm_score_histogram", ptr(x), n, ptr(e), nb, o, s))


@replay_case("mcm_maha_prepare")
def _(ctx, _v):
    net, c, C = ctx.net(), Case(20), 5
    mu, prec = c.normal(C, P), c.normal(P, P)
    c.out(C, P, dtype=torch.float64), c.out(C, dtype=torch.float64)
    c.run(lambda s, w, k: ctx.lib(net, "mcm_maha_prepare", ptr(mu), ptr(prec), C, w, k, s))


@replay_case("mcm_maha_score_features")
def _(ctx, _v):
    net, c, C = ctx.net(), Case(21), 5
    f, prec = c.normal(B, P), c.normal(P, P)
    w, k = c.normal(C, P, dtype=torch.float64), c.normal(C, dtype=torch.float64)
    c.out(B)
    c.run(lambda s, o: ctx.lib(net, "mcm_maha_score_features", ptr(f), B, ptr(prec), ptr(w), ptr(k), C, o, s))


@replay_case("mcm_maha_fit_accumulate")
def _(ctx, _v):
    net, c = ctx.net(), Case(22)
    f, shift = c.normal(B, P), c.normal(P)
    c.acc(P, P, zero=True), c.acc(P, zero=True)   # refresh() re-zeroes gram and sum: the call accumulates
    c.run(lambda s, gram, tot: ctx.lib(net, "mcm_maha_fit_accumulate", ptr(f), B, ptr(shift), gram, tot, s))


# ---- operators: M = 65, N = 208, one K-step (128 bytes per row) -----------------------------------------------------------------------
M_, N_ = 65, 208


@replay_case("mcm_op_linear")
def _(ctx, _v):
    net, c, Kd = ctx.net(), Case(23), 64
    x, w, b = c.normal(M_, Kd, dtype=torch.float16), c.normal(N_, Kd, dtype=torch.float16, scale=0.1), c.normal(N_)
    c.out(M_, N_, dtype=torch.float16)
    c.run(lambda s, y: ctx.lib(net, "mcm_op_linear", PREC["fp16"], ptr(x), ptr(w), ptr(b), y, None, M_, N_, Kd, 0, s))


@replay_case("mcm_op_linear_ex", "bf16 erf GELU", "fp32 residual", "fp16 split weight")
def _(ctx, v):
    net, c = ctx.net(), Case(24)
    prec = v.split()[0]
    Kd = 32 if prec == "fp32" else 64
    x, b = c.normal(M_, Kd, dtype=DT[prec]), c.normal(N_)
    if v == "fp32 residual":   # epilogue 2: resid += acc + bias, in place
        w = c.normal(N_, Kd, scale=0.1)
        c.acc(M_, N_, dtype=torch.float32)
        c.run(lambda s, r: ctx.lib(net, "mcm_op_linear_ex", PREC[prec], ptr(x), ptr(w), ptr(b), None, r, M_, N_, Kd, 2, 0, s))
        return
    split = v == "fp16 split weight"
    w = c.normal(N_, 2 * Kd if split else Kd, dtype=DT[prec], scale=0.1)   # (any 16-bit image is a split image of some weight)
    c.out(M_, N_, dtype=DT[prec])
    epi, flags = (0, 1) if split else (1, 8)   # MCM_LINEAR_SPLIT_W; QuickGELU's slot with MCM_LINEAR_ACT_GELU
    c.run(lambda s, y: ctx.lib(net, "mcm_op_linear_ex", PREC[prec], ptr(x), ptr(w), ptr(b), y, None, M_, N_, Kd, epi, flags, s))


@replay_case("mcm_op_split_weight")
def _(ctx, _v):
    net, c, Kd = ctx.net(), Case(25), 64
    w = c.normal(N_, Kd)
    c.out(N_, 2 * Kd, dtype=torch.float16)
    c.run(lambda s, o: ctx.lib(net, "mcm_op_split_weight", PREC["fp16"], ptr(w), N_, Kd, o, s))


@replay_case("mcm_op_layernorm", "fp16", "fp32")
def _(ctx, prec):
    net, c, D = ctx.net(), Case(26), 128
    x, g, b = c.normal(M_, D), c.normal(D), c.normal(D)
    c.out(M_, D, dtype=DT[prec])
    c.run(lambda s, y: ctx.lib(net, "mcm_op_layernorm", PREC[prec], ptr(x), ptr(g), ptr(b), y, M_, D, 1e-5, int(prec == "fp32"), s))


@replay_case("mcm_op_layernorm_split")
def _(ctx, _v):
    net, c, D = ctx.net(), Case(27), 128
    x, g, b = c.normal(M_, D), c.normal(D), c.normal(D)
    c.out(M_, 2 * D, dtype=torch.float16)
    c.run(lambda s, y: ctx.lib(net, "mcm_op_layernorm_split", ptr(x), ptr(g), ptr(b), y, M_, D, 1e-5, s))


@replay_case("mcm_op_attention", ("fp16", 50, 0), ("bf16", 50, 0), ("fp32", 50, 0), ("fp32", 7, 1))
def _(ctx, v):
    prec, L, causal = v
    net, c, nseq, heads = ctx.net(), Case(28), 3, 2
    qkv = c.normal(nseq * L, 3 * heads * 64, dtype=DT[prec])
    c.out(nseq * L, heads * 64, dtype=DT[prec])
    c.run(lambda s, o: ctx.lib(net, "mcm_op_attention", PREC[prec], ptr(qkv), o, nseq, L, heads, causal, s))


@replay_case("mcm_op_attention_split")
def _(ctx, _v):
    net, c, nseq, L, heads = ctx.net(), Case(29), 3, 50, 2
    qkv = c.normal(nseq * L, 6 * heads * 64, dtype=torch.float16)
    c.out(nseq * L, 2 * heads * 64, dtype=torch.float16)
    c.run(lambda s, o: ctx.lib(net, "mcm_op_attention_split", ptr(qkv), o, nseq, L, heads, s))


def _replay_params():
    for entry, (_, variants) in REPLAY_CASES.items():
        for v in variants:
            tag = "-".join(str(x) for x in (v if isinstance(v, tuple) else (v,))).replace(" ", "_")
            yield pytest.param(entry, v, id=entry if v is None else f"{entry}-{tag}")


@pytest.mark.parametrize("entry, variant", list(_replay_params()))
def test_a_replay_gives_the_eager_bits(ctx, entry, variant):
    REPLAY_CASES[entry][0](ctx, variant)


# ---- the helper discriminates ---------------------------------------------------------------------------------------------------------
def test_the_replay_check_reports_work_on_another_stream():
    """A callable of torch operations only, half of whose output is computed on a third stream: that half ran at capture time and
    is in no replay, so replay_equals_eager must raise AssertionError.  (The same callable wholly on the capture stream passes.)"""
    other = torch.cuda.Stream()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(2, 4096, generator=g, device="cuda")

    def refresh():
        x.normal_(generator=g)

    def call(astray):
        def run(s, bufs):
            torch.mul(x[0], 2.0, out=bufs[0][0])
            with torch.cuda.stream(other if astray else s):
                torch.mul(x[1], 3.0, out=bufs[0][1])
        return run

    gs.replay_equals_eager(call(False), [x], [torch.empty_like(x)], refresh)
    with pytest.raises(AssertionError):
        gs.replay_equals_eager(call(True), [x], [torch.empty_like(x)], refresh)
    torch.cuda.synchronize()
    assert not gs.capture_invalidated


# ---- eager stream order ---------------------------------------------------------------------------------------------------------------
class Ordered:
    """One eager-ordering case: device inputs with an old and a new value each, outputs, and the call."""

    def __init__(self):
        self.inputs, self.outputs = [], []

    def rewritten(self, old, new):
        """A device input that holds `old` until the side stream rewrites it with `new` just before the call."""
        t = old.clone()
        self.inputs.append((t, old, new))
        return t

    def out(self, *shape, dtype=torch.float32):
        self.outputs.append(torch.empty(shape, dtype=dtype, device="cuda"))
        return self.outputs[-1]

    def run(self, call):
        """call(stream pointer) writes self.outputs.  First the reference: the new values in place, a full synchronise, the call,
        a full synchronise.  Then the old values and 0xFF outputs, and on a side stream with no synchronisation in between: a few
        milliseconds of matmuls, the rewrite of every device input, the call; side.synchronize() alone follows."""
        side = torch.cuda.Stream()
        a = torch.randn(4096, 4096, device="cuda")
        b, c = torch.empty_like(a), torch.empty_like(a)
        for t, _, new in self.inputs:
            t.copy_(new)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.matmul(a, a, out=b)   # (also the matmul's own first-call set-up, outside the timed part below)
            call(side.cuda_stream)
        torch.cuda.synchronize()
        want = [o.clone() for o in self.outputs]
        for t, old, _ in self.inputs:
            t.copy_(old)
        for o in self.outputs:
            gs.raw_bytes(o).fill_(255)
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(side):
                for _ in range(2):
                    torch.matmul(a, b, out=c)
                    torch.matmul(a, c, out=b)
                for t, _, new in self.inputs:
                    t.copy_(new, non_blocking=True)
                call(side.cuda_stream)
            side.synchronize()
            for i, (got, ref) in enumerate(zip(self.outputs, want)):
                assert torch.equal(gs.raw_bytes(got), gs.raw_bytes(ref)), f"output {i}: not what the call gives after a full synchronise"
        finally:
            torch.cuda.synchronize()


def _ids(n, seed):
    from mcm_amd.synth import make_token_ids

    ids, _ = make_token_ids(n, seed=seed, min_len=14, max_len=14)   # [n, 16]: 16 prompts per pass of 256 tokens
    return np.ascontiguousarray(ids, dtype=np.int32)


@order_case("mcm_encode_text", "mcm_encode_text_ex")
def _(ctx, entry):
    """40 prompts = three passes through the one pinned staging buffer, and a second call right behind the first."""
    net, o, n = ctx.net(), Ordered(), 40
    ids = [_ids(n, 3), _ids(n, 4)]
    outs = [o.out(n, P), o.out(n, P)]
    extra = (1,) if entry.endswith("_ex") else ()

    def call(s):
        for i, out in zip(ids, outs):
            ctx.lib(net, entry, i.ctypes.data, n, i.shape[1], *extra, ptr(out), s)
    o.run(call)


@order_case("mcm_encode_text_ctx")
def _(ctx, entry):
    net, o, n, n_ctx = ctx.net(), Ordered(), 40, 4
    ids = _ids(n, 5)
    slots = np.full_like(ids, -1)
    slots[:, 1:1 + n_ctx] = np.arange(n_ctx, dtype=np.int32)
    g = torch.Generator(device="cuda").manual_seed(6)
    new_old = [torch.randn(n, n_ctx, net.geo.t_width, generator=g, device="cuda") * 0.02 for _ in range(2)]
    ctx_dev, out = o.rewritten(*new_old), o.out(n, P)
    o.run(lambda s: ctx.lib(net, entry, ids.ctypes.data, slots.ctypes.data, n, ids.shape[1], ptr(ctx_dev), n_ctx, n, 1, ptr(out), s))


@order_case("mcm_resize_crop_u8")
def _(ctx, entry):
    """Five calls in a row: one more than the staging ring has slots, so the fifth waits for the first one's copy."""
    net, o = ctx.net(), Ordered()
    S, sizes = net.geo.image_size, [(97, 131), (64, 64), (200, 70)]
    g = torch.Generator(device="cuda").manual_seed(7)
    imgs = [o.rewritten(*[torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g, device="cuda") for _ in range(2)])
            for h, w in sizes]
    ptrs = (ctypes.c_void_p * B)(*[im.data_ptr() for im in imgs])
    hs, ws = (ctypes.c_int32 * B)(*[h for h, _ in sizes]), (ctypes.c_int32 * B)(*[w for _, w in sizes])
    outs = [o.out(B, S, S, 3, dtype=torch.uint8) for _ in range(5)]

    def call(s):
        for out in outs:
            ctx.lib(net, entry, ptrs, hs, ws, B, ptr(out), s)
    o.run(call)


@order_case("mcm_jpeg_reconstruct")
def _(ctx, entry):
    pytest.importorskip("PIL")
    import tempfile

    from PIL import Image

    from tests.test_jpeg_oracle import _photo, entropy_decode

    net, o = ctx.net(), Ordered()
    sizes = [(40, 56), (24, 88), (64, 64)]   # (h w 3 bytes are multiples of 16: the images sit back to back, every byte is written)
    bufs = []
    with tempfile.TemporaryDirectory() as d:
        for k in range(2):   # two batches of the same files' shapes and tables, different pictures: the same records, other coefficients
            paths = []
            for i, (h, w) in enumerate(sizes):
                paths.append(f"{d}/{k}_{i}.jpg")
                Image.fromarray(_photo(h, w, 10 * k + i)).save(paths[-1], quality=90, subsampling=i % 3)
            meta, quant, buf = entropy_decode(paths)
            assert all(m.status == 0 for m in meta)
            bufs.append((meta, quant, buf))
    (meta, quant, old), (meta1, quant1, new) = bufs
    assert old.size == new.size and bytes(meta) == bytes(meta1) and np.array_equal(quant, quant1)
    coef = o.rewritten(torch.from_numpy(old).cuda(), torch.from_numpy(new).cuda())
    offs, total = [], 0
    for h, w in sizes:
        offs.append(total)
        total += h * w * 3
    outs = [o.out(total, dtype=torch.uint8) for _ in range(5)]   # one more call than the staging ring has slots
    offs_c = (ctypes.c_int64 * B)(*offs)

    def call(s):
        for out in outs:
            ctx.lib(net, entry, ptr(coef), ctypes.addressof(meta), quant.ctypes.data, B, ptr(out), offs_c, s)
    o.run(call)


@order_case("mcm_encode_image_ex")
def _(ctx, entry):
    net, o, S = ctx.net(), Ordered(), ctx.net().geo.image_size
    g = torch.Generator(device="cuda").manual_seed(8)
    px, out = o.rewritten(*[torch.randn(B, 3, S, S, generator=g, device="cuda") for _ in range(2)]), o.out(B, P)
    o.run(lambda s: ctx.lib(net, entry, ptr(px), F32, B, 1, ptr(out), s))


@order_case("mcm_score_glmcm")
def _(ctx, entry):
    net, o, S = ctx.net(), Ordered(), ctx.net().geo.image_size
    g = torch.Generator(device="cuda").manual_seed(9)
    px = o.rewritten(*[torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=g, device="cuda") for _ in range(2)])
    t = torch.nn.functional.normalize(torch.randn(K, P, generator=g, device="cuda"), dim=-1)
    out = o.out(B)
    o.run(lambda s: ctx.lib(net, entry, ptr(px), U8, B, ptr(t), K, 1.0, 0.5, ptr(out), None, None, None, s))


@order_case("mcm_score_features_stream", "mcm_knn_score_features")
def _(ctx, entry):
    net, o = ctx.net(), Ordered()
    g = torch.Generator(device="cuda").manual_seed(10)
    unit = lambda *shape: torch.nn.functional.normalize(torch.randn(*shape, generator=g, device="cuda"), dim=-1)  # noqa: E731
    f, bank, out = o.rewritten(unit(B, P), unit(B, P)), o.rewritten(unit(NB, P), unit(NB, P)), o.out(B)
    if entry == "mcm_knn_score_features":
        work = torch.empty(ctx.need(net, "mcm_knn_workspace_bytes", B, NB, 5, 3) // 4, device="cuda")
        o.run(lambda s: ctx.lib(net, entry, ptr(f), B, ptr(bank), NB, 5, 3, ptr(work), work.numel() * 4, ptr(out), None, s))
    else:
        work = torch.empty(ctx.need(net, "mcm_score_stream_workspace_bytes", B, NB, 0, 3) // 8, dtype=torch.float64, device="cuda")
        o.run(lambda s: ctx.lib(net, entry, ptr(f), B, ptr(bank), NB, 0.05, 0, 0, 3, ptr(work), work.numel() * 8, ptr(out), None,
                                None, None, s))


@pytest.mark.parametrize("entry", list(ORDER_CASES))
def test_a_call_queued_behind_work_reads_what_its_stream_wrote(ctx, entry):
    """Eager stream order, the only handle on the entries that cannot be captured.  This test can miss a bug when the race goes the
    lucky way (a kernel that ran on the wrong stream after all the queued work had finished anyway); it cannot fail on correct
    code: everything is queued on one stream, and stream order is the contract."""
    ORDER_CASES[entry](ctx, entry)
