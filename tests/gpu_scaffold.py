"""What the GPU test modules share: the tiny geometry widened to a proj_dim and the cache of such handles, host -> device and
bit-view helpers, and the reporter of the fp64 error budgets.  A plain module: the fixtures stay in the test modules, under
their own names, and delegate here.  torch is imported where it is used, so importing this module needs no GPU."""
import ctypes
import dataclasses

import numpy as np
import pytest

from tests import error_budget as eb


def widened_net(P=None, geo="tiny", seed=0, precision="fp16", max_batch=8, max_prompt_tokens=256, **kw):
    """A NativeCLIP of the `geo` geometry with seeded weights, widened to proj_dim = P where P is given and differs."""
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry(geo)
    if P is not None and P != geo.proj_dim:
        geo = dataclasses.replace(geo, name=f"{geo.name}-P{P}", proj_dim=P)
    return NativeCLIP(geo, synth_state_dict(geo, seed), precision=precision, max_batch=max_batch,
                      max_prompt_tokens=max_prompt_tokens, **kw)


def net_cache(make=widened_net):
    """The body of a module-scoped fixture: yields get(key) -> make(key), one handle per key, all closed at teardown."""
    nets = {}

    def get(key):
        if key not in nets:
            nets[key] = make(key)
        return nets[key]

    yield get
    for n in nets.values():
        n.close()


def dev(a):
    """A host array as a contiguous fp32 device tensor."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    """The int32 view of a host array of 32-bit numbers."""
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b, rows=slice(None), keys=()):
    """Whether two dicts of host arrays hold the same bits under every key, in `rows`."""
    return all(np.array_equal(bits(a[k][rows]), bits(b[k][rows])) for k in keys)


def raw_bytes(t):
    """A contiguous device tensor as its bytes."""
    import torch

    return t.reshape(-1).view(torch.uint8)


def holds_all_ones(t):
    """Whether some element of `t` is the all-ones bit pattern (what a 0xFF fill leaves: a NaN in every float format, -1 as an integer)."""
    import torch

    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return bool((t.reshape(-1).view(view) == (255 if t.element_size() == 1 else -1)).any())


capture_invalidated = False   # a capture raised in this process: replay_equals_eager starts no further one


def replay_equals_eager(call, inputs, outputs, refresh, inout=(), rounds=2, probe=None):
    """Hold `call` to the stream contract of a `replayable` entry (tests/stream_contract.py): captured once into a hipGraph, a replay
    on new input values writes the bits the eager call writes.

    call(stream, bufs)  makes the call(s) on `stream` (a torch.cuda.Stream) with preallocated buffers only: it reads `inputs`, writes
                        bufs[:len(outputs)] and updates bufs[len(outputs):] in place.  It is run four times or more: a warm-up, the
                        capture (both on outputs + inout themselves) and an eager call per round on twins of them.
    inputs              the device tensors it reads; refresh() rewrites every one in place with new values (checked: a replay that
                        baked an input's values in would otherwise pass)
    outputs             the device tensors it writes whole: filled with 0xFF bytes before each replay and each eager call
    inout               the device tensors it accumulates into: refresh() re-initialises them, and the eager call starts from a copy
                        of what the replay started from
    probe               optional: probe() reads (and resets) host-visible state of the handle outside any capture, a sticky counter
                        for instance; what it returns behind the replay must equal what it returns behind the eager call

    A fresh side stream; one warm-up call on it with the final arguments (the first launch of a kernel raises its LDS limit);
    torch.cuda.graph(graph, stream=side) in the default, global, capture-error mode — there a launch on the legacy null stream, a
    host synchronisation or an allocation raises —; then `rounds` times: refresh, 0xFF, replay, eager, and the assertions: every
    buffer equal bit for bit (torch.equal on the bytes) and no all-ones element left in an output.  Work that `call` put on
    another stream ran at capture time and is in no replay: its output is stale, or still 0xFF.  Bit equality is the header's
    "same arguments, same bits"; there is no tolerance.
    After a capture that raised, this and every later call fails at once: the process starts no further capture."""
    import torch

    global capture_invalidated
    if capture_invalidated:
        pytest.fail("an earlier capture was invalidated: no further capture is started in this process")
    bufs = list(outputs) + list(inout)
    twins = [torch.empty_like(b) for b in bufs]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call(side, bufs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=side):
            call(side, bufs)
    except BaseException:
        capture_invalidated = True
        raise
    torch.cuda.synchronize()
    for rnd in range(rounds):
        before = [t.clone() for t in inputs]
        refresh()
        torch.cuda.synchronize()
        for i, (t, old) in enumerate(zip(inputs, before)):
            assert not torch.equal(raw_bytes(t), raw_bytes(old)), f"round {rnd}: refresh() left input {i} as it was"
        start = [t.clone() for t in inout]
        for t in list(outputs) + twins[:len(outputs)]:
            raw_bytes(t).fill_(255)
        for t, s0 in zip(twins[len(outputs):], start):
            t.copy_(s0)
        torch.cuda.synchronize()
        if probe:
            probe()
        with torch.cuda.stream(side):
            graph.replay()
        torch.cuda.synchronize()
        seen = probe() if probe else None
        with torch.cuda.stream(side):
            call(side, twins)
        torch.cuda.synchronize()
        if probe:
            after = probe()
            assert seen == after, f"round {rnd}: the handle's state behind the replay is {seen!r}, behind the eager call {after!r}"
        for i, (got, want) in enumerate(zip(bufs, twins)):
            what = f"round {rnd}: " + (f"output {i}" if i < len(outputs) else f"accumulator {i - len(outputs)}")
            if i < len(outputs):
                assert not holds_all_ones(want), f"{what}: the eager call left 0xFF elements"
                assert not holds_all_ones(got), f"{what}: the replay left 0xFF elements (work that is not in the graph)"
            assert torch.equal(raw_bytes(got), raw_bytes(want)), f"{what}: the replay's bits are not the eager call's"


def check_budget(what, prec, got, ref, bud, where="", finite_budget=False):
    """Print "BUDGET <what> <prec> <worst ratio> <where>", fail with the worst element where |got - ref| exceeds its budget, and
    return the ratio.  `finite_budget`: also require every budget to be finite."""
    if finite_budget:
        assert np.isfinite(bud).all(), f"{what} {prec} {where}: a non-finite budget"
    r, i = eb.worst(got, ref, bud)
    print(f"BUDGET {what} {prec} {r:.3f} {where}")
    if r > 1.0:
        idx = np.unravel_index(i, np.shape(ref))
        pytest.fail(f"{what} {prec} {where}: max|got - ref| / budget = {r:.3g} at {idx}: got "
                    f"{np.asarray(got).flat[i]!r} ref {ref.flat[i]!r} budget {bud.flat[i]:.3g}")
    return r
