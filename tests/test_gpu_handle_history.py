"""A handle's results depend on the call's arguments only (include/mcm.h, Conventions): each compute entry of the catalogue
(tests/handle_history.py) returns the bits it returns as the first call on a fresh handle — after any other entry, at either
walk parity, over a workspace full of garbage, with the saturation watch off and with per-kernel profiling on — and the sticky
counters report only that call.  Bit equality throughout; no tolerance.

Handles: `tiny` at bf16, fp16 and fp32; `B16-2L` (768 wide: every dense GEMM takes the padded-row route, and at 197 tokens no
batch is a whole 256-row tile) at fp16 and bf16; max_batch 8, max_prompt_tokens 154; the harness library.  The state dict and the
inputs are built once per geometry, the pristine results once per (geometry, precision)."""
import collections

import numpy as np
import pytest

from tests import handle_history as hh

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = [("tiny", "bf16"), ("tiny", "fp16"), ("tiny", "fp32"), ("B16-2L", "fp16"), ("B16-2L", "bf16")]
_WORLD, _PRISTINE = {}, {}


def _world(geo_name):
    """(geometry, state dict, device inputs) of a geometry, built once."""
    from mcm_amd.config import geometry
    from mcm_amd.weights import synth_state_dict

    if geo_name not in _WORLD:
        geo = geometry(geo_name)
        _WORLD[geo_name] = (geo, synth_state_dict(geo, 0), hh.device_inputs(hh.make_inputs(geo)))
    return _WORLD[geo_name]


def _make(geo_name, prec):
    from mcm_amd.engine import NativeCLIP

    geo, sd, _ = _world(geo_name)
    return NativeCLIP(geo, sd, precision=prec, max_batch=hh.MAX_BATCH, max_prompt_tokens=hh.MAX_PROMPT_TOKENS, harness=True)


def _close(net):
    net.__dict__.pop("_history_scorer", None)   # (the captured graph of the graph_replay entry refers to the handle)
    net.close()


Result = collections.namedtuple("Result", "outs sat faults tensors")


def _call(net, entry, dev):
    """One call of a catalogue entry: its outputs on the host, the saturation counter read and reset, the fault word, and the
    device tensors as they were returned (not cloned)."""
    tensors = entry.run(net, dev)
    outs = hh.host(tensors)   # (the copies synchronise the stream)
    return Result(outs, net.saturation_count(reset=True), net.kernel_faults, tensors)


def _pristine(geo_name, prec):
    """{entry name: Result} with every entry the first compute call of a handle of its own (for graph_replay the capture is)."""
    key = (geo_name, prec)
    if key not in _PRISTINE:
        dev, res = _world(geo_name)[2], {}
        for entry in hh.catalogue(prec):
            net = _make(geo_name, prec)
            try:
                r = _call(net, entry, dev)
                res[entry.name] = r._replace(tensors=None)
            finally:
                _close(net)
        _PRISTINE[key] = res
    return _PRISTINE[key]


@pytest.fixture(scope="module")
def long_lived():
    """get(geometry, precision) -> the one long-lived handle of the case: the tests below run on it one after the other, so each
    also starts from whatever the one before it left behind."""
    nets = {}

    def get(geo_name, prec):
        if (geo_name, prec) not in nets:
            nets[geo_name, prec] = _make(geo_name, prec)
        return nets[geo_name, prec]

    yield get
    for n in nets.values():
        _close(n)


class Checker:
    """Runs entries on one handle and collects every departure from the pristine results."""

    def __init__(self, net, geo_name, prec, sat_on=True):
        self.net, self.dev, self.want = net, _world(geo_name)[2], _pristine(geo_name, prec)
        self.entries = {e.name: e for e in hh.catalogue(prec)}
        self.sat_on, self.missed, self.held, self.calls, self.pred = sat_on, [], [], 0, "(what the test before left)"

    def run(self, name, where=""):
        r, want = _call(self.net, self.entries[name], self.dev), self.want[name]
        self.calls += 1
        msg = hh.first_difference(name, self.pred, r.outs, want.outs, where)
        if msg:
            self.missed.append(msg)
        want_sat = want.sat if self.sat_on else 0
        if r.sat != want_sat or r.faults != 0:
            self.missed.append(f"{name} after {self.pred}{where}: saturation count {r.sat} (a fresh handle: {want_sat}), "
                               f"kernel faults {r.faults}")
        self.held.append((name, self.pred, where, r.tensors))
        self.pred = name

    def recheck_held(self):
        """The tensors the calls returned, read again now: one that aliased an internal buffer has changed since."""
        torch.cuda.synchronize()
        for name, pred, where, tensors in self.held:
            msg = hh.first_difference(name, pred, hh.host(tensors), self.want[name].outs, where + " (read again at the end)")
            if msg:
                self.missed.append(msg)
        self.held = []

    def done(self):
        assert not self.missed, f"{len(self.missed)} departures from the first-call bits:\n" + "\n".join(self.missed[:40])


def _line(geo_name, prec, entries, calls, fills, what):
    print(f"HISTORY {geo_name} {prec}: {entries} entries, {calls} calls, {fills} fills, all bit-equal [{what}]")


@pytest.mark.parametrize("geo_name,prec", CASES)
def test_pristine_results(geo_name, prec):
    """Every entry as the first compute call of a fresh handle: finite where the entry computes numbers, no fault, and a
    saturation count of 0 everywhere but at the saturating operator call.  What the tests below compare with."""
    res = _pristine(geo_name, prec)
    assert list(res) == [e.name for e in hh.catalogue(prec)]
    for name, r in res.items():
        assert r.faults == 0, name
        assert (r.sat >= 1) if name == "op_linear_saturating" else (r.sat == 0), (name, r.sat)
        for out, a in r.outs.items():
            if a.dtype.kind == "f":
                assert np.isfinite(a.astype(np.float32)).all(), (name, out)
    if prec == "fp16":   # the operator saturated as its own test says, and the split arm is not the fp16 arm's bits by accident
        y = res["op_linear_saturating"].outs["y"]
        assert y[3, 5] == 65504.0 and y[3, 6] == -65504.0
        assert not np.array_equal(res["image_x2_b3"].outs["feat"], res["image_f32_b3"].outs["feat"])
    _line(geo_name, prec, len(res), len(res), 0, "fresh handles")


@pytest.mark.parametrize("geo_name,prec", CASES)
def test_every_ordered_pair_at_both_parities(geo_name, prec, long_lived):
    """The schedule on one long-lived handle: every entry directly behind every entry, itself included; then once more with every
    position starting at the other walk parity.  mcm_op_layernorm, the one-launch call between the two rounds, does not move the
    parity (the operator-level entries launch with a fixed direction), which is asserted; the harness sets it."""
    net = long_lived(geo_name, prec)
    ck = Checker(net, geo_name, prec)
    walk = hh.schedule(list(ck.entries))
    parities = []
    for rnd in range(2):
        parities.append([])
        for name in walk:
            parities[rnd].append(hh.walk_parity(net))
            ck.run(name, where=f" (round {rnd}, parity {parities[rnd][-1]})")
        if rnd == 0:
            before = hh.walk_parity(net)
            ck.run("op_layernorm", where=" (between the rounds)")
            assert hh.walk_parity(net) == before
            hh.walk_parity(net, set_to=1 - parities[0][0])
    assert parities[1] == [1 - p for p in parities[0]]
    assert {0, 1} <= set(parities[0])   # (a vision forward makes an odd number of launches: one round already mixes them)
    for pred, name in hh.REGRESSIONS:   # the pairs that once differed, by name, at both parities
        if pred in ck.entries and name in ck.entries:
            for parity in (0, 1):
                ck.run(pred, where=" (regression pair, predecessor)")
                hh.walk_parity(net, set_to=parity)
                ck.run(name, where=f" (regression pair, parity {parity})")
    ck.recheck_held()
    ck.done()
    _line(geo_name, prec, len(ck.entries), ck.calls, 0, "every ordered pair, both parities")


@pytest.mark.parametrize("geo_name,prec", CASES)
def test_graph_replay_behind_operator_calls(geo_name, prec):
    """The pair that once differed (handle_history.REGRESSIONS), as it differed: a handle of its own whose first call is the
    capture, then rounds of mcm_op_layernorm and a replay on the default stream.  With the pad rows zeroed by hipMemsetAsync
    the replay of the 13th round counted 112 saturations on `tiny` at fp16 (none in eager calls, none on a side stream)."""
    net = _make(geo_name, prec)
    try:
        ck = Checker(net, geo_name, prec)
        ck.pred = "(a fresh handle)"
        ck.run("graph_replay", where=" (the capture)")
        for rnd in range(hh.REGRESSION_ROUNDS):
            for pred, name in hh.REGRESSIONS:
                ck.run(pred, where=f" (round {rnd})")
                ck.run(name, where=f" (round {rnd})")
        ck.recheck_held()
        ck.done()
    finally:
        _close(net)
    _line(geo_name, prec, len(hh.REGRESSIONS), ck.calls, 0, "the regression pair behind a capture")


@pytest.mark.parametrize("geo_name,prec", CASES)
def test_poisoned_workspace(geo_name, prec, long_lived):
    """Every entry at each parity directly behind a fill of the whole activation workspace, pad rows included: 0xFF bytes (NaN as
    fp32, fp16 and bf16) and 0x7B bytes (61 280 as fp16, finite and just under saturation; about 1.3e36 as bf16 and fp32 — a value
    the NaN-skipping maxima would not hide)."""
    net = long_lived(geo_name, prec)
    ck = Checker(net, geo_name, prec)
    fills = 0
    for byte in (0xFF, 0x7B):
        for parity in (0, 1):
            for name in ck.entries:
                hh.walk_parity(net, set_to=parity)
                hh.workspace_fill(net, byte)
                fills += 1
                ck.run(name, where=f" (workspace filled with 0x{byte:02X}, parity {parity})")
    ck.recheck_held()
    ck.done()
    _line(geo_name, prec, len(ck.entries), ck.calls, fills, "poisoned workspace")


@pytest.mark.parametrize("geo_name,prec", CASES)
def test_switches_do_not_change_the_bits(geo_name, prec, long_lived):
    """saturation_check(False) hands the kernels a null counter, profile(True) brackets every launch with events: the same bits,
    and no count with the watch off.  The graph entry stays in both runs: a replay launches what was captured (its counter pointer
    and no events), whatever the switches say now; its capture is made before profiling goes on, because a capture cannot hold the
    per-kernel events."""
    net = long_lived(geo_name, prec)
    plain = Checker(net, geo_name, prec)
    plain.run("graph_replay", where=" (capture before the switches)")
    plain.done()
    calls = plain.calls
    try:
        net.saturation_check(False)
        ck = Checker(net, geo_name, prec, sat_on=False)
        for name in ck.entries:
            ck.run(name, where=" (saturation watch off)")
        net.saturation_check(True)
        ck.sat_on = True
        ck.run("op_linear_saturating" if prec == "fp16" else "op_layernorm", where=" (saturation watch on again)")
        net.profile(True)
        for name in ck.entries:
            ck.run(name, where=" (profiling on)")
        prof = net.profile_read()
        assert prof["gemm"]["launches"] > 0 and prof["attention"]["launches"] > 0
    finally:
        net.saturation_check(True)
        net.profile(False)
        net.profile_read()
    for name in ck.entries:
        ck.run(name, where=" (switches back)")
    ck.recheck_held()
    ck.done()
    _line(geo_name, prec, len(ck.entries), calls + ck.calls, 0, "switches")


@pytest.mark.parametrize("geo_name,prec", CASES)
def test_positive_control_the_checker_sees_a_workspace_read(geo_name, prec, long_lived):
    """mcm_debug_vision_front(stage = 0) returns the residual rows behind the patch GEMM; its CLS rows are documented as whatever
    the workspace held.  Behind two different fills the checker must report a difference, on the CLS rows and only there: the fill
    reaches the buffers, and a workspace read does show in the comparison."""
    net = long_lived(geo_name, prec)
    dev = _world(geo_name)[2]
    B, ntok, D = 3, net.local_rows + 1, net.geo.v_width
    got = {}
    for byte in (0xFF, 0x7B):
        hh.workspace_fill(net, byte)
        got[byte] = hh.host(hh.control_vision_front(net, dev, B))
    assert net.saturation_count(reset=True) == 0 and net.kernel_faults == 0
    msg = hh.first_difference("control_vision_front", "workspace_fill(0x7B)", got[0x7B], got[0xFF])
    assert msg is not None and "'resid'" in msg and "flat index 0 (0, 0)" in msg and "0x7b7b7b7b" in msg and "0xffffffff" in msg, msg
    rows = np.unique(hh.differing(got[0x7B]["resid"], got[0xFF]["resid"]) // D)
    assert rows.tolist() == [b * ntok for b in range(B)]
    assert hh.differing(got[0x7B]["resid"], got[0xFF]["resid"]).size == B * D
    patch_rows = np.setdiff1d(np.arange(B * ntok), rows)
    assert np.isfinite(got[0xFF]["resid"][patch_rows]).all()
    # ... and the catalogue entry over the same pixels is unmoved by what the control left in the workspace
    ck = Checker(net, geo_name, prec)
    ck.pred = "control_vision_front"
    ck.run("image_f32_b3")
    ck.done()
    print(f"HISTORY-CONTROL {geo_name} {prec}: {msg}")
