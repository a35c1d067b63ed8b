"""The refusals of the bank-streamed scores and of the entries that share their argument checks, frozen.

tests/golden/refusals.json holds a table of bad-argument calls and what each gave when it was recorded:

    c_calls   an entry of the C ABI, the arguments that differ from the good call below, and (rc, mcm_last_error).  The
              *_workspace_bytes entries record rc alone: they set no message.  The table has every entry with a temperature
              or a pixel_format check, and both entries of k-NN, NegLabel, ViM, the GL-MCM local score and the streamed tail.
    py_calls  a NativeCLIP method, the keyword arguments that differ, and the exception: its class, and whether its message
              names each argument the call made bad ("T=", "splits=", ...).  A call with `stub_rc` runs with the score's
              *_workspace_bytes entry replaced by one that returns that code: a failure that is no refusal of the arguments.

The test runs the table and asserts the same results, and that no call wrote to an output or a workspace.  The golden was
recorded by `python -m tests.test_gpu_refusals_frozen --record` at the commit before the five scores' refusal paths became
one, and is the same after it with one marked exception ("aligned"): a code other than MCM_EINVAL from the k-NN entries was
reported as a ValueError about the arguments and is a RuntimeError now, as with the other four scores."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import gpu_scaffold as gs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals.json")
P, B, N = 64, 5, 300
SENTINEL = -2.5
# the good call of every entry, in the order of its prototype: "@name" is a buffer below, "@name+n" n bytes into it
I64 = "@need"
C_ENTRIES = {
    "mcm_knn_workspace_bytes": dict(h="@h", B=B, N=N, k=3, splits=2, bytes_out=I64),
    "mcm_knn_score_features": dict(h="@h", feats="@feat", B=B, bank="@bank", N=N, k=3, splits=2, work="@work", work_bytes="@wb",
                                   scores="@out", topv="@aux", stream="@stream"),
    "mcm_neglabel_workspace_bytes": dict(h="@h", B=B, K=100, G=4, gs=50, splits=2, bytes_out=I64),
    "mcm_neglabel_score_features": dict(h="@h", feats="@feat", B=B, bank="@bank", K=100, G=4, gs=50, T=0.01, splits=2,
                                        work="@work", work_bytes="@wb", scores="@out", group="@aux", stream="@stream"),
    "mcm_vim_workspace_bytes": dict(h="@h", B=B, K=260, R=40, splits=2, bytes_out=I64),
    "mcm_vim_score_features": dict(h="@h", feats="@feat", B=B, bank="@bank", K=260, R=40, off="null", T=0.01, alpha=1.0, splits=2,
                                   work="@work", work_bytes="@wb", scores="@out", parts="@aux", stream="@stream"),
    "mcm_score_stream_workspace_bytes": dict(h="@h", B=B, K=N, topk=0, splits=2, bytes_out=I64),
    "mcm_score_features_stream": dict(h="@h", img="@feat", B=B, text="@bank", K=N, T=0.01, kind=0, topk=0, splits=2, work="@work",
                                      work_bytes="@wb", scores="@out", parts="@aux", idx="@idx", prob="@aux2", stream="@stream"),
    "mcm_local_workspace_bytes": dict(h="@h", B=B, R="@R", K=N, bytes_out=I64),
    "mcm_local_score_features": dict(h="@h", local="@local", B=B, R="@R", text="@bank", K=N, T=1.0, work="@work", work_bytes="@wb",
                                     scores="@out", patch="@aux", stream="@stream"),
    "mcm_encode_image_ex": dict(h="@h", pixels="@px", pixel_format=0, B=B, normalize=1, out="@aux", stream="@stream"),
    "mcm_encode_image_x2": dict(h="@h", pixels="@px", pixel_format=0, B=B, normalize=1, out="@aux", stream="@stream"),
    "mcm_encode_image_local": dict(h="@h", pixels="@px", pixel_format=0, B=B, glob="@aux", local="@local_out", stream="@stream"),
    "mcm_score_topk": dict(h="@h", pixels="@px", pixel_format=0, x2=0, B=B, text="@bank", K=N, T=1.0, kind=0, topk=3, scores="@out",
                           idx="@idx", prob="@aux", stream="@stream"),
    "mcm_score_glmcm": dict(h="@h", pixels="@px", pixel_format=0, B=B, text="@bank", K=N, T=1.0, lam=1.0, scores="@out",
                            gscores="@aux", lscores="@aux2", patch="@local_out", stream="@stream"),
    "mcm_debug_vision_front": dict(h="@hh", pixels="@px", pixel_format=0, x2=0, B=B, stage=0, poison=0, resid="@aux", ln="@aux2",
                                   stream="@stream"),
}
# the good Python calls: (method, positional operands, keywords)
PY_METHODS = {
    "knn_scores": (("@feat", "@bank"), dict(k=3, splits=0)),
    "neglabel_scores": (("@feat", "@bank"), dict(n_id=100, groups=4, group_size=50, T=0.01, splits=0)),
    "vim_scores": (("@feat", "@bank"), dict(n_id=260, T=0.01, alpha=1.0, splits=0)),
    "local_scores": (("@local", "@bank"), dict(T=1.0)),
    "score_features": (("@feat", "@bank"), dict(T=0.01, tail="stream", topk=0, splits=0)),
}
PY_WORKSPACE_ENTRY = {"knn_scores": "mcm_knn_workspace_bytes", "neglabel_scores": "mcm_neglabel_workspace_bytes",
                      "vim_scores": "mcm_vim_workspace_bytes", "local_scores": "mcm_local_workspace_bytes",
                      "score_features": "mcm_score_stream_workspace_bytes"}

BAD_T = [0.0, -0.01, "nan", "inf"]


def _table():
    """The bad calls that record mode runs (the test itself runs the golden's copy)."""
    c = []

    def add(entry, **sets):
        for name, values in sets.items():
            c.extend({"entry": entry, "set": {name: v}} for v in (values if isinstance(values, list) else [values]))

    add("mcm_knn_workspace_bytes", B=0, N=0, k=[0, 1025], splits=[-1, 33], bytes_out="null")
    add("mcm_knn_score_features", feats=["null", "@feat+4"], bank="null", work="null", scores="null", B=0, N=0, k=[0, 1025],
        splits=[-1, 33], work_bytes=3)
    add("mcm_neglabel_workspace_bytes", B=0, K=0, G=[0, 1025], gs=0, splits=33)
    add("mcm_neglabel_score_features", T=BAD_T, G=1025, splits=33, B=0, work_bytes=3, bank="@bank+8")
    add("mcm_vim_workspace_bytes", B=0, K=0, R=0, splits=33)
    add("mcm_vim_score_features", T=BAD_T, alpha=["nan", "inf"], splits=33, R=0, K=2 ** 31 - 1, off="@off+4", work_bytes=3)
    add("mcm_score_stream_workspace_bytes", B=0, K=0, topk=9, splits=33)
    add("mcm_score_features_stream", T=BAD_T, topk=[9, -1], kind=[5, -1], splits=33, B=0, K=0, work_bytes=3, work="@work+4")
    c.append({"entry": "mcm_score_features_stream", "set": {"topk": 3, "idx": "null"}})
    add("mcm_local_workspace_bytes", B=0, R=0, K=0)
    add("mcm_local_score_features", T=BAD_T, B=0, R=0, K=0, local="@local+4", work_bytes=3, scores="null")
    for entry in ("mcm_encode_image_ex", "mcm_encode_image_x2", "mcm_encode_image_local", "mcm_score_topk",
                  "mcm_debug_vision_front"):
        add(entry, pixel_format=[2, -1])
    c.append({"entry": "mcm_score_topk", "set": {"pixel_format": 2, "x2": 1}})
    add("mcm_encode_image_local", local="null")
    add("mcm_score_glmcm", T=BAD_T, K=0, lam="nan", pixel_format=[2, -1], text="null")
    py = []
    for method, sets in (("knn_scores", [{"k": 2000}, {"k": 0}, {"splits": 33}, {"splits": -1}]),
                         ("neglabel_scores", [{"T": 0.0}, {"T": "nan"}, {"splits": 33}]),
                         ("vim_scores", [{"T": 0.0}, {"alpha": "nan"}, {"splits": 33}, {"T": "inf", "splits": -1}]),
                         ("local_scores", [{"T": 0.0}, {"T": "inf"}]),
                         ("score_features", [{"T": 0.0}, {"splits": 33}, {"splits": -1}, {"T": "nan", "splits": 40}])):
        py.extend({"method": method, "set": s, "stub_rc": None} for s in sets)
        py.append({"method": method, "set": {}, "stub_rc": -3})   # MCM_EHIP
    return c, py


class _Buffers:
    """One handle (and a harness one) at P = 64, the operands of B = 5 queries against 300 bank rows, sentinel-filled outputs."""

    def __init__(self):
        from mcm_amd import abi
        from mcm_amd.engine import _stream_ptr

        self.net, self.hnet = gs.widened_net(P), gs.widened_net(P, harness=True)
        abi.declare(self.net._lib, names=list(abi.EXTENSION_PROTOTYPES))
        rng = np.random.default_rng(5)
        unit = lambda *shape: (lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True))(rng.standard_normal(shape))  # noqa: E731
        S, R = self.net.geo.image_size, self.net.local_rows
        self.need = ctypes.c_int64(-1)
        self.t = {"feat": gs.dev(unit(B, P)), "bank": gs.dev(unit(N, P)), "local": gs.dev(unit(B, R, P)),
                  "off": torch.zeros(64, dtype=torch.float64, device="cuda"),
                  "px": torch.zeros((B, 3, S, S), device="cuda")}
        self.outs = {name: torch.full((n,), SENTINEL, device="cuda") for name, n in
                     (("work", 1 << 16), ("out", B), ("aux", B * 4096), ("aux2", B * 4096), ("local_out", B * R * P))}
        self.outs["idx"] = torch.full((B * 8,), -77, dtype=torch.int32, device="cuda")
        self.scalars = {"h": self.net._h, "hh": self.hnet._h, "R": R, "wb": self.outs["work"].numel() * 4,
                        "need": ctypes.byref(self.need), "stream": _stream_ptr()}

    def value(self, v, python=False):
        if not isinstance(v, str):
            return v
        if not v.startswith("@"):
            return None if v == "null" else float(v)
        name, _, off = v[1:].partition("+")
        if name in self.scalars:
            return self.scalars[name]
        t = self.t.get(name, self.outs.get(name))
        return t if python else t.data_ptr() + int(off or 0)

    def untouched(self):
        torch.cuda.synchronize()
        return self.need.value == -1 and all(bool((t == (-77 if name == "idx" else SENTINEL)).all())
                                             for name, t in self.outs.items())

    def close(self):
        self.net.close()
        self.hnet.close()


def _run_c(buf, call):
    args = {**C_ENTRIES[call["entry"]], **call["set"]}
    lib = (buf.hnet if args["h"] == "@hh" else buf.net)._lib
    rc = getattr(lib, call["entry"])(*[buf.value(v) for v in args.values()])
    says = call["entry"].endswith("_workspace_bytes")
    return {"rc": rc, "err": None if says else lib.mcm_last_error(buf.value(args["h"])).decode()}


class _StubLib:
    """The library with one entry replaced by a function that returns `rc`."""

    def __init__(self, lib, entry, rc):
        self.__dict__.update(_lib=lib, _entry=entry, _rc=rc)

    def __getattr__(self, name):
        return (lambda *a: self._rc) if name == self._entry else getattr(self._lib, name)


def _run_py(buf, call):
    net, (operands, kw) = buf.net, PY_METHODS[call["method"]]
    kw = {**kw, **{k: buf.value(v) for k, v in call["set"].items()}}
    real = net._lib
    if call["stub_rc"] is not None:
        net._lib = _StubLib(real, PY_WORKSPACE_ENTRY[call["method"]], call["stub_rc"])
    try:
        getattr(net, call["method"])(*[buf.value(v, python=True) for v in operands], **kw)
    except Exception as e:  # noqa: BLE001 (the class is what is recorded)
        return {"exc": type(e).__name__, "names": {k: re.search(rf"(?<![A-Za-z_]){k}=", str(e)) is not None for k in call["set"]}}
    finally:
        net._lib = real
    return {"exc": None, "names": {}}


@pytest.fixture(scope="module")
def buffers():
    buf = _Buffers()
    yield buf
    buf.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_refusal_is_the_recorded_one(buffers, golden):
    covered = {c["entry"] for c in golden["c_calls"]}
    assert covered == set(C_ENTRIES) and {c["method"] for c in golden["py_calls"]} == set(PY_METHODS)
    for call in golden["c_calls"]:
        got = _run_c(buffers, call)
        assert got["rc"] != 0 and got == {"rc": call["rc"], "err": call["err"]}, (call, got)
    assert buffers.untouched()
    for call in golden["py_calls"]:
        got = _run_py(buffers, call)
        want = "RuntimeError" if call.get("aligned") else call["exc"]
        assert got["exc"] is not None and got == {"exc": want, "names": call["names"]}, (call, got)
        if call.get("aligned"):   # the one deliberate change: k-NN's failures that are no refusal
            assert call["method"] == "knn_scores" and call["stub_rc"] not in (None, -1) and call["exc"] == "ValueError"
    assert buffers.untouched()


def _record():
    c_calls, py_calls = _table()
    buf = _Buffers()
    c_calls = [{**c, **_run_c(buf, c)} for c in c_calls]
    assert buf.untouched()
    py_calls = [{**c, **_run_py(buf, c)} for c in py_calls]
    assert buf.untouched()
    buf.close()
    for c in py_calls:
        if c["method"] == "knn_scores" and c["stub_rc"] is not None and c["exc"] == "ValueError":
            c["aligned"] = True
    lines = lambda calls: "[\n" + ",\n".join("  " + json.dumps(c) for c in calls) + "\n ]"  # noqa: E731
    with open(GOLDEN, "w") as f:
        f.write('{"geometry": "tiny, proj_dim %d; B = %d queries, %d bank rows",\n "c_calls": %s,\n "py_calls": %s}\n'
                % (P, B, N, lines(c_calls), lines(py_calls)))
    print(f"recorded {len(c_calls)} C calls and {len(py_calls)} Python calls to {GOLDEN}")


if __name__ == "__main__":
    import sys

    if sys.argv[1:] == ["--record"]:
        _record()
