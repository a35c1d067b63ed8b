"""Measurements of the two tails of the MCM family side by side.  Not a leg of bench.py; nothing is asserted.

  python tools/score_stream_probe.py [--out FILE] [--batch 512] [--reps 30]

One child process per bank size under a time limit, stopping at the first one that fails.  Per K in 1 000, 10 000, 21 841,
37 888 (the last the LDS tail takes at P = 512) and 80 000, at B = --batch queries, P = 512, T = 0.01, kind MCM, unit-norm seeded
rows (fp16 handle of the tiny geometry widened to P), with topk 0 and 5, the routes alternating in one process, all warmed up
first, each call between two device events and a synchronise behind every round:
  stream_ms  per call of `score_features(..., tail="stream")`: both kernels of score_stream.hip, splits = the library's choice;
  lds_ms     per call of `score_features(..., tail="lds")`: score.hip's one launch, where it takes the shape (else null);
  torch_ms   the yardstick: torch on the materialised [B, K] fp32 matrix (f @ bank.T, softmax(s / T), its maximum; with topk
             torch.topk of s and the probabilities gathered).
The times are host-enqueued calls seen by device events: at the small K they hold launch overhead, which is part of what a
caller pays.  One JSON object per (K, topk) on stdout (and, with --out, all of them in FILE), then the table."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probe_common as pc  # noqa: E402

P, T = 512, 0.01
BANKS = [1000, 10000, 21841, 37888, 80000]
TOPKS = [0, 5]


def _torch_route(f, bank, topk):
    import torch

    s = f @ bank.T
    p = torch.softmax(s / T, dim=1)
    if not topk:
        return -p.max(dim=1).values
    idx = torch.topk(s, topk, dim=1).indices
    return -p.max(dim=1).values, idx, torch.gather(p, 1, idx)


def step(K, batch, reps):
    import torch

    from mcm_amd import abi

    net = pc.tiny_handle(P)
    g = torch.Generator(device="cuda").manual_seed(1)
    bank = torch.nn.functional.normalize(torch.randn((K, P), device="cuda", generator=g), dim=-1)
    f = torch.nn.functional.normalize(bank[torch.randint(0, K, (batch,), device="cuda", generator=g)]
                                      + 0.5 * torch.randn((batch, P), device="cuda", generator=g), dim=-1)
    lds_ok = (P + K) * 4 <= abi.DEFINES["MCM_SCORE_LDS_MAX_BYTES"]
    for topk in TOPKS:
        routes = {"stream": lambda: net.score_features(f, bank, T, "MCM", topk=topk, tail="stream"),
                  "torch": lambda: _torch_route(f, bank, topk)}
        if lds_ok:
            routes["lds"] = lambda: net.score_features(f, bank, T, "MCM", topk=topk, tail="lds")
        first = {}
        for name, fn in routes.items():                      # warm-up of every route; what they return is compared, not judged
            for _ in range(2):
                first[name] = fn()
        torch.cuda.synchronize()
        score = {n: (r[0] if topk else r) for n, r in first.items()}
        diff = {n: float((score[n] - score["stream"]).abs().max()) for n in score if n != "stream"}
        ms = dict.fromkeys(routes, 0.0)
        ev = {n: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for n in routes}
        for _ in range(reps):                                # alternating
            for name, fn in routes.items():
                ev[name][0].record()
                fn()
                ev[name][1].record()
            torch.cuda.synchronize()
            for name in routes:
                ms[name] += ev[name][0].elapsed_time(ev[name][1])
        res = {"K": K, "P": P, "B": batch, "T": T, "topk": topk, "reps": reps, "stream_ms": ms["stream"] / reps,
               "lds_ms": ms["lds"] / reps if lds_ok else None, "torch_ms": ms["torch"] / reps,
               "stream_tflops_fp32": 2.0 * batch * K * P / (ms["stream"] / reps) / 1e9,
               "max_abs_diff_vs_stream": diff}
        pc.emit(res)
    net.close()


def table(results):
    rows = ["| K | topk | streamed | LDS | torch on [B, K] | streamed / LDS | streamed TF/s fp32 |", "|---|---|---|---|---|---|---|"]
    for r in results:
        lds = "refused" if r["lds_ms"] is None else f"{r['lds_ms']:.3f} ms"
        rel = "" if r["lds_ms"] is None else f"{r['stream_ms'] / r['lds_ms']:.2f}"
        rows.append(f"| {r['K']} | {r['topk']} | {r['stream_ms']:.3f} ms | {lds} | {r['torch_ms']:.3f} ms | {rel} | "
                    f"{r['stream_tflops_fp32']:.1f} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--limit", type=int, default=150, help="seconds per bank size")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        step(a.child, a.batch, a.reps)
        return 0
    rc, results = pc.drive(__file__, [(K,) for K in BANKS], ["--batch", a.batch, "--reps", a.reps], a.limit, a.out, len(TOPKS),
                           lambda s: f"K = {s[0]}")
    if not rc:
        print(table(results))
    return rc


if __name__ == "__main__":
    sys.exit(main())
