"""Measurements of the NegLabel score.  Not a leg of bench.py.

  python tools/neglabel_probe.py [--out FILE] [--batch 512] [--reps 5]

One child process per bank size under a time limit, stopping at the first one that fails.  Per M (negatives kept), at B = --batch
queries, P = 512 (the ViT-B/16 projection width; fp16 handle), K = 1000 ID rows, G = 100 groups of M / 100, T = 0.01, unit-norm
seeded rows, the three routes alternating in one process:
  neglabel_ms       per call of mcm_neglabel_score_features (both kernels), timed under MCM_KC_SCORE through mcm_profile_read;
  torch_ms          the yardstick: torch on the materialised [B, N] fp32 matrix (f @ bank.T / T, two logsumexp, the logistic, the
                    mean), HIP events;
  score_kernel_ms   mcm_score_features(kind = MCM) of the same handle over the same N rows, under mcm_profile_read: the time
                    only (its value is another score); null where its K + P rows do not fit LDS and the call is refused.
One JSON object per M on stdout (and, with --out, all of them in FILE)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probe_common as pc  # noqa: E402

SIZES = [1_000, 10_000, 50_000]
K, G, T = 1000, 100, 0.01


def _torch_route(f, bank, gs):
    import torch

    logit = (f @ bank.T) / T
    LI = torch.logsumexp(logit[:, :K], dim=1)
    LN = torch.logsumexp(logit[:, K:].reshape(f.shape[0], G, gs), dim=2)
    return -(1.0 / (1.0 + torch.exp(LN - LI[:, None]))).mean(dim=1)


def step(M, batch, reps):
    import torch

    net = pc.b16_handle(batch)
    P, gs = net.geo.proj_dim, M // G
    N = K + G * gs
    g = torch.Generator(device="cuda").manual_seed(1)
    bank = torch.nn.functional.normalize(torch.randn((N, P), device="cuda", generator=g), dim=-1)
    f = torch.nn.functional.normalize(bank[torch.randint(0, N, (batch,), device="cuda", generator=g)]
                                      + 0.5 * torch.randn((batch, P), device="cuda", generator=g), dim=-1)
    try:                                                      # the MCM tail over the same bank, where it takes it
        net.score_features(f, bank, T, "MCM")
        parent = True
    except (RuntimeError, ValueError):
        parent = False
    net.profile(True)
    t = pc.agree_and_time(net, lambda: net.neglabel_scores(f, bank, K, G, gs, T=T), lambda: _torch_route(f, bank, gs), reps)
    pk_ms = None
    if parent:
        for _ in range(reps):
            net.score_features(f, bank, T, "MCM")
        pk_ms = net.profile_read()["score"]["ms"] / reps
    res = pc.emit({"M": G * gs, "N": N, "K": K, "G": G, "gs": gs, "B": batch, "P": P, "T": T, "neglabel_ms": t["ms"],
                   "torch_ms": t["yardstick_ms"], "neglabel_over_torch": t["ms"] / t["yardstick_ms"], "score_kernel_ms": pk_ms,
                   "neglabel_over_score_kernel": t["ms"] / pk_ms if parent else None,
                   "neglabel_tflops_fp32": t["flops"] / t["ms"] / 1e9, "max_abs_diff_vs_torch": t["max_abs_diff"]})
    net.profile(False)
    net.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per bank size")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        step(a.child, a.batch, a.reps)
        return 0
    return pc.drive(__file__, [(M,) for M in SIZES], ["--batch", a.batch, "--reps", a.reps], a.limit, a.out,
                    name=lambda s: f"M = {s[0]}")[0]


if __name__ == "__main__":
    sys.exit(main())
