"""Measurements of the ViM score.  Not a leg of bench.py.

  python tools/vim_probe.py [--out FILE] [--batch 512] [--reps 20]

One child process per shape under a time limit, stopping at the first one that fails.  Per (P, R), at B = --batch queries,
K = 1000 prompt rows, T = 0.01, unit-norm seeded rows and an orthonormal basis (fp16 handle of the tiny geometry widened to P),
the two routes alternating in one process, both warmed up first:
  vim_ms     per call of mcm_vim_score_features (both kernels), timed under MCM_KC_SCORE through mcm_profile_read;
  torch_ms   the yardstick: torch on the materialised [B, K + R] fp32 matrix (f @ bank.T, logsumexp of the prompt columns / T
             plus the norm of the basis columns), HIP events.
One JSON object per shape on stdout (and, with --out, all of them in FILE)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probe_common as pc  # noqa: E402

SHAPES = [(512, 256), (1024, 512)]   # (P, R): ViT-B/16's and ViT-H/14's projection widths at the default D
K, T, ALPHA = 1000, 0.01, 1.5


def _torch_route(f, bank):
    import torch

    s = f @ bank.T
    return ALPHA * torch.linalg.vector_norm(s[:, K:], dim=1) - torch.logsumexp(s[:, :K] / T, dim=1)


def step(P, R, batch, reps):
    import torch

    net = pc.tiny_handle(P)
    g = torch.Generator(device="cuda").manual_seed(1)
    prompts = torch.nn.functional.normalize(torch.randn((K, P), device="cuda", generator=g), dim=-1)
    basis = torch.linalg.qr(torch.randn((P, R), device="cuda", generator=g)).Q.T.contiguous()
    bank = torch.cat([prompts, basis]).contiguous()
    f = torch.nn.functional.normalize(prompts[torch.randint(0, K, (batch,), device="cuda", generator=g)]
                                      + 0.5 * torch.randn((batch, P), device="cuda", generator=g), dim=-1)
    net.profile(True)
    t = pc.agree_and_time(net, lambda: net.vim_scores(f, bank, K, T=T, alpha=ALPHA), lambda: _torch_route(f, bank), reps)
    res = pc.emit({"P": P, "R": R, "K": K, "N": K + R, "B": batch, "T": T, "reps": reps, "vim_ms": t["ms"],
                   "torch_ms": t["yardstick_ms"], "vim_over_torch": t["ms"] / t["yardstick_ms"],
                   "vim_tflops_fp32": t["flops"] / t["ms"] / 1e9, "max_abs_diff_vs_torch": t["max_abs_diff"]})
    net.profile(False)
    net.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=120, help="seconds per shape")
    ap.add_argument("--child", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        step(a.child[0], a.child[1], a.batch, a.reps)
        return 0
    return pc.drive(__file__, SHAPES, ["--batch", a.batch, "--reps", a.reps], a.limit, a.out,
                    name=lambda s: f"P = {s[0]}, R = {s[1]}")[0]


if __name__ == "__main__":
    sys.exit(main())
