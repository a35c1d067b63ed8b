"""Measurements of the k-nearest-neighbour score.  Not a leg of bench.py.

  python tools/knn_probe.py [--out FILE] [--batch 512] [--reps 3]

One child process per bank size under a time limit, stopping at the first one that fails.  Per (N, k), at B = --batch queries
and P = 512 (the ViT-B/16 projection width; fp16 handle), unit-norm seeded rows:
  knn_launch_ms     per call of mcm_knn_score_features (both kernels), timed under MCM_KC_SCORE through mcm_profile_read;
  torch_topk_ms     the yardstick: torch.topk(f @ bank.T, k) on the same device and data, the bank in chunks of 131072 rows
                    (one [B, chunk] matrix at a time) and a last top-k over the chunks' winners; HIP events, alternating with
                    the calls above in the same process;
  score_step_ms     the kernels of one mcm_score step of the same handle at the same batch.
One JSON object per (N, k) on stdout (and, with --out, all of them in FILE)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probe_common as pc  # noqa: E402

SIZES = [25_000, 250_000, 1_281_167]
KS = [10, 200, 1000]
CHUNK = 131072


def _torch_route(f, bank, k):
    import torch

    best = None
    for s in range(0, bank.shape[0], CHUNK):
        v = torch.topk(f @ bank[s:s + CHUNK].T, min(k, bank.shape[0] - s), dim=1).values
        best = v if best is None else torch.topk(torch.cat([best, v], dim=1), min(k, best.shape[1] + v.shape[1]), dim=1).values
    return torch.sqrt(torch.clamp(2.0 - 2.0 * best[:, -1], min=0.0))


def step(N, batch, reps):
    import torch

    net = pc.b16_handle(batch)
    geo, P = net.geo, net.geo.proj_dim
    g = torch.Generator(device="cuda").manual_seed(1)
    bank = torch.nn.functional.normalize(torch.randn((N, P), device="cuda", generator=g), dim=-1)
    f = torch.nn.functional.normalize(bank[torch.randint(0, N, (batch,), device="cuda", generator=g)]
                                      + 0.05 * torch.randn((batch, P), device="cuda", generator=g), dim=-1)
    px = torch.randn((batch, 3, geo.image_size, geo.image_size), device="cuda", generator=g)
    prompts = torch.nn.functional.normalize(torch.randn((1000, P), device="cuda", generator=g), dim=-1)
    for _ in range(2):
        net.score_images(px, prompts, 1.0, "MCM")
    torch.cuda.synchronize()
    net.profile(True)
    net.profile_read()
    for _ in range(reps):
        net.score_images(px, prompts, 1.0, "MCM")
    step_ms = pc.kernels_ms(net.profile_read()) / reps
    out = []
    for k in KS:
        t = pc.agree_and_time(net, lambda: net.knn_scores(f, bank, k), lambda: _torch_route(f, bank, k), reps)
        out.append(pc.emit({"N": N, "k": k, "B": batch, "P": P, "knn_launch_ms": t["ms"], "torch_topk_ms": t["yardstick_ms"],
                            "knn_over_torch": t["ms"] / t["yardstick_ms"], "score_step_ms": step_ms,
                            "knn_over_step": t["ms"] / step_ms, "knn_tflops_fp32": t["flops"] / t["ms"] / 1e9,
                            "max_abs_diff_vs_torch": t["max_abs_diff"]}))
    net.profile(False)
    net.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per bank size")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        step(a.child, a.batch, a.reps)
        return 0
    return pc.drive(__file__, [(N,) for N in SIZES], ["--batch", a.batch, "--reps", a.reps], a.limit, a.out, len(KS),
                    lambda s: f"N = {s[0]}")[0]


if __name__ == "__main__":
    sys.exit(main())
