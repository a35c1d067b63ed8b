"""Measurements of the GL-MCM score.  Not a leg of bench.py.

  python tools/glmcm_probe.py [--out FILE] [--batch 512] [--reps 5]

One child process under a time limit.  ViT-B/16 (fp16 handle, fp16-exact seeded weights), B = --batch images, K = 1000
unit-norm seeded prompts, T = 1:
  score_ms          wall time of one `score_images` call (the forward and the MCM tail), HIP events;
  glmcm_ms          the same for `score_images_glmcm` (the forward, the local pass, both tails and the combination),
                    alternating with the call above in the same process;
  local_pass_ms     the launches `get_local_features` adds behind the forward (memsets excluded: they are not timed
                    launches): the kernels of one call minus the kernels of one `get_image_features` call, both through
                    mcm_profile_read;
  local_tail_ms     per call of mcm_local_score_features on [B, R, P] rows (both kernels), timed under MCM_KC_SCORE.
One JSON object on stdout (and, with --out, in FILE)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probe_common as pc  # noqa: E402


def step(batch, reps):
    import torch

    net = pc.b16_handle(batch)
    geo, (P, K, T) = net.geo, (net.geo.proj_dim, 1000, 1.0)
    g = torch.Generator(device="cuda").manual_seed(1)
    px = torch.randn((batch, 3, geo.image_size, geo.image_size), device="cuda", generator=g)
    prompts = torch.nn.functional.normalize(torch.randn((K, P), device="cuda", generator=g), dim=-1)
    for _ in range(2):                                        # warm-up of both routes
        plain = net.score_images(px, prompts, T, "MCM")
        score, gs, ls, _patch = net.score_images_glmcm(px, prompts, T, 1.0, return_parts=True)
    torch.cuda.synchronize()
    assert torch.equal(gs, plain) and torch.isfinite(score).all() and (ls < 0).all()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    s_ms = g_ms = 0.0
    for _ in range(reps):                                     # alternating
        ev[0].record()
        net.score_images(px, prompts, T, "MCM")
        ev[1].record()
        net.score_images_glmcm(px, prompts, T, 1.0)
        ev[2].record()
        torch.cuda.synchronize()
        s_ms += ev[0].elapsed_time(ev[1])
        g_ms += ev[1].elapsed_time(ev[2])
    net.profile(True)
    net.profile_read()
    for _ in range(reps):
        net.get_image_features(px, normalize=True)
    fwd = net.profile_read()
    for _ in range(reps):
        _glob, loc = net.get_local_features(px)
    both = net.profile_read()
    for _ in range(reps):
        net.local_scores(loc, prompts, T)
    tail = net.profile_read()["score"]
    assert tail["launches"] == reps, tail
    res = {"model": "ViT-B/16", "precision": "fp16", "B": batch, "R": net.local_rows, "K": K, "P": P, "T": T,
           "score_ms": s_ms / reps, "glmcm_ms": g_ms / reps, "glmcm_over_score": g_ms / s_ms,
           "forward_kernels_ms": pc.kernels_ms(fwd) / reps, "local_pass_ms": (pc.kernels_ms(both) - pc.kernels_ms(fwd)) / reps,
           "local_pass_launches": (sum(v["launches"] for kc, v in both.items() if not kc.startswith("gemm_"))
                                   - sum(v["launches"] for kc, v in fwd.items() if not kc.startswith("gemm_"))) // reps,
           "local_tail_ms": tail["ms"] / reps, "local_tail_tflops_fp32": tail["flops"] / reps / (tail["ms"] / reps) / 1e9}
    pc.emit(res)
    net.profile(False)
    net.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds for the child")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        step(a.batch, a.reps)
        return 0
    rc, results = pc.drive(__file__, [()], ["--batch", a.batch, "--reps", a.reps], a.limit, name=lambda s: "the probe")
    if not rc and a.out:
        with open(a.out, "w") as fh:
            json.dump(results[0], fh, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
