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
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

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

    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry("ViT-B/16")
    net = NativeCLIP(geo, synth_state_dict(geo, 0, regime="fp16-exact"), precision="fp16", max_batch=batch,
                     synthetic_weights=True, x2_max_batch=-1)
    P, gs = geo.proj_dim, M // G
    N = K + G * gs
    g = torch.Generator(device="cuda").manual_seed(1)
    bank = torch.nn.functional.normalize(torch.randn((N, P), device="cuda", generator=g), dim=-1)
    f = torch.nn.functional.normalize(bank[torch.randint(0, N, (batch,), device="cuda", generator=g)]
                                      + 0.5 * torch.randn((batch, P), device="cuda", generator=g), dim=-1)
    mine = net.neglabel_scores(f, bank, K, G, gs, T=T)        # warm-up of the routes, and the first two must agree
    ref = _torch_route(f, bank, gs)
    try:
        net.score_features(f, bank, T, "MCM")
        parent = True
    except (RuntimeError, ValueError):
        parent = False
    torch.cuda.synchronize()
    agree = float((mine - ref).abs().max())
    net.profile(True)
    net.profile_read()
    t_ms, ev = 0.0, [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(reps):                                     # alternating
        net.neglabel_scores(f, bank, K, G, gs, T=T)
        ev[0].record()
        _torch_route(f, bank, gs)
        ev[1].record()
        torch.cuda.synchronize()
        t_ms += ev[0].elapsed_time(ev[1])
    mn = net.profile_read()["score"]
    assert mn["launches"] == reps, mn
    pk = None
    if parent:
        for _ in range(reps):
            net.score_features(f, bank, T, "MCM")
        pk = net.profile_read()["score"]
    res = {"M": G * gs, "N": N, "K": K, "G": G, "gs": gs, "B": batch, "P": P, "T": T, "neglabel_ms": mn["ms"] / reps,
           "torch_ms": t_ms / reps, "neglabel_over_torch": mn["ms"] / t_ms,
           "score_kernel_ms": pk["ms"] / reps if pk else None, "neglabel_over_score_kernel": mn["ms"] / pk["ms"] if pk else None,
           "neglabel_tflops_fp32": mn["flops"] / reps / (mn["ms"] / reps) / 1e9, "max_abs_diff_vs_torch": agree}
    print("PROBE " + json.dumps(res), flush=True)
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
    results = []
    for M in SIZES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--batch", str(a.batch),
               "--reps", str(a.reps), "--child", str(M)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln[6:] for ln in r.stdout.splitlines() if ln.startswith("PROBE ")]
        for ln in lines:
            results.append(json.loads(ln))
            print(ln, flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(results, fh, indent=1)
        if r.returncode or len(lines) != 1:
            print(f"M = {M} failed (exit {r.returncode}); stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
