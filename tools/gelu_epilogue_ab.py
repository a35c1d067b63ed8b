"""A/B of the fc1 epilogue: QuickGELU (`ViT-B/16`) against the exact erf GELU (`ViT-B/16-laion2b`) in ONE process, interleaved.

Two fp16 handles on the same seeded fp16-exact weights (the single-operand regime) and the same pixels; the shapes are
identical, so the whole difference is the activation in the fc1 epilogue.  Rounds alternate A, B, A, B ...; each round is
`--steps` score_images calls between two device synchronisations, timed on the host clock (20 steps of ~20 ms).  Prints img/s
(median / min over the rounds) per handle.  The MCM_KC_GEMM_FC1 time per launch comes from a SEPARATE 5-step pass at the end
with the library's event timing on (mcm_profile_enable brackets every launch with events: not the timed rounds).

    python tools/gelu_epilogue_ab.py [--batch 512] [--rounds 6] [--steps 20]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.synth import make_token_ids
    from mcm_amd.weights import synth_state_dict

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--precision", default="fp16")
    a = ap.parse_args()
    names = ("ViT-B/16", "ViT-B/16-laion2b")
    sd = synth_state_dict(geometry(names[0]), 0, "fp16-exact")
    ids, mask = make_token_ids(1000, seed=2)
    g = torch.Generator(device="cuda").manual_seed(1)
    px = torch.randn((a.batch, 3, 224, 224), device="cuda", generator=g)
    nets, banks = {}, {}
    for n in names:
        nets[n] = NativeCLIP(geometry(n), sd, precision=a.precision, max_batch=a.batch, x2_max_batch=-1 if a.precision == "fp16" else None)
        banks[n] = nets[n].get_text_features(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), normalize=True)
    out = torch.empty(a.batch, device="cuda")

    def run(n, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            nets[n].score_images(px, banks[n], out=out)
        torch.cuda.synchronize()
        return a.batch * steps / (time.perf_counter() - t0)

    for n in names:
        run(n, 5)   # warm-up
    rates = {n: [] for n in names}
    for _ in range(a.rounds):
        for n in names:
            rates[n].append(run(n, a.steps))
    fc1 = {}
    for n in names:
        nets[n].profile(True)
        run(n, 5)
        p = nets[n].profile_read()
        nets[n].profile(False)
        fc1[n] = (1e3 * p["gemm_fc1"]["ms"] / max(1, p["gemm_fc1"]["launches"]), p["gemm_fc1"]["launches"],
                  p["gemm_fc1"]["flops"] / max(1e-9, p["gemm_fc1"]["ms"]) / 1e9)
    print(f"fc1 epilogue A/B, {a.precision}, batch {a.batch}, {a.rounds} interleaved rounds x {a.steps} steps, fp16-exact seeded weights")
    for n in names:
        r = rates[n]
        print(f"  {n:18s} img/s median {statistics.median(r):9.1f}  min {min(r):9.1f}  max {max(r):9.1f}   "
              f"fc1 {fc1[n][0]:7.1f} us / launch ({fc1[n][1]} launches, {fc1[n][2]:.0f} TFLOP/s)")
    ma, mb = (statistics.median(rates[n]) for n in names)
    print(f"  erf / quick: end to end {mb / ma:.4f}, fc1 time {fc1[names[1]][0] / fc1[names[0]][0]:.4f}")
    for n in names:
        nets[n].close()


if __name__ == "__main__":
    main()
