"""What the score probes of tools/ share: the driver that runs one child process per shape, the handles they measure on, and
the loop that times a score of the library against a yardstick on the same device.  Each probe keeps its shapes, inputs,
yardstick and result keys."""
import dataclasses
import json
import os
import subprocess
import sys


def drive(script, shapes, args, limit, out=None, lines_per_shape=1, name=str):
    """One child `python script *args --child *shape` per shape under `timeout -k 10 limit`, stopping at the first that fails
    or prints another number of "PROBE " lines than expected.  Every line is printed as it comes and parsed; `out` is rewritten
    with all results so far after each shape.  Returns (exit code, results)."""
    results = []
    for shape in shapes:
        cmd = (["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(script)] + [str(v) for v in args]
               + ["--child"] + [str(v) for v in shape])
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln[6:] for ln in r.stdout.splitlines() if ln.startswith("PROBE ")]
        for ln in lines:
            results.append(json.loads(ln))
            print(ln, flush=True)
        if out:
            with open(out, "w") as fh:
                json.dump(results, fh, indent=1)
        if r.returncode or len(lines) != lines_per_shape:
            print(f"{name(shape)} failed (exit {r.returncode}); stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1, results
    return 0, results


def emit(res):
    print("PROBE " + json.dumps(res), flush=True)
    return res


def b16_handle(batch, P=None):
    """The ViT-B/16 towers (fp16, fp16-exact seeded weights, no split-activation workspace), widened to proj_dim = P if given."""
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry("ViT-B/16")
    if P is not None and P != geo.proj_dim:
        geo = dataclasses.replace(geo, name=f"ViT-B/16-P{P}", proj_dim=P)
    return NativeCLIP(geo, synth_state_dict(geo, 0, regime="fp16-exact"), precision="fp16", max_batch=batch,
                      synthetic_weights=True, x2_max_batch=-1)


def tiny_handle(P):
    """The tiny geometry widened to proj_dim = P: a handle for a score that runs on features alone."""
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = dataclasses.replace(geometry("tiny"), name=f"tiny-P{P}", proj_dim=P)
    return NativeCLIP(geo, synth_state_dict(geo, 0), precision="fp16", max_batch=8, max_prompt_tokens=256)


def kernels_ms(stats):
    """The kernel time of a `profile_read` (the gemm_* classes repeat launches of "gemm")."""
    return sum(v["ms"] for kc, v in stats.items() if not kc.startswith("gemm_"))


def agree_and_time(net, mine, yardstick, reps):
    """Warm both routes up and compare what they return; then `reps` rounds of mine() followed by yardstick(), mine timed under
    MCM_KC_SCORE through mcm_profile_read (profiling must be on), the yardstick by HIP events around it.  Returns per call of
    mine its ms and flops, the launches counted over all rounds, the yardstick's ms per call and the largest difference."""
    import torch

    a, b = mine(), yardstick()
    torch.cuda.synchronize()
    agree = float((a - b).abs().max())
    net.profile_read()
    t_ms, ev = 0.0, [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(reps):
        mine()
        ev[0].record()
        yardstick()
        ev[1].record()
        torch.cuda.synchronize()
        t_ms += ev[0].elapsed_time(ev[1])
    st = net.profile_read()["score"]
    assert st["launches"] == reps, st
    return {"ms": st["ms"] / reps, "flops": st["flops"] / reps, "launches": st["launches"], "yardstick_ms": t_ms / reps,
            "max_abs_diff": agree}
