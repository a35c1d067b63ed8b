"""Measurements of the device Mahalanobis fit.  Not a leg of bench.py.

  python tools/maha_fit_probe.py [--out FILE] [--images 20480] [--batch 512]

Runs every GPU step as a child process of its own under a time limit and stops at the first one that fails:
  launch P   per-launch time of mcm_maha_fit_accumulate at B = --batch through mcm_profile_read, next to one mcm_score step of
             the same handle (ViT-B/16 towers, fp16 operands; P = 512 is the checkpoint's own projection width, 768 and 1024
             are the same towers with a wider projection: the tower step hardly moves, the fit launch grows with P^2);
  fit ROUTE  wall time, images/s and peak host RSS of get_mean_prec (host) and get_mean_prec_device (device) over --images
             seeded synthetic ViT-B/16 images at --batch.
One JSON object per step on stdout (and, with --out, all of them in FILE)."""
import argparse
import os
import resource
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probe_common as pc  # noqa: E402


def step_launch(P, batch, reps=20):
    import torch

    net = pc.b16_handle(batch, P)
    g = torch.Generator(device="cuda").manual_seed(1)
    px = torch.randn((batch, 3, net.geo.image_size, net.geo.image_size), device="cuda", generator=g)
    bank = torch.nn.functional.normalize(torch.randn((1000, P), device="cuda", generator=g), dim=-1)
    feats = net.get_image_features(px)
    state = net.maha_fit_state(feats.mean(dim=0))
    for _ in range(3):                       # warm-up of both
        net.score_images(px, bank, 1.0, "MCM")
        net.maha_fit_accumulate(feats, state)
    torch.cuda.synchronize()
    net.profile(True)
    net.profile_read()
    for _ in range(reps):
        net.maha_fit_accumulate(feats, state)
    fit = net.profile_read()["score"]
    for _ in range(reps):
        net.score_images(px, bank, 1.0, "MCM")
    step = net.profile_read()
    net.profile(False)
    assert fit["launches"] == reps, fit
    step_ms = pc.kernels_ms(step) / reps
    fit_ms = fit["ms"] / reps
    net.close()
    return {"step": "launch", "P": P, "B": batch, "fit_launch_ms": fit_ms, "score_step_kernel_ms": step_ms,
            "fit_over_step": fit_ms / step_ms, "fit_gflops_fp64": fit["flops"] / reps / fit_ms / 1e6}


def step_fit(route, images, batch, tdir):
    import torch

    from mcm_amd.detection import get_mean_prec, get_mean_prec_device
    from mcm_amd.synth import DevicePatternLoader

    net = pc.b16_handle(batch, 512)
    args = types.SimpleNamespace(n_cls=1000, feat_dim=512, model="CLIP", normalize=False, template_dir=tdir,
                                 in_dataset="ImageNet", max_count=250, batch_size=batch)
    fn = get_mean_prec_device if route == "device" else get_mean_prec

    def loader(n):
        return DevicePatternLoader(n, net.geo.image_size, 1000, batch, net.device, ood=False, seed=7)

    fn(args, net, loader(2 * batch))       # warm-up: kernels loaded, LAPACK initialised
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(args, net, loader(images))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    net.close()
    return {"step": "fit", "route": route, "images": images, "batch": batch, "wall_s": dt, "images_per_s": images / dt,
            "peak_host_rss_mb": resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=20480)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        import tempfile

        if a.child[0] == "launch":
            res = step_launch(int(a.child[1]), a.batch)
        else:
            with tempfile.TemporaryDirectory() as tdir:
                res = step_fit(a.child[1], a.images, a.batch, tdir)
        pc.emit(res)
        return 0
    steps = [["launch", "512"], ["launch", "768"], ["launch", "1024"], ["fit", "device"], ["fit", "host"]]
    return pc.drive(__file__, steps, ["--images", a.images, "--batch", a.batch], a.limit, a.out,
                    name=lambda s: f"step {s}")[0]


if __name__ == "__main__":
    sys.exit(main())
