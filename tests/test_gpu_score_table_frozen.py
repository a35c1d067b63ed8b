"""The command-line driver, frozen: one `eval_ood_detection.main` run per --score (and per --maha-fit, --predict and
--refine-threshold arm) must give, bit for bit, the scores, measures, predictions, log lines, CSV and JSON files that the commit
before the scores moved into the table of mcm_amd/scores.py gave on an MI355X (tests/golden/score_table_frozen.npz, recorded there
by tests/golden/make_score_table_frozen.py), and leave `net.kernel_faults` at 0.  Shape: ImageNet10 against ImageNet20, 80 seeded
synthetic images per set in batches of 32 (32 + 32 + 16: the tail cut runs, and the Mahalanobis rule that an OOD set's trailing
partial batch is not scored leaves 64 of the 80), ViT-B/32 with seeded weights."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_table_frozen.npz")
REGENERATE = ("to regenerate: check out the commit whose bits are to be kept, build it, and run "
              "`python tests/golden/make_score_table_frozen.py --commit HASH` there on an MI355X (with this module and that script "
              "copied in)")
BASE = ["--in_dataset", "ImageNet10", "--CLIP_ckpt", "ViT-B/32", "--synthetic", "--synthetic-n", "80", "-b", "32", "--name", "f"]
RUNS = {s: ["--score", s] for s in ("MCM", "energy", "max-logit", "entropy", "var", "GL-MCM", "knn")}
RUNS.update({
    "maha-host": ["--score", "maha", "--maha-fit", "host"],
    "maha-device": ["--score", "maha", "--maha-fit", "device"],
    "neglabel": ["--score", "neglabel", "--neg-words", "words.txt", "--neg-groups", "4"],
    "vim": ["--score", "vim", "--vim-dim", "32"],      # (80 training rows determine 32 principal directions)
    "MCM-predict": ["--score", "MCM", "--predict", "3"],
    "MCM-refine-on": ["--score", "MCM", "--dtype", "fp16", "--refine-threshold", "on"],
    "MCM-refine-exact": ["--score", "MCM", "--dtype", "fp16", "--refine-threshold", "exact"],
})
WORDS = [a + b for a in ("ka", "lo", "mi", "ne", "pu", "ra") for b in ("bar", "den", "fil", "gom", "hut", "jix", "zor", "wyn")]
STAMP = re.compile(r"^\d{4}-\d\d-\d\d \d\d:\d\d:\d\d,\d{3} : ", re.M)


def _host(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)


def run_case(name, workdir):
    """One run of the driver in `workdir`: ({array name: array}, [kernel_faults of every handle of the run, read as it closes])."""
    import eval_ood_detection as cli
    import mcm_amd.engine as eng

    faults, real = [], eng.build_model

    def build_model(*a, **kw):
        net = real(*a, **kw)
        close = net.close

        def closing():
            if getattr(net, "_h", None):
                faults.append(net.kernel_faults)
            close()

        net.close = closing
        return net

    here = os.getcwd()
    os.chdir(workdir)
    eng.build_model = build_model
    try:
        with open("words.txt", "w") as f:
            f.write("\n".join(WORDS) + "\n")
        res = cli.main(BASE + RUNS[name])
        sets = list(res["out_scores"])
        out = {"in_score": _host(res["in_score"]), "measures": np.array([res["measures"][d] for d in sets], np.float64)}
        for d in sets:
            out[f"out/{d}"] = _host(res["out_scores"][d])
        logdir = res["log_directory"]
        for what in ["id"] + sets:
            f = os.path.join(logdir, f"predictions_{what}.npz")
            if os.path.exists(f):
                with np.load(f) as z:
                    out.update({f"pred/{what}/{k}": z[k] for k in ("idx", "prob", "scores", "labels")})
        for f in ("ood_eval_info.log", "f.csv", "data_sources.json", "refine_rank0.json"):
            if os.path.exists(os.path.join(logdir, f)):
                out[f"file/{f}"] = np.array(STAMP.sub("", open(os.path.join(logdir, f)).read()))
        return out, faults
    finally:
        eng.build_model = real
        os.chdir(here)


def _same(w, g):
    if w.dtype == np.float32:
        w, g = w.view(np.int32), g.view(np.int32)
    return np.array_equal(w, g)


@pytest.mark.parametrize("name", list(RUNS))
def test_the_run_keeps_the_recorded_bits(name, tmp_path):
    with np.load(FIXTURE) as z:
        want = {n[len(name) + 1:]: z[n] for n in z.files if n.startswith(name + "/")}
        made_with = (f"(fixture made at commit {z['commit'].item()} with ROCm {z['rocm'].item()}; this is ROCm "
                     f"{torch.version.hip}; {REGENERATE})")
    got, faults = run_case(name, tmp_path)
    assert faults and all(f == 0 for f in faults), faults
    assert sorted(want) == sorted(got), made_with
    assert want["in_score"].dtype == np.float32 and want["in_score"].shape == (80,)
    for n in sorted(want):
        w, g = want[n], got[n]
        assert w.dtype == g.dtype and w.shape == g.shape, (n, made_with)
        assert _same(w, g), (n, w, g, made_with)
    print(f"FROZEN {name}: {len(want)} arrays and files equal to the recorded ones")
