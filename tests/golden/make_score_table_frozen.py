"""Record tests/golden/score_table_frozen.npz: what `eval_ood_detection.main` of this tree returns and writes for the runs of
tests/test_gpu_score_table_frozen.py (one per --score, per --maha-fit, and the --predict and --refine-threshold arms of MCM), as
the library built in this tree computes them on an MI355X, with the ROCm version and the commit they were made at.

  python tests/golden/make_score_table_frozen.py --commit HASH [--out FILE]

The fixture in git was recorded at the commit before the scores moved into the table of mcm_amd/scores.py.  Run this only at a
commit whose bits are meant to become the yardstick, never to make a failing test pass."""
import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(HERE, "score_table_frozen.npz"))
    ap.add_argument("--commit", required=True, help="the commit this tree is a checkout of (recorded in the fixture)")
    a = ap.parse_args()
    a.out = os.path.abspath(a.out)
    import torch

    from tests.test_gpu_score_table_frozen import RUNS, run_case

    out = {}
    for name in RUNS:
        with tempfile.TemporaryDirectory() as tmp:
            got, faults = run_case(name, tmp)
        assert faults and all(f == 0 for f in faults), (name, faults)
        out.update({f"{name}/{k}": v for k, v in got.items()})
    np.savez_compressed(a.out, rocm=np.array(str(torch.version.hip)), commit=np.array(a.commit), **out)
    print(f"{a.out}: {len(out)} arrays, {os.path.getsize(a.out)} bytes, ROCm {torch.version.hip}, commit {a.commit}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
