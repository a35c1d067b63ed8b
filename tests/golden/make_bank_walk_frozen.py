"""Record a frozen-bits fixture of the bank-streamed scores, as the library built in this tree computes them on an MI355X, with
the ROCm version and the commit they were made at:
  --which walk (the default)  tests/golden/bank_walk_frozen.npz: the k-NN and NegLabel scores at the cases of
                              tests/test_gpu_bank_walk_frozen.py;
  --which fold                tests/golden/bank_fold_frozen.npz: the ViM and GL-MCM local scores at the cases of
                              tests/test_gpu_bank_fold_frozen.py.

  python tests/golden/make_bank_walk_frozen.py --commit HASH [--which walk|fold] [--out FILE]

The walk fixture in git was recorded at the commit before knn.hip and neglabel.hip took their walk from bank_sim.hpp, the fold
fixture at the commit before neglabel.hip, vim.hip and glmcm.hip took their log-sum-exp fold from it.  Run this only at a commit
whose bits are meant to become the yardstick, never to make a failing test pass."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--which", choices=("walk", "fold"), default="walk")
    ap.add_argument("--out", default=None, help="default: bank_WHICH_frozen.npz next to this script")
    ap.add_argument("--commit", required=True, help="the commit this tree is a checkout of (recorded in the fixture)")
    a = ap.parse_args()
    a.out = a.out or os.path.join(HERE, f"bank_{a.which}_frozen.npz")
    import importlib

    import torch

    out = importlib.import_module(f"tests.test_gpu_bank_{a.which}_frozen").frozen_outputs()
    np.savez_compressed(a.out, rocm=np.array(str(torch.version.hip)), commit=np.array(a.commit), **out)
    print(f"{a.out}: {len(out)} arrays, {os.path.getsize(a.out)} bytes, ROCm {torch.version.hip}, commit {a.commit}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
