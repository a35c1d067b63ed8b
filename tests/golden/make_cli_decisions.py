"""Record tests/golden/cli_decisions.json: what `eval_ood_detection.process_args` of this tree decides for the command lines
of tests/test_cli_decisions_cpu.py (every --score crossed with --predict, --refine-threshold, --ctx, --dtype and --maha-fit):
the refusal message, or the resolved T, refine_threshold, predict and log directory.  Needs no GPU.

  python tests/golden/make_cli_decisions.py [--out FILE]

The file in git was recorded at the commit before the scores moved into the table of mcm_amd/scores.py.  Run this only at a commit
whose decisions are meant to become the yardstick, never to make a failing test pass."""
import argparse
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(HERE, "cli_decisions.json"))
    a = ap.parse_args()
    from tests.test_cli_decisions_cpu import decisions

    with tempfile.TemporaryDirectory() as tmp:
        out = decisions(tmp)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(f"{a.out}: {len(out)} command lines, {sum('error' in d for d in out)} refused")
    return 0


if __name__ == "__main__":
    sys.exit(main())
