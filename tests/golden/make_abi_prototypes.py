"""Record tests/golden/abi_prototypes.json: what this tree's Python binds of the C ABI (include/mcm.h) — the restype and argtypes
mcm_amd.engine.load_library declares for every entry (as type names; every pointer type but c_char_p written c_void_p, a missing
argtypes written []), EXPORTED_SYMBOLS and HARNESS_ONLY_SYMBOLS (sorted), the constants that mirror a #define, and the fields and
sizes of CConfig and JpegImage.  Loads nothing native (a recorder stands where ctypes.CDLL does) and needs no GPU.

  python tests/golden/make_abi_prototypes.py [--out FILE]

The file in git was recorded at the commit before the binding was derived from the header, when all of it was written out by hand.
Run this only at a commit whose binding is meant to become the yardstick, never to make a failing test pass."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(HERE, "abi_prototypes.json"))
    a = ap.parse_args()
    from tests.test_abi_derived_cpu import bound

    out = bound()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{a.out}: {len(out['prototypes'])} product and {len(out['harness_prototypes'])} harness prototypes, "
          f"{len(out['constants'])} constants, {len(out['structs'])} structs")
    return 0


if __name__ == "__main__":
    sys.exit(main())
