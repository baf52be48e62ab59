"""Record tests/golden/loss_bytes.json: what the loss passes write, byte for byte, for the cases of tests/loss_bytes_cases.py.

Run ONCE, on one MI355X, with S2D_LIBRARY naming a build of the commit before a change of the loss kernels -- never the tree
under test, whose bytes tests/test_gpu_loss_bytes.py then compares with the record:

    S2D_LIBRARY=build/libsplat2d_hip_parent.so python tools/record_loss_bytes.py [--out tests/golden/loss_bytes.json]

(the library: `_build.build_experiment("parent", csrc=<a checkout of that commit's csrc>)`).

Without S2D_LIBRARY it refuses, unless --tree says that the tree's own library is meant (to look at a difference, into
another file).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import loss_bytes_cases as LB
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=LB.FIXTURE)
    ap.add_argument("--tree", action="store_true", help="record the tree's own library (not a fixture: name another --out)")
    a = ap.parse_args()
    if not os.environ.get("S2D_LIBRARY") and not (a.tree and os.path.abspath(a.out) != LB.FIXTURE):
        sys.exit("S2D_LIBRARY does not name a build of the parent commit: the fixture is never recorded from the code under test")
    cases = {LB.group_key(*g): LB.evaluate(*g) for g in LB.GROUPS}
    LB.write_fixture(cases, a.out)
    print("%d groups of %d weightings -> %s" % (len(cases), len(LB.WEIGHTINGS), a.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
