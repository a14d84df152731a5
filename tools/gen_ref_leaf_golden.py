"""Writes tests/golden/ref_leaf_v1.json: the outputs of the reference's own header-only leaf functions (oracle/_ref/libref_leaf.so,
built by `make -C oracle ref` where the reference sources are present), recorded so that tests/test_oracle_column.py can hold the
oracle to them on every machine.

    python tools/gen_ref_leaf_golden.py            # regenerate from oracle/_ref
    python tools/gen_ref_leaf_golden.py --check    # recompute and compare with the committed file, exit 1 on any difference

Values are C99 hex floats (exact).  Inputs: the salinities of the test, 200 seeded draws in [0, 45) plus 0, 32 and 35 g/kg.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "ref_leaf_v1.json")
# the order of ref_constant(k) in oracle/ref_leaf_driver.cpp
CONSTANTS = ["PhysicalConstants::sigma", "Ice::cp", "Ice::epsilon", "Ice::kappa", "Ice::Lf", "Ice::rho", "Ice::rhoSnow", "Ice::s", "Ice::Tm",
             "Air::cp", "Air::Ra", "Vapour::cp", "Vapour::Lv0", "Vapour::Ra", "Water::cp", "Water::Lf", "Water::mu", "Water::rhoOcean",
             "Water::Tf", "Nextsim::kelvin(0.)"]


def salinities():
    return [float(s) for s in np.random.default_rng(7).uniform(0, 45, 200)] + [0.0, 32.0, 35.0]


def compute(R):
    sss = salinities()
    return {"title": "outputs of the reference's header-only freezing-point models and constants (oracle/ref_leaf_driver.cpp), C99 hex floats",
            "sss": [s.hex() for s in sss],
            "freezing_linear": [R.ref_freezing_linear(s).hex() for s in sss],
            "freezing_unesco": [R.ref_freezing_unesco(s).hex() for s in sss],
            "constants": [{"name": n, "value": R.ref_constant(k).hex()} for k, n in enumerate(CONSTANTS)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    R = O.ref_leaf()
    if R is None:
        raise SystemExit("oracle/_ref/libref_leaf.so is not built (make -C oracle ref, with the reference sources present)")
    d = compute(R)
    if args.check:
        same = json.load(open(PATH)) == d
        print("ref_leaf_v1.json %s" % ("matches" if same else "DIFFERS"))
        sys.exit(0 if same else 1)
    with open(PATH, "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")
    print("wrote", PATH)


if __name__ == "__main__":
    main()
