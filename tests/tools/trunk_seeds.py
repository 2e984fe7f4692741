"""Seeds of tests/trunk_cases.py (CPU only): for each case, try seeds 0, 1, 2, ... and print the first at which every ReLU input of
the fp64 reference lies at least M from zero and the fp32 oracle stays within DEV_MAX of fp64, in all three modes, with the
margins reached.  The output is pasted into the case
table; a case that finds none within LIMIT seeds has to shrink (M does not).

    python tests/tools/trunk_seeds.py [case ...]"""
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(os.path.dirname(_HERE))
for _p in (os.path.join(_REPO, "mopoe-mimic_amd"), os.path.join(_REPO, "oracle"), os.path.join(_REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import trunk_cases as TC  # noqa: E402

LIMIT = 200


def first_seed(case):
    for seed in range(LIMIT):
        margins, devs = [], []
        for mode in TC.MODES:
            ref = TC.make_reference(case, seed, mode)
            margins.append(ref.margin)
            devs.append(max(ref.dev.values()))
            if margins[-1] < TC.M or devs[-1] > TC.DEV_MAX:
                break
        else:
            return seed, margins, devs
    return None, None, None


def main(names):
    for case in TC.CASES:
        if names and case.name not in names:
            continue
        seed, margins, devs = first_seed(case)
        if seed is None:
            print(f"{case.name}: no seed below {LIMIT} meets M = {TC.M:g}: shrink the case")
        else:
            print(f"{case.name}: seed {seed}  margins " + " ".join(f"{m}={v:.2e}" for m, v in zip(TC.MODES, margins))
                  + "  fp32 oracle's worst deviation " + " ".join(f"{v:.1e}" for v in devs))


if __name__ == "__main__":
    main(sys.argv[1:])
