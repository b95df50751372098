"""Runs named subsets of the device-primitive case lists (tests/device_prims.py) in a
process of its own: the environment forms of the radix segment (SH_RADIX_XCD,
SH_RADIX10, SH_SEG_LASTCARRY, SH_SEG_SMALL) are read once per process, so each is
tested in a fresh child (tests/test_gpu_device_prims.py).

    python tests/device_prims_child.py SUBSET [SUBSET ...]      (`all`: every subset)

Exits 1 on the first mismatch, printing the case."""
import os
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import device_prims as dp  # noqa: E402


def main(argv):
    names = [s for s in dp.SUBSETS if s not in ("small", "large", "radix10")] if argv == ["all"] else argv
    case = [""]

    def report(s):
        case[0] = s

    done = 0
    for name in names:
        try:
            dp.run_subset(name, report)
        except AssertionError:
            traceback.print_exc()
            print("MISMATCH in", case[0], flush=True)
            return 1
        done += 1
    print(f"ok: {done} subsets ({' '.join(names)})", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
