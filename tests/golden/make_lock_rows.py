"""Writes tests/golden/lock_rows.json: the compressed keys [s] H of the full-size scalars in the 64-share
rows of the lock check's tests (tests/gpu_helpers/lock_check.py big_rows), computed by the oracle alone.

    python tests/golden/make_lock_rows.py

tests/test_lock_check_oracle.py recomputes a sample of the entries and checks that none is missing.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests", "gpu_helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lock_check as lc  # noqa: E402


def main():
    keys = {}
    for n, t in lc.BIG_SHAPES:
        for _, scalars, _ in lc.big_rows(n, t):
            for s in scalars:
                if s.bit_length() > 64:
                    keys[hex(s)] = lc.key(s, cached=False).hex()
    with open(lc.GOLDEN_ROWS, "w") as f:
        json.dump({"h_scalar": hex(lc.H_SCALAR), "keys": dict(sorted(keys.items()))}, f, indent=0)
        f.write("\n")
    print(f"{len(keys)} keys -> {lc.GOLDEN_ROWS}")


if __name__ == "__main__":
    main()
