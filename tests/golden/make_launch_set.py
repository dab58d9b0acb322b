"""Writes tests/golden/launch_set.json: the profile rows of tests/launch_set_cases.py on the library of the checkout it runs in
(an MI355X is needed).  The committed file was written on the commit before csrc/engine.hip was split.

    python tests/golden/make_launch_set.py [OUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from launch_set_cases import GROUPS, record  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "launch_set.json")
    with open(out, "w") as f:
        json.dump({g: record(g) for g in GROUPS}, f, indent=1)
    print("wrote", out)
