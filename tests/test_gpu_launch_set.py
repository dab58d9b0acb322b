"""Launch-set identity: for a fixed list of calls (tests/launch_set_cases.py) the library issues exactly the launches recorded in
tests/golden/launch_set.json -- kernel and role names, call counts, and the flops / bytes doubles the host computes for each,
compared with ==.  The recording was made before csrc/engine.hip was split into handle.h / towers.hip / heads.hip: a refactor of
the host code that drops, adds, reorders into another kernel or re-sizes a launch shows here."""
import json
import os

import pytest

from launch_set_cases import GROUPS, record

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_set.json")) as _f:
    RECORDED = json.load(_f)


def test_recording_covers_every_group():
    assert set(RECORDED) == set(GROUPS)
    assert all(rows for cases in RECORDED.values() for rows in cases.values())


@pytest.mark.parametrize("group", GROUPS)
def test_launch_set_is_the_recorded_one(group):
    got, want = record(group), RECORDED[group]
    assert sorted(got) == sorted(want)
    for case in want:
        assert got[case] == want[case], (case, got[case], want[case])
