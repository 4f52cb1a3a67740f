"""What the closed-loop entry points refuse, and with which words, is what tests/golden/closed_loop_refusals.json recorded: the
grid of tests/closed_loop_refusal_cases.py, replayed without a GPU.  The file is regenerated with
`python -m tests.closed_loop_refusal_cases`; a change of it is a change of behaviour and is reviewed as one."""
import json

import pytest

from tests import closed_loop_refusal_cases as rc


@pytest.fixture(scope="module")
def replayed():
    return rc.all_cases()


def test_the_grid_is_the_recorded_one(replayed):
    recorded = json.loads(rc.GOLDEN.read_text())
    assert sorted(replayed) == sorted(recorded)
    assert len(recorded) > 1800


def test_every_outcome_is_the_recorded_one(replayed):
    recorded = json.loads(rc.GOLDEN.read_text())
    differ = {cid: (recorded[cid], got) for cid, got in replayed.items() if recorded.get(cid) != got}
    assert not differ, f"{len(differ)} of {len(replayed)} outcomes differ, the first: {next(iter(differ.items()))}"


def test_the_grid_covers_every_entry_and_both_sides_of_every_limit(replayed):
    for name in rc.METHODS:
        py = {cid: v for cid, v in replayed.items() if cid.startswith(f"py/{name}/")}
        c = {cid: v for cid, v in replayed.items() if cid.startswith(f"c/{name}/")}
        sizes = [v for cid, v in py.items() if "/size-" in cid and cid.endswith("/validator")]
        assert {v[0] for v in sizes} == {"ok", "raise"}, name                       # served and refused shapes
        assert {v[1] for cid, v in c.items() if "/size-" in cid and "bad-argument" not in cid} == {0, -2}, name
        assert all(v[0] == "raise" and v[1] == "ValueError" for cid, v in py.items() if not cid.endswith("/validator") and "/good" not in cid
                   and "trusted" not in cid), name
        assert py[f"py/{name}/good"][0] == "ok" and c[f"c/{name}/good"] == ["rc", 0, ""], name
    assert all(v[:2] == ["raise", "ValueError"] for cid, v in replayed.items() if cid.startswith("loop/"))
    # no case is answered by a device, or by the lack of one
    assert not [cid for cid, v in replayed.items() if v[0] == "rc" and v[1] not in (0, -1, -2)]
