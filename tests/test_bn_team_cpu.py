"""The cases of tests/test_bn_team_gpu.py reach what they are named for, from the CPU alone (no GPU, no kernel):

1. The plan arithmetic of the team backward (make_bwd_plan of bn.hip, restated in _bn_team_refs.team_plan) gives every
   case the members per channel, teams, rounds and ragged last member it is listed with; the natural cases at the 256
   compute units of an MI355X.
2. The kink set of ReLU / LeakyReLU (tests/_bn_refs.py) is all but empty in every case, by the condition of _bn_refs:
   at most 1e-5 of a case's elements, none in a case of fewer than 100 000 -- from the fp64 reference alone.
"""
import pytest

import _bn_refs as R
import _bn_team_refs as T


@pytest.mark.parametrize("shape", list(T.FORCED))
def test_forced_plans(shape):
    max_wgs, want = T.FORCED[shape]
    p = T.team_plan(shape, max_wgs or T.MI355X_CUS, forced_nv=1)
    assert p["path"] == "team" and p["nv"] == 1, p
    assert {k: p[k] for k in want} == want, (shape, p)
    assert p["teams"] * p["T"] <= (max_wgs or T.MI355X_CUS)


def test_forced_cases_reach_their_edges():
    p = {s: T.team_plan(s, T.FORCED[s][0] or T.MI355X_CUS, forced_nv=1) for s in T.FORCED}
    ragged = p[(9, 5, 32, 32)]
    assert 0 < ragged["last"] < 4096 and ragged["rounds"] * ragged["teams"] > 5      # an idle team in the last round
    assert ragged["rounds"] >= 3                                                     # both granule sets are used again
    assert p[(4, 3, 64, 64)]["last"] == 4096 and p[(4, 3, 64, 64)]["rounds"] == 1
    assert p[(683, 6, 3, 4)]["last"] == 4 and (3 * 4) & (3 * 4 - 1)                  # the plane is no power of two
    assert p[(3, 7, 64, 64)]["teams"] == 1 and p[(3, 7, 64, 64)]["rounds"] == 7


@pytest.mark.parametrize("shape", list(T.NATURAL))
def test_natural_plans(shape):
    want = T.NATURAL[shape]
    p = T.team_plan(shape, T.MI355X_CUS)
    assert {k: p[k] for k in want} == want, (shape, p)
    if p["path"] == "team":
        assert p["nv"] == 8 and p["teams"] * p["T"] <= T.MI355X_CUS
    # _bn_refs.bwd_path knows the dispatch from before the team form: it calls these shapes "two"
    assert R.bwd_path(shape[0], shape[1], shape[2] * shape[3]) == "two"


def test_plan_edges():
    """The thresholds of the rule, one step to either side."""
    assert T.team_plan((32, 128, 32, 32), 256)["path"] == "one<8>"          # 32768 per channel: still one workgroup
    assert T.team_plan((128, 128, 32, 32), 256) == dict(path="team", nv=8, T=4, teams=64, rounds=2, last=32768)
    assert T.team_plan((128, 32, 64, 64), 256) == dict(path="team", nv=8, T=16, teams=16, rounds=2, last=32768)
    assert T.team_plan((129, 32, 64, 64), 256)["path"] == "two"             # 17 members
    assert T.team_plan((33, 63, 32, 32), 256)["path"] == "two"              # C * T = 126
    assert T.team_plan((33, 64, 32, 32), 256)["path"] == "team"             # C * T = 128
    assert T.team_plan((33, 128, 32, 32), 256, aligned=False)["path"] == "two"
    assert T.team_plan((33, 128, 32, 32), 1)["path"] == "two"               # a channel's members do not fit the device
    assert T.team_plan((17, 3, 64, 64), 256)["path"] == "two"               # the 64-slice case of _bn_refs stays


@pytest.mark.parametrize("shape", T.SHAPES)
def test_kink_sets_are_all_but_empty(shape):
    n = 1
    for d in shape:
        n *= d
    for act in ("relu", "lrelu"):
        kinks = int(T.bwd_ref(shape, act)["kink"].sum())
        print(f"{shape} {act}: {kinks} kink elements of {n} ({kinks / n:.1e})")
        assert kinks <= 1e-5 * n, (shape, act, kinks)
        if n < 100_000:
            assert kinks == 0, (shape, act, kinks)
    assert int(T.bwd_ref(shape, "none")["kink"].sum()) == 0
