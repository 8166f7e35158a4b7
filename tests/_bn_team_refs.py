"""Cases, plan arithmetic and shared references for the team form of the BatchNorm backward (csrc/bn.hip,
bn_bwd_team_kernel).  A plain module: nothing here touches a GPU, and nothing of tests/_bn_refs.py is changed -- the
references (R.bn_bwd, fp64), the tolerances (R.K, from the CPU restatement table of tests/test_bn_cpu.py) and the seeded
inputs (R.bn_inputs) are the ones the other BatchNorm tests use.

The plan, restated from make_bwd_plan of bn.hip: a member (one workgroup of 1024 lanes) holds cap = 1024 * 4 * NV
elements of a channel, a channel takes T = ceil(B * HW / cap) members, the persistent grid has
teams = min(C, max_wgs // T) teams of T, and team t works off channels t, t + teams, ... in rounds = ceil(C / teams)
rounds.  Without the tuning knob (NV = 8) the team form is taken for 16-byte streams with B * HW > 32768, T <= 16 and
C * T >= 128; with it (NV = 1 or 8 forced) on every 16-byte-stream shape with T <= 16 and T <= max_wgs.
"""
import functools

import _bn_refs as R

ONE_NT, MAX_T = R.ONE_NT, 16
PATHS = {"1d": 0, "one<2>": 1, "one<8>": 2, "two": 3, "team": 4}      # out[0] of vg_debug_bn_bwd_plan
MI355X_CUS = 256                                                         # what the CPU test evaluates the natural cases at


def team_plan(shape, max_wgs, forced_nv=0, aligned=True):
    """dict(path, nv, T, teams, rounds, last): what vg_bn_act_bwd launches for ``shape`` on a device of ``max_wgs``
    compute units (or the knob's cap); ``last``: the elements the last member of a channel holds."""
    B, C = shape[0], shape[1]
    HW = 1
    for d in shape[2:]:
        HW *= d
    off = dict(nv=0, T=0, teams=0, rounds=0, last=0)
    if HW == 1:
        return dict(path="1d", **off)
    total = B * HW
    vec = HW % 4 == 0 and aligned
    if not forced_nv and vec and 4 <= total <= ONE_NT * 4 * 8 and C >= 128:
        return dict(path="one<2>" if total <= ONE_NT * 4 * 2 else "one<8>", **off)
    if not vec or total < 4 or (not forced_nv and total <= ONE_NT * 4 * 8):
        return dict(path="two", **off)
    nv = forced_nv or 8
    cap = ONE_NT * 4 * nv
    T = -(-total // cap)
    if T > MAX_T or (not forced_nv and C * T < 128) or max_wgs < T:
        return dict(path="two", **off)
    teams = min(C, max_wgs // T)
    return dict(path="team", nv=nv, T=T, teams=teams, rounds=-(-C // teams), last=total - (T - 1) * cap)


# shape -> (the knob's max_wgs (0: the device's), what the case is there for: T, teams, rounds, last member's elements)
FORCED = {        # knob NV = 1: cap = 4096
    (9, 5, 32, 32): (6, dict(T=3, teams=2, rounds=3, last=1024)),       # ragged last member, an idle team in round 3
    (4, 3, 64, 64): (0, dict(T=4, teams=3, rounds=1, last=4096)),       # T members exactly, one round
    (683, 6, 3, 4): (0, dict(T=3, teams=6, rounds=1, last=4)),          # one vector in the last member, division path
    (3, 7, 64, 64): (3, dict(T=3, teams=1, rounds=7, last=4096)),       # one team, seven rounds
}
NATURAL = {       # no knob: NV = 8, cap = 32768; teams / rounds on 256 compute units
    (33, 128, 32, 32): dict(path="team", T=2, teams=128, rounds=1, last=1024),
    (65, 160, 32, 32): dict(path="team", T=3, teams=85, rounds=2, last=1024),
    (2731, 60, 3, 4): dict(path="two", T=0, teams=0, rounds=0, last=0),  # C * T = 120: the two passes, ragged vectors
}
SHAPES = tuple(FORCED) + tuple(NATURAL)


@functools.lru_cache(maxsize=None)
def saved(shape):
    """The fp64 reference's saved statistics as the backward receives them: fp32."""
    i = R.bn_inputs(shape)
    r = R.bn_coefficients_from_x(i["x"], i["gamma"], i["beta"], R.EPS, 0.1)
    return r["mean"].float(), r["invstd"].float()


@functools.lru_cache(maxsize=None)
def bwd_ref(shape, act):
    """R.bn_bwd in fp64, once per (shape, activation), shared by the CPU and the GPU tests; never modified."""
    i = R.bn_inputs(shape)
    mean, invstd = saved(shape)
    return R.bn_bwd(i["gy"], i["x"], i["gamma"], i["beta"], mean, invstd, act)
