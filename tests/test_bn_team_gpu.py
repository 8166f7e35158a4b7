"""The team form of the BatchNorm backward (csrc/bn.hip, bn_bwd_team_kernel: a channel larger than one workgroup's
registers is held by T cooperating workgroups, one pass over x and gy) through ops.bn_act_bwd, judged as
tests/test_bn_gpu.py judges the other paths: gx, dgamma, dbeta per element against the fp64 reference R.bn_bwd with the
tolerances R.K (from the CPU restatement table; nothing measured from a kernel), the emitted gx_amax exactly, for the
three activations, with and without the accumulate flag.

Forced cases (tuning library, vg_debug_set_bn_team(1, max_wgs): 4096 elements per member) are the smallest shapes that
reach each edge of the team kernel; the natural cases run the product rule (32768 per member); tests/test_bn_team_cpu.py
shows from the CPU that each case has the members, rounds and ragged last member it is listed for, and here the library
is asked for its own plan (vg_debug_bn_bwd_plan) and has to agree.  After every call the status word of the exchange
block is 0 (no sweep gave up).  Two calls give the same bits; a captured and replayed call gives the eager call's bits
(the zeroing node clears the granules again before the replay's kernel), also on the second replay with other
launches in between.
"""
import ctypes

import pytest
import torch

import _bn_refs as R
import _bn_team_refs as T
from test_bn_gpu import check

pytestmark = pytest.mark.gpu

CASES = [(s, 1, T.FORCED[s][0]) for s in T.FORCED] + [(s, 0, 0) for s in T.NATURAL]


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import _lib, ops
    with _lib.use_tuning() as lib:
        try:
            yield ops, lib
        finally:
            lib.vg_debug_set_bn_team(0, 0)


def device_plan(lib, shape, gy, x):
    B, C, HW = shape[0], shape[1], shape[2] * shape[3]
    out = (ctypes.c_int * 5)()
    assert lib.vg_debug_bn_bwd_plan(B, C, HW, gy.data_ptr(), x.data_ptr(), x.data_ptr(), out) == 0
    return list(out)


def status_word(ops, lib, C, device):
    """First word of the BatchNorm workspace of the current stream: the team kernel's status (0: no sweep gave up)."""
    return int(ops.workspace(lib.vg_bn_workspace_bytes(C), device)[:4].view(torch.int32))


def exact_amax(ops, gx, what):
    slot = ops.known_amax(gx)
    assert slot is not None, what
    assert float(slot) == float(gx.abs().max()), (what, float(slot), float(gx.abs().max()))


@pytest.mark.parametrize("act", list(R.ACTS))
@pytest.mark.parametrize("shape,nv,max_wgs", CASES, ids=[f"{s}-nv{n}-wgs{w}" for s, n, w in CASES])
def test_bn_team_bwd(H, shape, nv, max_wgs, act):
    ops, lib = H
    assert lib.vg_debug_set_bn_team(nv, max_wgs) == 0
    i = R.bn_inputs(shape)
    C, code = shape[1], R.ACTS[act]
    gy, x, gamma, beta = (i[n].cuda() for n in ("gy", "x", "gamma", "beta"))
    mean, invstd = (t.cuda() for t in T.saved(shape))
    cus = torch.cuda.get_device_properties(x.device).multi_processor_count
    want = T.team_plan(shape, min(max_wgs, cus) if max_wgs else cus, forced_nv=nv)
    got = device_plan(lib, shape, gy, x)
    assert got == [T.PATHS[want["path"]], want["nv"], want["T"], want["teams"], want["rounds"]], (shape, got, want)
    listed = T.FORCED[shape][1] if nv else T.NATURAL[shape]
    assert want["path"] == listed.get("path", "team"), (shape, want)
    if cus == T.MI355X_CUS or nv:
        assert {k: want[k] for k in listed} == listed, (shape, want, listed)
    team = want["path"] == "team"

    ref = T.bwd_ref(shape, act)
    what = f"bn_act_bwd (team) {shape} nv={nv} max_wgs={max_wgs} {act}"
    gx, dgamma, dbeta = ops.bn_act_bwd(gy, x, gamma, beta, mean, invstd, code)
    if team:
        assert status_word(ops, lib, C, x.device) == 0, what + ": a sweep gave up"
    check(gx, ref, "gx", what), check(dgamma, ref, "dgamma", what), check(dbeta, ref, "dbeta", what)
    exact_amax(ops, gx, what)

    # a second identical call: the sums do not depend on timing
    gx2, dgamma2, dbeta2 = ops.bn_act_bwd(gy, x, gamma, beta, mean, invstd, code)
    assert torch.equal(gx2, gx) and torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta), what + ": a second call differs"
    gx3, none_g, none_b = ops.bn_act_bwd(gy, x, gamma, beta, mean, invstd, code, need_param_grads=False)
    assert none_g is None and none_b is None and torch.equal(gx3, gx), what + ": need_param_grads=False changes gx"

    # the accumulate flag: dgamma / dbeta are added to what is there, gx and its bound are what they were
    g0, b0 = R.randn(C, seed=31).cuda(), R.randn(C, seed=32).cuda()
    acc_g, acc_b = g0.clone(), b0.clone()
    gx4, rg, rb = ops.bn_act_bwd(gy, x, gamma, beta, mean, invstd, code, accumulate_into=(acc_g, acc_b))
    assert rg is acc_g and rb is acc_b and torch.equal(gx4, gx), what + ": accumulate_into changes gx"
    assert torch.equal(acc_g, dgamma + g0) and torch.equal(acc_b, dbeta + b0), what + ": accumulate_into does not add exactly"
    exact_amax(ops, gx4, what + " (accumulate)")
    if team:
        assert status_word(ops, lib, C, x.device) == 0, what + ": a sweep gave up"

    # captured once, replayed twice: the eager call's bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.bn_act_bwd(gy, x, gamma, beta, mean, invstd, code)         # warm-up on the capture stream: its workspace
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with ops.amax_capture_scope(), torch.cuda.graph(graph, stream=side):
        cgx, cdg, cdb = ops.bn_act_bwd(gy, x, gamma, beta, mean, invstd, code)
    keep, cslot = ops.buffers_in_use(), ops.known_amax(cgx)
    assert cslot is not None, what
    for _ in range(2):
        cgx.zero_(), cdg.zero_(), cdb.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cgx, gx) and torch.equal(cdg, dgamma) and torch.equal(cdb, dbeta), what + ": the replay differs"
        assert float(cslot) == float(gx.abs().max()), what + ": the replay's gx_amax"
        if team:
            with torch.cuda.stream(side):
                assert status_word(ops, lib, C, x.device) == 0, what + ": a sweep gave up in the replay"
    del keep, graph
