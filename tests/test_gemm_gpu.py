"""The Linear fp16x3 GEMM of csrc/gemm_split.hip (vg_gemm_nt_f16x3, vg_gemm_nt_f16x3_grouped) per element at every
dispatch edge, through ops._gemm_nt / ops._gemm_nt_grouped (explicit strides, bounds and output) and, at the end,
through ops.linear_fwd / linear_dgrad / linear_wgrad.

Every case: the output is a window of a NaN-filled buffer and the stream's workspace is filled with NaN bytes before the
launch; afterwards the guards around the window are still NaN, every element inside is finite and

    |got - emul64| <= k_acc(K, splits) 2^-24 mag        per element, no element excluded

with emul64 (tests/_gemm_refs.py) the fp64 value of the three plane products for the very bounds the kernel was handed and
mag = |A| |B|^T + |bias|; a second launch returns the same bits.  K_ACC comes from the fp32 restatement measured in
tests/test_gemm_cpu.py, which also shows that the same check rejects each of the mutations listed in _gemm_refs at the
inputs used here.  Nothing in the tolerance is taken from a kernel run.  Every case prints its worst ratio (pytest -s)
before it asserts; the module prints the worst per edge and what it covered at its end.

All four layouts: fwd (both reductions contiguous), dgrad (B strided), wgrad (both strided) and atbc (A strided, B
contiguous: compiled and reachable through the C ABI, used by no ops function).
"""
import ctypes

import pytest
import torch

import _gemm_refs as R
from test_losses_gpu import at_offset

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64                    # floats of NaN on either side of an output window
WORST, COVER = {}, {"layouts": set(), "stages per split": set(), "splits": set()}


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    yield ops
    print(f"\nedge                 worst on the device (2^-24)   K_ACC = {R.K_ACC} (capped at 3 K + splits)")
    for edge, w in WORST.items():
        print(f"{edge:<22}{w:>10.2f}")
    for what, s in COVER.items():
        print(f"{what}: {sorted(s)}")


def dev_bound(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


def window(M, N, off=0):
    """(buffer, start): a NaN-filled buffer whose floats [start, start + M N) are the output, `off` floats past a
    16-byte boundary."""
    buf = torch.full((2 * GUARD + M * N + 8,), NAN, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, GUARD + off


def bits(t):
    return t.contiguous().view(torch.int32)


def poison_workspace(H, need):
    ws = H.workspace(max(need, 1), torch.device("cuda", torch.cuda.current_device()))
    ws.fill_(0xFF)             # every float of it a NaN
    return ws


def launch(H, lib, As, B, bias, M, N, K, st, a_bounds, b_bound, c_off=0, grouped=False):
    """Two launches into fresh NaN windows (the workspace NaN each time): guards intact, same bits.  Returns the list
    of outputs on the CPU."""
    G = len(As)
    need = (lib.vg_gemm_nt_f16x3_grouped_workspace_bytes(G, M, N, K) if grouped
            else lib.vg_gemm_nt_f16x3_workspace_bytes(M, N, K))
    outs = []
    for _ in range(2):
        poison_workspace(H, need)
        wins = [window(M, N, c_off) for _ in range(G)]
        Cs = [buf[s:s + M * N].view(M, N) for buf, s in wins]
        assert all(c.data_ptr() % 16 == 4 * (c_off % 4) for c in Cs)
        if grouped:
            H._gemm_nt_grouped(As, B, bias, Cs, M, N, K, *st, a_bounds, b_bound)
        else:
            H._gemm_nt(As[0], B, bias, Cs[0], M, N, K, *st, a_bounds[0], b_bound)
        for buf, s in wins:
            assert bool(torch.isnan(buf[:s]).all()) and bool(torch.isnan(buf[s + M * N:]).all()), "guard overwritten"
        outs.append([c.clone() for c in Cs])
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b)), "a second launch returned other bits"
    return [c.cpu() for c in outs[0]]


def record(layout, M, N, K, lib):
    ks = R.ksplit_of(M, N, K)
    assert ks == max(lib.vg_gemm_nt_f16x3_workspace_bytes(M, N, K) // (4 * M * N), 1)
    COVER["layouts"].add(layout)
    COVER["splits"].add(ks)
    COVER["stages per split"].add(K // ks // R.GKC)
    return ks


def judge(got, A, B, bias, a_bound, b_bound, edge, what, rows=None):
    """The per-element check of one output against emul64 at the bounds the kernel was handed."""
    M, K = A.shape
    ks = R.ksplit_of(M, B.shape[0], K)
    ref, m = R.emul64(A, B, bias, a_bound, b_bound), R.mag(A, B, bias)
    if rows is not None:
        got, ref, m = got[rows], ref[rows], m[rows]
    ok, w = R.check(got, ref, m, R.k_acc(K, ks))
    if w == w:
        WORST[edge] = max(WORST.get(edge, 0.0), w)
    print(f"{edge} {what}: worst {w:.2f} x 2^-24 (K = {R.k_acc(K, ks)})")
    assert ok, (f"{edge} {what}: off by more than {R.k_acc(K, ks)} x 2^-24 x magnitude (worst {w:.2f}), or not finite; "
                f"first at {(~(((got.double() - ref).abs()) <= R.k_acc(K, ks) * R.U * m)).nonzero()[0].tolist()}")


def run_case(H, lib, layout, M, N, K, edge, bias=True, loose=(0, 0), seed=0, c_off=0, **kw):
    """One single-call case from the shared operands: launch twice, judge."""
    A, B, bv = R.matrices(M, N, K, seed, **kw)
    ab, bb = R.bound_of(A) * 2.0 ** loose[0], R.bound_of(B) * 2.0 ** loose[1]
    ks = record(layout, M, N, K, lib)
    bv = bv if bias else None
    got, = launch(H, lib, [R.as_stored(layout, A, "A").cuda()], R.as_stored(layout, B, "B").cuda(),
                  None if bv is None else bv.cuda(), M, N, K, R.strides_of(layout, M, N, K), [dev_bound(ab)],
                  dev_bound(bb), c_off)
    judge(got, A, B, bv, ab, bb, edge, f"{layout} M {M} N {N} K {K} splits {ks} bias {bias} loose {loose}")
    return got


@pytest.fixture(scope="module")
def lib():
    from disentangle_mlp_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------- the edges
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_stage_counts_without_a_split(H, lib, layout):
    """nst = 1..7 on one partial tile: the prologue with fewer stages than register slots, a whole unrolled trip of
    G_PD = 3 and both tail branches."""
    nst = set()
    for K in R.STAGE_KS:
        assert R.ksplit_of(*R.STAGE_MN, K) == 1
        nst.add(K // R.GKC)
        for bias in (False, True):
            run_case(H, lib, layout, *R.STAGE_MN, K, "stage counts", bias)
    assert nst == {1, 2, 3, 4, 5, 6, 7}


@pytest.mark.parametrize("M,N", R.SPLIT_MNS, ids=["one tile", "four tiles"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_k_split(H, lib, layout, M, N):
    """2 and 4 splits (plain mapping), 8 (XCD mapping, j / per == 0), 16 and 32 (j / per >= 1), per > 1 at four tiles;
    8, 10 and 12 stages per split (tails 2, 1, 0); bias on and off.  The split count is the workspace query's."""
    cover = set()
    for K in R.SPLIT_KS:
        ks = R.ksplit_of(M, N, K)
        assert lib.vg_gemm_nt_f16x3_workspace_bytes(M, N, K) == 4 * ks * M * N and ks > 1
        cover.add((ks, K // ks // R.GKC))
        for bias in (False, True):
            run_case(H, lib, layout, M, N, K, "K split", bias)
    assert cover == R.SPLIT_COVER, cover      # a change of the heuristic must not silently empty this test
    assert max(k for k, _ in cover) >= 32


@pytest.mark.parametrize("K", R.RAGGED_KS, ids=["unsplit", "split"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_ragged_tiles(H, lib, layout, K):
    """M of {1, 127, 128, 129} x N of {1, 3, 127, 128, 129, 257}, each with a whole and with a ragged partner."""
    assert {m for m, _ in R.RAGGED_MN} == {1, 127, 128, 129} and {n for _, n in R.RAGGED_MN} == {1, 3, 127, 128, 129, 257}
    for (M, N) in R.RAGGED_MN:
        assert (R.ksplit_of(M, N, K) > 1) == (K == R.RAGGED_KS[1])
        for bias in (False, True):
            run_case(H, lib, layout, M, N, K, "ragged tiles", bias)


@pytest.mark.parametrize("shape", [R.SMALL, R.SMALL_SPLIT], ids=["unsplit", "split"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_loose_bounds(H, lib, layout, shape):
    """The bound is an UPPER bound: exact, and loose by 2^1, 2^5, 2^10 on A only, on B only and on both."""
    for l in (0,) + R.LOOSE:
        for loose in ((l, 0), (0, l), (l, l)) if l else ((0, 0),):
            for bias in (False, True):
                run_case(H, lib, layout, *shape, "loose bounds", bias, loose)


@pytest.mark.parametrize("shape", [R.SMALL, R.SMALL_SPLIT], ids=["unsplit", "split"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_grouped_bounds_decades_apart(H, lib, layout, shape):
    """The grouped entry at G = 3, the groups' bounds decades apart on either side of group 0's: each group against
    emul64 at its own bound.  (Without the bias, which is most of `mag` next to the small group; and with it.)"""
    M, N, K = shape
    _, B, bv = R.matrices(M, N, K)
    As = [R.matrices(M, N, K, seed=10 + g)[0] * s for g, s in enumerate(R.GROUP_SCALES)]
    bounds, bb = [R.bound_of(a) for a in As], R.bound_of(B)
    assert bounds[1] > 100 * bounds[0] > 1e4 * bounds[2]
    record(layout, M, N, K, lib)
    for bias in (None, bv):
        gots = launch(H, lib, [R.as_stored(layout, a, "A").cuda() for a in As], R.as_stored(layout, B, "B").cuda(),
                      None if bias is None else bias.cuda(), M, N, K, R.strides_of(layout, M, N, K),
                      [dev_bound(b) for b in bounds], dev_bound(bb), grouped=True)
        for g, got in enumerate(gots):
            judge(got, As[g], B, bias, bounds[g], bb, "grouped bounds", f"{layout} {shape} group {g} bias {bias is not None}")


@pytest.mark.parametrize("shape", [R.SMALL, R.SMALL_SPLIT], ids=["unsplit", "split"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_zero_operand(H, lib, layout, shape):
    """All-zero A with bound 0 (the largest scale), then all-zero B: the output is exactly the bias, or exactly 0."""
    M, N, K = shape
    A, B, bv = R.matrices(M, N, K)
    record(layout, M, N, K, lib)
    for zero in "AB":
        a, b = (torch.zeros_like(A), B) if zero == "A" else (A, torch.zeros_like(B))
        for bias in (None, bv):
            got, = launch(H, lib, [R.as_stored(layout, a, "A").cuda()], R.as_stored(layout, b, "B").cuda(),
                          None if bias is None else bias.cuda(), M, N, K, R.strides_of(layout, M, N, K),
                          [dev_bound(R.bound_of(a))], dev_bound(R.bound_of(b)))
            want = torch.zeros(M, N) if bias is None else bias[None, :].expand(M, N)
            assert torch.equal(got, want), (layout, shape, zero, bias is not None)


def _floor(t, lo):
    """|t| raised to at least lo: no element of the scaled operand is an fp32 subnormal."""
    return torch.where(t.abs() < lo, torch.copysign(torch.full_like(t, lo), t), t)


CLAMPS = {                    # name: (A's factor, B's factor)
    "2^-100 x 2^100": (2.0 ** -100, 2.0 ** 100),
    "2^100 x 2^-100": (2.0 ** 100, 2.0 ** -100),
    "2^-60 x 2^-56": (2.0 ** -60, 2.0 ** -56),
    "2^-115 x 2^100 (exponent clamped to 15)": (2.0 ** -115, 2.0 ** 100),
}


@pytest.mark.parametrize("case", list(CLAMPS))
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_exponent_range(H, lib, layout, case):
    """Operands at the ends of the exponent range, the true result a normal fp32 number: the epilogue's acc * ua * ub
    must not lose the result's bits to a subnormal or infinite intermediate.  In the last case A's bound (about
    2^-113) lies under the clamp of f16_bound_exp: A is scaled by 2^126, the largest scale, and keeps its 22 bits."""
    fa, fb = CLAMPS[case]
    for shape in (R.SMALL, R.SMALL_SPLIT):
        M, N, K = shape
        A, B, bv = R.matrices(M, N, K, decades=0)
        A, B, bv = _floor(A, 2.0 ** -6) * fa, _floor(B, 2.0 ** -10) * fb, _floor(bv, 2.0 ** -6) * (fa * fb)
        ab, bb = R.bound_of(A), R.bound_of(B)
        assert ("clamped" in case) == (R.bound_exp(ab) == 15 and ab < 2.0 ** -112)
        tiny = float(torch.finfo(torch.float32).tiny)
        assert float(A.abs().min()) >= tiny and float(B.abs().min()) >= tiny and float(R.mag(A, B).min()) >= tiny
        record(layout, M, N, K, lib)
        for bias in (None, bv):
            got, = launch(H, lib, [R.as_stored(layout, A, "A").cuda()], R.as_stored(layout, B, "B").cuda(),
                          None if bias is None else bias.cuda(), M, N, K, R.strides_of(layout, M, N, K),
                          [dev_bound(ab)], dev_bound(bb))
            judge(got, A, B, bias, ab, bb, "exponent range", f"{layout} {shape} {case} bias {bias is not None}")


@pytest.mark.parametrize("value", [NAN, float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_nonfinite_data_reaches_its_row_or_column(H, lib, layout, value):
    """One NaN / Inf element in row m of A (its bound inf, as vg_absmax would leave it): every output of row m is
    non-finite; one in row n of B: every output of column n.  The rest may be anything."""
    for shape in (R.SMALL, R.SMALL_SPLIT):
        M, N, K = shape
        A, B, bv = R.matrices(M, N, K)
        record(layout, M, N, K, lib)
        for which, r, k in (("A", M // 3, K - 7), ("B", N - 1, 5)):
            a, b = A.clone(), B.clone()
            (a if which == "A" else b)[r, k] = value
            ab = float("inf") if which == "A" else R.bound_of(A)
            bb = float("inf") if which == "B" else R.bound_of(B)
            got, = launch(H, lib, [R.as_stored(layout, a, "A").cuda()], R.as_stored(layout, b, "B").cuda(), bv.cuda(),
                          M, N, K, R.strides_of(layout, M, N, K), [dev_bound(ab)], dev_bound(bb))
            hit = got[r, :] if which == "A" else got[:, r]
            assert not bool(torch.isfinite(hit).any()), (layout, shape, which, value, int(torch.isfinite(hit).sum()))


@pytest.mark.parametrize("shape", [R.SMALL, R.ENTRY_SHAPES[0], R.SMALL_SPLIT], ids=str)
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_nan_in_the_last_row_stays_there(H, lib, layout, shape):
    """Ragged M: the clamped re-reads duplicate the last row of A into the tile's padding.  A NaN there (the bound is
    that of the finite elements) fills its own output row and no other: the other rows pass the per-element check."""
    M, N, K = shape
    assert M % R.TILE
    A, B, bv = R.matrices(M, N, K)
    a = A.clone()
    a[M - 1, 3] = NAN
    ab, bb = R.bound_of(A), R.bound_of(B)
    record(layout, M, N, K, lib)
    got, = launch(H, lib, [R.as_stored(layout, a, "A").cuda()], R.as_stored(layout, B, "B").cuda(), bv.cuda(),
                  M, N, K, R.strides_of(layout, M, N, K), [dev_bound(ab)], dev_bound(bb))
    assert bool(torch.isnan(got[M - 1]).all())
    judge(got, A, B, bv, ab, bb, "NaN in the last row", f"{layout} {shape}", rows=slice(0, M - 1))


def place(t, extra, off=0, col0=0):
    """The stored operand t inside a NaN-filled buffer: rows `extra` floats longer than t's, the first element `off`
    floats past a 16-byte boundary and `col0` columns into its row.  Returns (view, row pitch)."""
    r, c = t.shape
    pitch = c + extra
    flat = torch.full((r * pitch + 8 + off,), NAN, device="cuda")
    assert flat.data_ptr() % 16 == 0
    v = flat[off:off + r * pitch].view(r, pitch)[:, col0:col0 + c]
    v.copy_(t)
    return v, pitch


@pytest.mark.parametrize("shape", [R.SMALL, R.SMALL_SPLIT], ids=["unsplit", "split"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_pointers_and_row_strides(H, lib, layout, shape):
    """Row-strided operands and the output at 1, 2, 3 floats off a 16-byte boundary (a k-contiguous operand must be
    aligned: it stays so); then row strides wider than the matrix: a strided operand with a pitch of its row count
    + 5, a k-contiguous one as a column window (from column 4) of a matrix 8 columns wider.  What surrounds an operand
    is NaN: a read outside it shows in the output."""
    M, N, K = shape
    A, B, bv = R.matrices(M, N, K)
    ab, bb = R.bound_of(A), R.bound_of(B)
    at, bt = layout in ("wgrad", "atbc"), layout in ("dgrad", "wgrad")
    sa, sb = R.as_stored(layout, A, "A"), R.as_stored(layout, B, "B")
    record(layout, M, N, K, lib)
    for off in (1, 2, 3):
        a = at_offset(sa.cuda(), off) if at else sa.cuda()
        b = at_offset(sb.cuda(), off) if bt else sb.cuda()
        assert a.data_ptr() % 16 == (4 * off if at else 0) and b.data_ptr() % 16 == (4 * off if bt else 0)
        got, = launch(H, lib, [a], b, bv.cuda(), M, N, K, R.strides_of(layout, M, N, K), [dev_bound(ab)], dev_bound(bb),
                      c_off=off)
        judge(got, A, B, bv, ab, bb, "pointers and strides", f"{layout} {shape} offset {off}")
    for off in (0, 1):        # wide rows, aligned and (the strided operands) one float off
        a, pa = place(sa.cuda(), 5, off) if at else place(sa.cuda(), 8, 0, 4)
        b, pb = place(sb.cuda(), 5, off) if bt else place(sb.cuda(), 8, 0, 4)
        st = R.strides_of(layout, M, N, K, pa, pb)
        assert st != R.strides_of(layout, M, N, K)
        got, = launch(H, lib, [a], b, bv.cuda(), M, N, K, st, [dev_bound(ab)], dev_bound(bb))
        judge(got, A, B, bv, ab, bb, "pointers and strides", f"{layout} {shape} wide rows, offset {off}")


# ------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(H, lib):
    """VG_ERR_BAD_ARG (-1) / VG_ERR_WORKSPACE (-2) on the host, before any launch: the NaN-filled output stays NaN."""
    M, N, K = R.SMALL_SPLIT
    big = torch.zeros(4 * (M + N) * (K + 64) + 64, device="cuda")      # room for every operand below
    assert big.data_ptr() % 16 == 0
    one = dev_bound(1.0)
    C = torch.full((M, N), NAN, device="cuda")
    need = lib.vg_gemm_nt_f16x3_workspace_bytes(M, N, K)
    assert need > 0
    ws = poison_workspace(H, need)
    p, stream = big.data_ptr(), torch.cuda.current_stream().cuda_stream

    def single(A=p, B=p, K_=K, st=(K, 1, K, 1), ws_bytes=need):
        return lib.vg_gemm_nt_f16x3(A, B, None, C.data_ptr(), M, N, K_, *st, one.data_ptr(), one.data_ptr(),
                                    ws.data_ptr(), ws_bytes, stream)

    def grouped(G):
        ptrs = ctypes.c_void_p * 4
        return lib.vg_gemm_nt_f16x3_grouped(G, ptrs(p, p, p, p), p, None, ptrs(*([C.data_ptr()] * 4)), M, N, K, K, 1, K, 1,
                                            ptrs(*([one.data_ptr()] * 4)), one.data_ptr(), ws.data_ptr(), 3 * need, stream)

    refused = {
        "K not a multiple of 32": (single(K_=K - 24, st=(K - 24, 1, K - 24, 1)), -1),
        "K = 16": (single(K_=16, st=(16, 1, 16, 1)), -1),
        "k-contiguous A off 16 bytes": (single(A=p + 4), -1),
        "k-contiguous B off 16 bytes": (single(B=p + 8), -1),
        "k-contiguous B off 16 bytes, A strided": (single(B=p + 12, st=(1, M, K, 1)), -1),
        "k-contiguous A, row stride K + 2": (single(st=(K + 2, 1, K, 1)), -1),
        "k-contiguous B, row stride K + 1": (single(st=(K, 1, K + 1, 1)), -1),
        "k-contiguous B, row stride K + 2, A strided": (single(st=(1, M, K + 2, 1)), -1),
        "neither stride of A is 1": (single(st=(K, 2, K, 1)), -1),
        "workspace one byte short": (single(ws_bytes=need - 1), -2),
        "no workspace": (single(ws_bytes=0), -2),
        "0 groups": (grouped(0), -1),
        "4 groups": (grouped(4), -1),
    }
    torch.cuda.synchronize()
    assert {k: rc for k, (rc, _) in refused.items()} == {k: want for k, (_, want) in refused.items()}
    assert bool(torch.isnan(C).all())
    # ... and the same arguments without the flaw are taken
    assert single() == 0 and grouped(3) == 0
    torch.cuda.synchronize()
    assert bool((C == 0).all())


# ------------------------------------------------------------------------------------------------ the ops entry points
@pytest.mark.parametrize("shape", R.ENTRY_SHAPES, ids=["ragged", "split"])
def test_ops_entry_points(H, lib, shape):
    """linear_fwd, linear_dgrad and linear_wgrad on one ragged and one split GEMM each, against emul64 at the bounds they
    used: amax_of leaves its slot on the activation, weight_bound measures the weight."""
    M, N, K = shape
    A, B, bv = R.matrices(M, N, K)
    need = lib.vg_gemm_nt_f16x3_workspace_bytes(M, N, K)
    assert (need > 0) == (shape == R.ENTRY_SHAPES[1])

    poison_workspace(H, need)
    x, w = A.cuda(), B.cuda()                                        # x (M, K), w (N, K)
    y = H.linear_fwd(x, w, bv.cuda())
    ab, bb = float(H.amax_of(x)), float(H.weight_bound(w))
    assert (ab, bb) == (R.bound_of(A), R.bound_of(B))
    judge(y.cpu(), A, B, bv, ab, bb, "ops entry points", f"linear_fwd {shape}")

    poison_workspace(H, need)
    gy, w = A.cuda(), R.as_stored("dgrad", B, "B").cuda()            # gy (M, K), w (K, N): gx = gy w, (M, N)
    gx = H.linear_dgrad(gy, w)
    ab, bb = float(H.amax_of(gy)), float(H.weight_bound(w))
    judge(gx.cpu(), A, B, None, ab, bb, "ops entry points", f"linear_dgrad {shape}")

    poison_workspace(H, need)
    gy, x = R.as_stored("wgrad", A, "A").cuda(), R.as_stored("wgrad", B, "B").cuda()      # gy (K, M), x (K, N)
    gw = H.linear_wgrad(gy, x)
    ab, bb = float(H.amax_of(gy)), float(H.amax_of(x))
    assert (ab, bb) == (R.bound_of(A), R.bound_of(B))
    judge(gw.cpu(), A, B, None, ab, bb, "ops entry points", f"linear_wgrad {shape}")

