"""The kernels of csrc/losses.hip (and channel_sum / BatchNorm's activation in csrc/bn.hip) and the autograd Functions
over them against the fp64 references of tests/_loss_refs.py, at the sizes where their loops, tails, index arithmetic
and clamps can go wrong.

Element-wise results are judged per element: |got - ref| <= k 2^-24 magnitude, k per operation from the fp32
restatement measured in tests/test_losses_cpu.py (R.K); reduced scalars at the figures of test_loss_kats (2e-6 for the
KL and the squared difference, 1e-5 for BCE; exactly 0 where the reference is 0); "same bits" is torch.equal.
Every check prints its worst ratio (pytest -s) before it asserts.

Non-finite values: where torch gives NaN / inf, so must the kernel (isnan and isinf compared separately with the fp64
reference).  reparam_kl_bwd is held to that with gz, gkl or both present: an absent upstream gradient takes its whole
term out, as in autograd (0 * inf would be a NaN that torch does not have).

Misaligned inputs: a contiguous view at 1-3 floats from a 16-byte boundary is a legal argument; the host side picks the
scalar loops for it.  Every output of these operations is allocated by the operation itself (there is no out= path), so
there is no view to write around.
"""
import pytest
import torch

import _loss_refs as R

pytestmark = pytest.mark.gpu

ACTS = {"none": 0, "relu": 1, "lrelu": 2}      # VG_ACT_*


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


@pytest.fixture(scope="module")
def Fn():
    from disentangle_mlp_amd import functional
    return functional


def at_offset(t, o):
    """A contiguous copy of t whose first element lies o floats past a 16-byte boundary."""
    t = t.contiguous()
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[o:o + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * (o % 4)
    return v


def check(got, ref, mag, k, what):
    """Per element: |got - ref| <= k 2^-24 magnitude."""
    got = got.detach().cpu().double()
    ref, mag = ref.double(), mag.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    w = R.worst_ratio(got, ref, mag)
    print(f"{what}: worst {w:.2f} x 2^-24 (k = {k})")
    bad = (got - ref).abs() > k * R.U * mag
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements off by more than {k} x 2^-24 x "
                                 f"magnitude (worst {w:.2f}); first at {bad.nonzero()[0].tolist()}")


def check_scalar(got, ref, rel, what):
    got, ref = float(torch.as_tensor(got).detach()), float(ref)
    print(f"{what}: {got!r} vs {ref!r} ({abs(got - ref) / max(abs(ref), 1e-300):.2e} rel, bound {rel:.0e})")
    if ref == 0.0:
        assert got == 0.0, (what, got)
    else:
        assert abs(got - ref) <= rel * abs(ref), (what, got, ref)


def same_nonfinite(got, ref, what):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), \
        f"{what}: isnan differs from the fp64 reference: {int(torch.isnan(got).sum())} NaN, {int(torch.isnan(ref).sum())} expected"
    assert torch.equal(torch.isinf(got), torch.isinf(ref)), \
        f"{what}: isinf differs from the fp64 reference: {int(torch.isinf(got).sum())} inf, {int(torch.isinf(ref).sum())} expected"


NONFINITE = (float("nan"), float("inf"), float("-inf"))


def planted(t, v):
    """t with the value v at a middle element."""
    t = t.clone()
    t.view(-1)[t.numel() // 2] = v
    return t


# which inputs sit at an offset: all of them by o floats, or the first one only
def offsets_for(n_inputs):
    return [(o,) * n_inputs for o in (1, 2, 3)] + [(1,) + (0,) * (n_inputs - 1), (0,) * (n_inputs - 1) + (2,)]


# ------------------------------------------------------------------------------------------------- flat kernels
_flat_ref = {}


def flat_ref(key, fn):
    if key not in _flat_ref:
        _flat_ref[key] = fn()
    return _flat_ref[key]


@pytest.mark.parametrize("n", R.FLAT_SIZES)
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_act_bwd(H, n, kind):
    f = R.flat_inputs(n)
    y = R.act(f["x"], kind)
    ref = flat_ref(("act_bwd", n, kind), lambda: R.act_bwd(f["gy"], y, kind))
    gx = H.act_bwd(f["gy"].cuda(), y.cuda(), R.KINDS[kind])
    check(gx, ref["gx"], ref["gx_mag"], R.K["act_bwd"], f"act_bwd {kind} n={n}")
    check(gx[-3:], ref["gx"][-3:], ref["gx_mag"][-3:], R.K["act_bwd"], "  its last three elements")
    if n in (4, 1027, R.FLAT_BIG):
        for og, oy in offsets_for(2) if n != R.FLAT_BIG else [(3, 3)]:
            gx = H.act_bwd(at_offset(f["gy"].cuda(), og), at_offset(y.cuda(), oy), R.KINDS[kind])
            check(gx, ref["gx"], ref["gx_mag"], R.K["act_bwd"], f"  gy at +{og}, y at +{oy} floats")


@pytest.mark.parametrize("n", R.FLAT_SIZES)
def test_scale_by_scalar(H, n):
    g = R.flat_inputs(n)["gy"]
    gd = g.cuda()
    for s in (0.37, 0.0, -1.0, 2.0 ** -20):
        sd = torch.tensor(s, device="cuda")
        out = H.scale_by_scalar(gd, sd)
        ref = R.scale_by_scalar(g, torch.tensor(s))
        check(out, ref["out"], ref["out_mag"], R.K["scale_by_scalar"], f"scale_by_scalar n={n} s={s}")
        assert torch.equal(out, gd * sd), (n, s)                      # one fp32 product per element: the same bits
        assert torch.equal(out[-3:], (gd * sd)[-3:]), (n, s)
        if n in (4, 1027) or (n == R.FLAT_BIG and s == 0.37):
            for o in (1, 2, 3):
                assert torch.equal(H.scale_by_scalar(at_offset(gd, o), sd), out), (n, s, o)


@pytest.mark.parametrize("n", R.FLAT_SIZES)
def test_sqdiff(H, n):
    f = R.flat_inputs(n)
    a, b = f["a"].cuda(), f["b"].cuda()
    for scale in (0.5, 1.0):
        for gscale in (1.0, 0.37):
            ref = flat_ref(("sqdiff", n, scale, gscale), lambda: R.sqdiff(f["a"], f["b"], scale, gscale))
            what = f"sqdiff n={n} scale={scale} gscale={gscale}"
            loss, ga = H.sqdiff_loss(a, b, scale, gscale)
            check_scalar(loss, ref["loss"], R.REL_SQDIFF, what + " loss")
            check(ga, ref["ga"], ref["ga_mag"], R.K["sqdiff_ga"], what + " ga")
            check(ga[-3:], ref["ga"][-3:], ref["ga_mag"][-3:], R.K["sqdiff_ga"], "  its last three elements")
            loss2, none = H.sqdiff_loss(a, b, scale, gscale, want_grad=False)
            assert none is None and torch.equal(loss2, loss), what + ": want_grad=False changes the loss"
            loss3, ga3 = H.sqdiff_loss(a, b, scale, gscale)
            assert torch.equal(loss3, loss) and torch.equal(ga3, ga), what + ": a second call differs"
    if n in (4, 1027, R.FLAT_BIG):
        ref = flat_ref(("sqdiff", n, 0.5, 0.37), lambda: R.sqdiff(f["a"], f["b"], 0.5, 0.37))
        for oa, ob in offsets_for(2) if n != R.FLAT_BIG else [(3, 3)]:
            loss, ga = H.sqdiff_loss(at_offset(a, oa), at_offset(b, ob), 0.5, 0.37)
            check_scalar(loss, ref["loss"], R.REL_SQDIFF, f"sqdiff n={n}, a at +{oa}, b at +{ob} floats: loss")
            check(ga, ref["ga"], ref["ga_mag"], R.K["sqdiff_ga"], "  ga")


@pytest.mark.parametrize("n", (5, 1027, R.FLAT_BIG))
def test_sqdiff_one_ulp_apart(H, n):
    """a and b one ulp apart in a few elements (the first, the last -- in the tail -- and a middle one), equal elsewhere:
    the loss is the fp64 sum of the squares of the fp32 differences, nothing else."""
    a = R.flat_inputs(n)["a"].clone()
    b = a.clone()
    idx = sorted({0, n // 2, n - 1})
    b[idx] = torch.nextafter(a[idx], torch.full((len(idx),), float("inf")))
    d = (a - b).double()
    assert int((d != 0).sum()) == len(idx)
    loss, ga = H.sqdiff_loss(a.cuda(), b.cuda(), 1.0)
    want = (d * d).sum()
    assert float(loss) == float(want.float()), (float(loss), float(want))
    assert torch.equal(ga.cpu(), 2 * (a - b))


# ------------------------------------------------------------------------------------------- bias_act / BiasActFn
_bias_ref = {}


def bias_ref(shape, form, kind):
    key = (shape, form, kind)
    if key not in _bias_ref:
        i = R.bias_inputs(shape)
        _bias_ref[key] = R.bias_act(i["x"], R.bias_values(shape[1], form), kind, gy=i["gy"])
    return _bias_ref[key]


@pytest.mark.parametrize("shape", R.BIAS_SHAPES)
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_bias_act_fwd(H, shape, kind):
    x = R.bias_inputs(shape)["x"].cuda()
    for form in R.BIAS_FORMS:
        bias = R.bias_values(shape[1], form)
        bd = None if bias is None else bias.cuda()
        ref = bias_ref(shape, form, kind)
        what = f"bias_act_fwd {shape} {kind} bias={form}"
        y = H.bias_act_fwd(x, bd, R.KINDS[kind])
        check(y, ref["y"], ref["y_mag"], R.K["bias_act_y"], what)
        for o in (1, 2, 3):
            check(H.bias_act_fwd(at_offset(x, o), bd, R.KINDS[kind]), ref["y"], ref["y_mag"], R.K["bias_act_y"],
                  f"  x at +{o} floats")


@pytest.mark.parametrize("shape", R.BIAS_SHAPES)
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_bias_act_function(H, Fn, shape, kind):
    """functional.bias_act: gx (act_bwd) and gb (channel_sum at HW = 1 and HW > 1) against fp64 autograd, the upstream
    gradient a non-contiguous view."""
    i = R.bias_inputs(shape)
    wide = torch.zeros(shape[0], shape[1], 2 * shape[2], device="cuda")
    wide[..., ::2] = i["gy"].cuda()
    gy = wide[..., ::2]
    assert gy.numel() == 1 or not gy.is_contiguous()
    for form in R.BIAS_FORMS:
        ref = bias_ref(shape, form, kind)
        what = f"BiasActFn {shape} {kind} bias={form}"
        x = i["x"].cuda().requires_grad_()
        bias = None if form == "none" else R.bias_values(shape[1], form).cuda().requires_grad_()
        y = Fn.bias_act(x, bias, R.KINDS[kind])
        check(y, ref["y"], ref["y_mag"], R.K["bias_act_y"], what + " y")
        y.backward(gy)
        check(x.grad, ref["gx"], ref["gx_mag"], R.K["bias_act_gx"], what + " gx")
        if bias is not None:
            check(bias.grad, ref["gb"], ref["gb_mag"], R.K["bias_act_gb"], what + " gb")
            x2, frozen = i["x"].cuda().requires_grad_(), bias.detach().clone()
            Fn.bias_act(x2, frozen, R.KINDS[kind]).backward(gy)
            assert frozen.grad is None and torch.equal(x2.grad, x.grad), what + ": frozen bias"


# ------------------------------------------------------------------------------------------------- channel_sum
@pytest.mark.parametrize("shape", R.CSUM_SHAPES)
def test_channel_sum(H, shape):
    g = R.csum_input(shape)
    ref = R.channel_sum(g)
    out = H.channel_sum(g.cuda())
    check(out, ref["out"], ref["out_mag"], R.K["channel_sum"], f"channel_sum {shape}")
    for o in (1, 2, 3):
        check(H.channel_sum(at_offset(g.cuda(), o)), ref["out"], ref["out_mag"], R.K["channel_sum"], f"  g at +{o} floats")


# ---------------------------------------------------------------------------------------------------- reparam + KL
_rkl_ref = {}


def rkl_ref(shape, beta, with_gz, with_gkl):
    key = (shape, beta, with_gz, with_gkl)
    if key not in _rkl_ref:
        i = R.rkl_inputs(shape)
        _rkl_ref[key] = R.reparam_kl(i["mu"], i["lv"], i["eps"], beta, gz=i["gz"] if with_gz else None,
                                     gkl=i["gkl"] if with_gkl else None)
    return _rkl_ref[key]


@pytest.mark.parametrize("shape", R.RKL_SHAPES)
@pytest.mark.parametrize("beta", (1.0, 25.0))
def test_reparam_kl_ops(H, shape, beta):
    i = R.rkl_inputs(shape)
    mu, lv, eps, gz, gkl = (i[k].cuda() for k in ("mu", "lv", "eps", "gz", "gkl"))
    ref = rkl_ref(shape, beta, True, True)
    what = f"reparam_kl {shape} beta={beta}"
    z, kl, rows = H.reparam_kl_fwd(mu, lv, eps, beta, want_rows=True)
    check(z, ref["z"], ref["z_mag"], R.K["rkl_z"], what + " z")
    check(rows, ref["rows"], ref["rows_mag"], R.K["rkl_rows"], what + " rows")
    check_scalar(kl, ref["kl"], R.REL_KL, what + " kl")
    if i["zero_row"] is not None:
        assert float(rows[i["zero_row"]]) == 0.0, what + ": KL of the mu = 0, logvar = 0 row"
    z2, kl2, none = H.reparam_kl_fwd(mu, lv, eps, beta)
    assert none is None and torch.equal(z2, z) and torch.equal(kl2, kl)
    if beta == 25.0 and shape in ((17, 65), (5, 128), (1, 1)):          # offset views: scalar loops, the same expectations
        full = rkl_ref(shape, beta, True, True)
        for o in (1, 2, 3):
            mo, lo, eo, go = (at_offset(t, o) for t in (mu, lv, eps, gz))
            zo, klo, ro = H.reparam_kl_fwd(mo, lo, eo, beta, want_rows=True)
            check(zo, ref["z"], ref["z_mag"], R.K["rkl_z"], f"  inputs at +{o} floats: z")
            check(ro, ref["rows"], ref["rows_mag"], R.K["rkl_rows"], "  rows")
            check_scalar(klo, ref["kl"], R.REL_KL, "  kl")
            gmo, glo = H.reparam_kl_bwd(go, mo, lo, eo, gkl, beta)
            check(gmo, full["gmu"], full["gmu_mag"], R.K["rkl_gmu"], "  gmu")
            check(glo, full["glv"], full["glv_mag"], R.K["rkl_glv"], "  glv")
    for with_gz, with_gkl in ((True, True), (False, True), (True, False), (False, False)):
        gmu, glv = H.reparam_kl_bwd(gz if with_gz else None, mu, lv, eps, gkl if with_gkl else None, beta)
        tag = f"{what} bwd gz={'given' if with_gz else None} gkl={'given' if with_gkl else None}"
        if not (with_gz or with_gkl):           # legal at this level: nothing upstream, zero gradients
            assert not bool(gmu.any()) and not bool(glv.any()), tag
            continue
        r = rkl_ref(shape, beta, with_gz, with_gkl)
        check(gmu, r["gmu"], r["gmu_mag"], R.K["rkl_gmu"], tag + " gmu")
        check(glv, r["glv"], r["glv_mag"], R.K["rkl_glv"], tag + " glv")


@pytest.mark.parametrize("shape", ((17, 65), (5, 128), (300, 128), (1, 200)))
def test_reparam_kl_functions(H, Fn, shape):
    """reparam_kl with only kl.backward(), only z.sum().backward() and both; kld_loss; KLRowsFn."""
    i = R.rkl_inputs(shape)
    beta = 25.0
    dev = lambda: (i["mu"].cuda().requires_grad_(), i["lv"].cuda().requires_grad_(), i["eps"].cuda())      # noqa: E731
    full = rkl_ref(shape, beta, True, True)
    ones = torch.ones(shape)
    # both: z . gz + 0.75 kl
    mu, lv, eps = dev()
    z, kl = Fn.reparam_kl(mu, lv, eps, beta)
    check(z, full["z"], full["z_mag"], R.K["rkl_z"], f"ReparamKLFn {shape} z")
    check_scalar(kl, full["kl"], R.REL_KL, "  kl")
    ((z * i["gz"].cuda()).sum() + 0.75 * kl).backward()
    check(mu.grad, full["gmu"], full["gmu_mag"], R.K["rkl_gmu"], "  both: gmu")
    check(lv.grad, full["glv"], full["glv_mag"], R.K["rkl_glv"], "  both: glv")
    # only the KL, upstream 0.75
    r = rkl_ref(shape, beta, False, True)
    mu, lv, eps = dev()
    (0.75 * Fn.reparam_kl(mu, lv, eps, beta)[1]).backward()
    check(mu.grad, r["gmu"], r["gmu_mag"], R.K["rkl_gmu"], "  kl only: gmu")
    check(lv.grad, r["glv"], r["glv_mag"], R.K["rkl_glv"], "  kl only: glv")
    mu2, lv2 = i["mu"].cuda().requires_grad_(), i["lv"].cuda().requires_grad_()
    kld = Fn.kld_loss(mu2, lv2, beta)
    check_scalar(kld, full["kl"], R.REL_KL, "  kld_loss")
    (0.75 * kld).backward()
    check(mu2.grad, r["gmu"], r["gmu_mag"], R.K["rkl_gmu"], "  kld_loss: gmu")
    check(lv2.grad, r["glv"], r["glv_mag"], R.K["rkl_glv"], "  kld_loss: glv")
    # only z
    rz = R.reparam_kl(i["mu"], i["lv"], i["eps"], beta, gz=ones)
    mu, lv, eps = dev()
    Fn.reparam_kl(mu, lv, eps, beta)[0].sum().backward()
    check(mu.grad, rz["gmu"], rz["gmu_mag"], R.K["rkl_gmu"], "  z only: gmu")
    check(lv.grad, rz["glv"], rz["glv_mag"], R.K["rkl_glv"], "  z only: glv")
    # KLRowsFn: the rows are not differentiable, the gradient flows through z
    r1 = R.reparam_kl(i["mu"], i["lv"], i["eps"], 1.0, gz=i["gz"])
    mu, lv, eps = dev()
    z, rows = Fn.KLRowsFn.apply(mu, lv, eps)
    assert not rows.requires_grad
    check(rows, r1["rows"], r1["rows_mag"], R.K["rkl_rows"], "  KLRowsFn rows")
    check(z, r1["z"], r1["z_mag"], R.K["rkl_z"], "  KLRowsFn z")
    (z * i["gz"].cuda()).sum().backward()
    check(mu.grad, r1["gmu"], r1["gmu_mag"], R.K["rkl_gmu"], "  KLRowsFn gmu")
    check(lv.grad, r1["glv"], r1["glv_mag"], R.K["rkl_glv"], "  KLRowsFn glv")


# ------------------------------------------------------------------------------------------------------------ BCE
@pytest.mark.parametrize("B", R.BCE_B)
@pytest.mark.parametrize("label", R.BCE_LABELS)
def test_bce(H, Fn, B, label):
    p, planted_at = R.bce_input(B)
    pd = p.cuda()
    ref = R.bce(p, label)
    what = f"bce B={B} label={label}"
    loss, gp = H.bce_loss(pd, label)
    check_scalar(loss, ref["loss"], R.REL_BCE, what + " loss")
    # the planted saturated probabilities included: the reference IS the clamped formula in fp64 on the fp32 p
    check(gp, ref["gp"], ref["gp_mag"], R.K["bce_gp"], what + " gp")
    check(gp[planted_at], ref["gp"][planted_at], ref["gp_mag"][planted_at], R.K["bce_gp"], "  the planted elements")
    loss_d, gp_d = H.bce_loss(pd, torch.tensor([label], device="cuda"))
    assert torch.equal(loss_d, loss) and torch.equal(gp_d, gp), what + ": device label"
    loss_h, gp_h = H.bce_loss(pd, label, divisor=2 * B)
    assert torch.equal(loss_h, loss / 2) and torch.equal(gp_h, gp / 2), what + ": divisor 2B"
    loss_s, gp_s = H.bce_loss(pd, label, gscale=0.75)
    rs = R.bce(p, label, gscale=0.75)
    assert torch.equal(loss_s, loss), what + ": gscale touches the loss"
    check(gp_s, rs["gp"], rs["gp_mag"], R.K["bce_gp"], what + " gp, gscale 0.75")
    loss_n, none = H.bce_loss(pd, label, want_grad=False)
    assert none is None and torch.equal(loss_n, loss), what + ": want_grad=False"
    check(H.bce_loss(at_offset(pd, 1), label)[1], ref["gp"], ref["gp_mag"], R.K["bce_gp"], "  p at +1 float")
    # BCELossFn, upstream gradient 0.75, against fp64 autograd of nn.BCELoss
    from oracle import steps as S
    p64 = p.double().requires_grad_()
    (0.75 * S.bce_loss(p64, R.f32(label))).backward()
    for lab in (label, torch.tensor([label], device="cuda")):
        pg = pd.clone().requires_grad_()
        lf = Fn.bce_loss(pg, lab)
        assert torch.equal(lf.detach(), loss)
        (0.75 * lf).backward()
        check(pg.grad, p64.grad, rs["gp_mag"], R.K["bce_gp"], what + " BCELossFn gp")


# -------------------------------------------------------------------------------- sim_loss / reconstruction_loss
@pytest.mark.parametrize("name,scale", (("sim_loss", 0.5), ("reconstruction_loss", 1.0)))
def test_sqdiff_functions(H, Fn, name, scale):
    """Upstream gradient 0.37; the target hangs on a graph of its own and receives nothing."""
    n = 1027
    f = R.flat_inputs(n)
    ref = R.sqdiff(f["a"], f["b"], scale, 0.37)
    a = f["a"].cuda().requires_grad_()
    leaf = f["b"].cuda().requires_grad_()
    target = leaf * 1.0
    assert target.requires_grad
    loss = getattr(Fn, name)(a, target)
    check_scalar(loss, ref["loss"], R.REL_SQDIFF, name)
    (0.37 * loss).backward()
    assert leaf.grad is None
    # (the Function rounds 2 scale (a - b), then the product with 0.37: part of the sqdiff_ga row of the fp32 table)
    check(a.grad, ref["ga"], ref["ga_mag"], R.K["sqdiff_ga"], name + " ga")


# ------------------------------------------------------------------------------------- non-finite in, non-finite out
@pytest.mark.parametrize("v", NONFINITE)
def test_nonfinite_flat(H, v):
    n = 1027
    f = R.flat_inputs(n)
    for kind in R.KINDS:
        y = R.act(f["x"], kind)
        for gy_, y_ in ((planted(f["gy"], v), y), (f["gy"], planted(y, v))):
            same_nonfinite(H.act_bwd(gy_.cuda(), y_.cuda(), R.KINDS[kind]), R.act_bwd(gy_, y_, kind)["gx"], f"act_bwd {kind} {v}")
    g = planted(f["gy"], v)
    same_nonfinite(H.scale_by_scalar(g.cuda(), torch.tensor(0.37, device="cuda")), R.scale_by_scalar(g, torch.tensor(0.37))["out"],
                   f"scale_by_scalar {v}")
    same_nonfinite(H.scale_by_scalar(f["gy"].cuda(), torch.tensor(v, device="cuda")), R.scale_by_scalar(f["gy"], torch.tensor(v))["out"],
                   f"scale_by_scalar by {v}")
    for a_, b_ in ((planted(f["a"], v), f["b"]), (f["a"], planted(f["b"], v))):
        loss, ga = H.sqdiff_loss(a_.cuda(), b_.cuda(), 0.5)
        ref = R.sqdiff(a_, b_, 0.5)
        same_nonfinite(loss, ref["loss"], f"sqdiff loss {v}")
        same_nonfinite(ga, ref["ga"], f"sqdiff ga {v}")


@pytest.mark.parametrize("v", NONFINITE)
def test_nonfinite_bias_act_channel_sum(H, v):
    for shape in ((3, 7, 1), (2, 5, 8), (5, 3, 6)):
        i = R.bias_inputs(shape)
        bias = R.bias_values(shape[1], "small")
        for kind in R.KINDS:
            for x_, b_ in ((planted(i["x"], v), bias), (planted(i["x"], v), None), (i["x"], planted(bias, v))):
                y = H.bias_act_fwd(x_.cuda(), None if b_ is None else b_.cuda(), R.KINDS[kind])
                same_nonfinite(y, R.bias_act(x_, b_, kind)["y"], f"bias_act_fwd {shape} {kind} {v}")
        g = planted(i["gy"], v)
        same_nonfinite(H.channel_sum(g.cuda()), R.channel_sum(g)["out"], f"channel_sum {shape} {v}")


@pytest.mark.parametrize("v", NONFINITE)
def test_nonfinite_reparam_kl(H, v):
    """Forward, and backward with gz, gkl or both given: an absent gradient's term is absent, not 0 * inf."""
    shape = (17, 65)
    i = R.rkl_inputs(shape)
    for name in ("mu", "lv", "eps", "gz"):
        t = {k: i[k] for k in ("mu", "lv", "eps", "gz")}
        t[name] = planted(t[name], v)
        mu, lv, eps, gz = (t[k].cuda() for k in ("mu", "lv", "eps", "gz"))
        z, kl, rows = H.reparam_kl_fwd(mu, lv, eps, 25.0, want_rows=True)
        what = f"reparam_kl {name}={v}"
        for with_gz, with_gkl in ((True, True), (False, True), (True, False)):
            ref = R.reparam_kl(t["mu"], t["lv"], t["eps"], 25.0, gz=t["gz"] if with_gz else None,
                               gkl=i["gkl"] if with_gkl else None)
            if with_gz and with_gkl:
                same_nonfinite(z, ref["z"], what + " z"), same_nonfinite(rows, ref["rows"], what + " rows")
                same_nonfinite(kl, ref["kl"], what + " kl")
            gmu, glv = H.reparam_kl_bwd(gz if with_gz else None, mu, lv, eps, i["gkl"].cuda() if with_gkl else None, 25.0)
            tag = f"{what} gz={'given' if with_gz else None} gkl={'given' if with_gkl else None}"
            same_nonfinite(gmu, ref["gmu"], tag + " gmu"), same_nonfinite(glv, ref["glv"], tag + " glv")


@pytest.mark.parametrize("v", NONFINITE)
def test_nonfinite_bce(H, v):
    """A NaN probability is a NaN loss (torch's log().clamp(min=-100) keeps it; fmaxf dropped it)."""
    for B in (65, 257):
        p = planted(R.bce_input(B)[0], v)
        ref = R.bce(p, 0.9)
        for lab in (0.9, torch.tensor([0.9], device="cuda")):
            loss, gp = H.bce_loss(p.cuda(), lab)
            same_nonfinite(loss, ref["loss"], f"bce_loss B={B} p={v}: loss")
            same_nonfinite(gp, ref["gp"], f"bce_loss B={B} p={v}: gp")
    for B, K in ((5, 70), (17, 256)):          # the scalar and the 16-byte row loop of the fused head
        feat, w, b = R.randn(B, K, seed=150), R.randn(K, seed=151) / K ** 0.5, R.randn(1, seed=152)
        feat = planted(feat, v)
        ref = R.dot_sigmoid_bce(feat, w, b, 0.9)
        p, loss, dlogit = H.dot_sigmoid_bce_fwd(feat.cuda(), w.cuda(), b.cuda(), 0.9)
        what = f"dot_sigmoid_bce_fwd ({B}, {K}) feat={v}"
        same_nonfinite(p, ref["p"], what + ": p"), same_nonfinite(loss, ref["loss"], what + ": loss")
        same_nonfinite(dlogit, ref["dlogit"], what + ": dlogit")


@pytest.mark.parametrize("v", NONFINITE)
@pytest.mark.parametrize("act", list(ACTS))
def test_nonfinite_bn_affine(H, v, act):
    """A poisoned channel leaves BatchNorm + activation as NaN -- with ReLU too, not as zeros."""
    for shape in ((4, 3, 2, 2), (3, 5, 3, 3), (6, 5)):          # 16-byte and scalar plane loops, BatchNorm1d
        C = shape[1]
        x = planted(R.randn(*shape, seed=160), v)
        gamma, beta = 1 + 0.1 * R.randn(C, seed=161), 0.1 * R.randn(C, seed=162)
        ref = R.bn_act(x, gamma, beta, act)
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        y, mean, invstd = H.bn_act_fwd(x.cuda(), gamma.cuda(), beta.cuda(), rm, rv, 1e-5, 0.1, ACTS[act])
        what = f"bn_act_fwd {shape} {act} x={v}"
        assert bool(torch.isnan(ref["y"]).reshape(shape[0], C, -1).all(2).all(0).any()), "the reference has a NaN channel"
        same_nonfinite(y, ref["y"], what + ": y")
        same_nonfinite(mean, ref["mean"], what + ": mean"), same_nonfinite(invstd, ref["invstd"], what + ": invstd")
        same_nonfinite(rm, ref["rm"], what + ": running_mean"), same_nonfinite(rv, ref["rv"], what + ": running_var")
        if len(shape) == 4:
            scale, shift = R.randn(C, seed=163), R.randn(C, seed=164)          # both signs: inf goes either way
            same_nonfinite(H.affine_act(x.cuda(), scale.cuda(), shift.cuda(), ACTS[act]),
                           R.affine_act(x, scale, shift, act)["y"], f"affine_act {shape} {act} x={v}")


@pytest.mark.parametrize("shape", ((2, 3, 2, 2), (3, 5, 8, 16), (2, 3, 3, 3)))
def test_affine_act_misaligned(H, shape):
    """vg_affine_act: x at 1-3 floats from a 16-byte boundary gives the bits of the aligned call."""
    C = shape[1]
    x, scale, shift = R.randn(*shape, seed=170).cuda(), R.randn(C, seed=171).cuda(), R.randn(C, seed=172).cuda()
    for act in ACTS.values():
        y = H.affine_act(x, scale, shift, act)
        ref = R.affine_act(x, scale, shift, {v: k for k, v in ACTS.items()}[act])["y"]
        assert float((y.cpu().double() - ref).abs().max()) <= 4 * R.U * float(ref.abs().max() + 1)
        for o in (1, 2, 3):
            assert torch.equal(H.affine_act(at_offset(x, o), scale, shift, act), y), (shape, act, o)
