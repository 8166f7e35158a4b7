"""The kernels of csrc/gan_loss.hip and the autograd Functions over them against the fp64 references of
tests/_gan_loss_refs.py, at the sizes where the row ownership, the loops and the loss formulas can go wrong.

Per element: |got - ref| <= k 2^-24 magnitude with k = R.K[name] = 4 x the fp32 restatement's own ratio
(tests/test_gan_loss_cpu.py); the logit alone is held to its chain bound, R.logit_k(K).  The magnitudes carry the
logit's error through each function (see _gan_loss_refs).  The loss scalar is held to the same form of bound, relative
to its magnitude.  Every check prints its worst ratio (pytest -s) before it asserts; "same bits" is torch.equal.
"""
import pytest
import torch

import _gan_loss_refs as R
from test_losses_gpu import NONFINITE, at_offset, check, same_nonfinite

pytestmark = pytest.mark.gpu

KIND_NAMES = sorted(R.KINDS)


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


@pytest.fixture(scope="module")
def Fn():
    from disentangle_mlp_amd import functional
    return functional


def labels_of(kind):
    return R.LABELS if kind in R.USES_LABEL else (0.9,)


@pytest.fixture(scope="module")
def ref():
    """fp64 references, computed once per (shape, kind, label, divisor) and shared."""
    cache = {}

    def get(shape, kind, label, div=None):
        key = (shape, kind, label, div)
        if key not in cache:
            x = R.head_inputs(shape)
            cache[key] = R.dot_gan_loss(x["feat"], x["w"], x["bias"], kind, label, div)
        return cache[key]

    return get


def check_head(got, r, Kdim, what):
    logit, p, loss, dlogit = got
    check(logit, r["logit"], r["logit_mag"], R.logit_k(Kdim), what + " logit")
    check(p, r["p"], r["p_mag"], R.k_for("p", Kdim), what + " p")
    ok = ~r["tie"]
    check(dlogit.cpu()[ok], r["dlogit"][ok], r["dlogit_mag"][ok], R.k_for("dlogit", Kdim), what + " dlogit")
    check(loss.reshape(1), r["loss"].reshape(1), r["loss_mag"].reshape(1), R.k_for("loss", Kdim), what + " loss")


# ------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"B{s[0]}-K{s[1]}")
def test_edges(H, ref, shape):
    B, Kdim = shape
    x = {k: v.cuda() for k, v in R.head_inputs(shape).items()}
    for kind in KIND_NAMES:
        code = R.KINDS[kind]
        for label in labels_of(kind):
            what = f"dot_gan_loss {shape} {kind} t={label}"
            got = H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], code, label)
            check_head(got, ref(shape, kind, label), Kdim, what)
            dev = H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], code, torch.tensor([label], device="cuda"))
            assert all(torch.equal(a, b) for a, b in zip(got, dev)), what + ": device label"
            div = 3 * B
            got3 = H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], code, label, divisor=div)
            check_head(got3, ref(shape, kind, label, div), Kdim, what + f" divisor {div}")
            assert torch.equal(got3[0], got[0]) and torch.equal(got3[1], got[1]), what + ": the divisor touches logit or p"
            if kind not in R.USES_LABEL:        # the hinge kinds ignore the label: any other one, the same bits
                for other in R.LABELS:
                    alt = H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], code, other)
                    assert all(torch.equal(a, b) for a, b in zip(got, alt)), what + f": label {other} changes a hinge kind"
            nog = H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], code, label, want_grad=False)
            assert nog[3] is None and all(torch.equal(a, b) for a, b in zip(got[:3], nog[:3])), what + ": want_grad=False"
    nob = H.dot_gan_loss_fwd(x["feat"], x["w"], None, R.KINDS["lsgan"], 0.9)
    r0 = R.dot_gan_loss(x["feat"], x["w"], None, "lsgan", 0.9, grads=False)
    check_head(nob, r0, Kdim, f"dot_gan_loss {shape} lsgan, no bias")


# ------------------------------------------------------------------------------------------------ planted logits
PLANTED_AT = {float(v): i for i, v in enumerate(R.PLANTED)}


def test_planted_logits(H):
    """A one-hot weight and a zero bias: the logit IS the planted fp32 number.  Divisor 1: dlogit is dl/ds itself."""
    pl = R.planted_inputs()
    feat, w, bias, s = pl["feat"].cuda(), pl["w"].cuda(), pl["bias"].cuda(), pl["logits"]
    lo, hi = R.NEAR_ONE                     # both fp32 numbers: the neighbours of the hinge's tie
    for kind in KIND_NAMES:
        for label in labels_of(kind):
            logit, p, loss, dlogit = H.dot_gan_loss_fwd(feat, w, bias, R.KINDS[kind], label, divisor=1)
            assert torch.equal(logit.cpu(), s), "the planted logit is the logit"
            r = R.gan_loss(s, kind, label, divisor=1)
            what = f"planted {kind} t={label}"
            check(p, r["p"], r["p_mag"], R.K["v_p"], what + " p")
            check(dlogit, r["glogit"], r["glogit_mag"], R.K["v_glogit"], what + " dlogit")
            check(loss.reshape(1), r["loss"].reshape(1), r["loss_mag"].reshape(1), R.K["v_loss"], what + " loss")
            at = {float(v): float(dlogit[i]) for i, v in enumerate(s)}
            assert sorted(at) == sorted(PLANTED_AT)
            if kind == "hinge_real":      # -1 where 1 - s > 0; the tie has no gradient
                assert (at[1.0], at[hi], at[lo], at[0.0], at[40.0], at[-40.0]) == (0.0, 0.0, -1.0, -1.0, 0.0, -1.0), at
            if kind == "hinge_fake":      # +1 where 1 + s > 0
                assert (at[-1.0], at[-hi], at[-lo], at[0.0], at[-40.0], at[40.0]) == (0.0, 0.0, 1.0, 1.0, 0.0, 1.0), at
            if kind == "hinge_gen":
                assert set(at.values()) == {-1.0}, at
            if kind == "logistic" and label in (0.1, 0.9):      # (with a label of 0 or 1 one side's gradient does vanish)
                for v in (17.0, -17.0, 40.0, -40.0, 104.0, -104.0):
                    assert abs(at[v]) >= 0.09, (label, v, at[v])
    # the on-device record of the defect: the BCE head on the same rows
    for label, rows in ((0.1, (40.0,)), (0.9, (40.0, -40.0))):
        _, _, old = H.dot_sigmoid_bce_fwd(feat, w, bias, label, divisor=1)
        new = H.dot_gan_loss_fwd(feat, w, bias, R.KINDS["logistic"], label, divisor=1)[3]
        for v in rows:
            i = PLANTED_AT[v]
            print(f"s = {v}, t = {label}: BCE dlogit = {float(old[i])!r}, logistic {float(new[i])!r}")
            assert abs(float(old[i])) <= 1e-5 and abs(float(new[i])) >= 0.09, (v, label)
        assert float(old[PLANTED_AT[40.0]]) == 0.0


# ---------------------------------------------------------------------------------------------------- misaligned
@pytest.mark.parametrize("offsets", [(1, 1), (2, 2), (3, 3), (1, 0), (0, 2)], ids=str)
def test_misaligned_pointers_take_the_scalar_loop(H, ref, offsets):
    for shape in ((17, 260), (33, 2048)):
        x = {k: v.cuda() for k, v in R.head_inputs(shape).items()}
        f, w = at_offset(x["feat"], offsets[0]), at_offset(x["w"], offsets[1])
        for kind in ("logistic", "hinge_real"):
            got = H.dot_gan_loss_fwd(f, w, x["bias"], R.KINDS[kind], 0.9)
            check_head(got, ref(shape, kind, 0.9), shape[1], f"misaligned {offsets} {shape} {kind}")


# ---------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("v", NONFINITE, ids=str)
def test_nonfinite(H, v):
    for shape in ((17, 260), (5, 3)):
        x = R.head_inputs(shape)
        feat = x["feat"].clone()
        feat[shape[0] // 2, shape[1] // 2] = v
        wd = x["w"].cuda()
        for kind in KIND_NAMES:
            for label in labels_of(kind):
                r = R.dot_gan_loss(feat, x["w"], x["bias"], kind, label, grads=False)
                got = H.dot_gan_loss_fwd(feat.cuda(), wd, x["bias"].cuda(), R.KINDS[kind], label)
                what = f"dot_gan_loss {shape} {kind} t={label} feat={v}"
                for name, g in zip(("logit", "p", "loss", "dlogit"), got):
                    same_nonfinite(g.reshape(r[name].shape), r[name].float(), f"{what}: {name}")
                rv = R.gan_loss(r["logit"].float(), kind, label)
                pv, lv, gv = H.gan_loss(got[0], R.KINDS[kind], label)
                same_nonfinite(pv, rv["p"].float(), what + ": gan_loss p")
                same_nonfinite(lv, rv["loss"].float(), what + ": gan_loss loss")
                same_nonfinite(gv, rv["glogit"].float(), what + ": gan_loss glogit")
                if v != v:
                    assert bool(torch.isnan(got[3][shape[0] // 2])), what + ": a NaN logit, a NaN gradient"
    # planted non-finite LOGITS: the rule for +-inf is IEEE arithmetic on the formulas
    pl = R.planted_inputs(values=(v, 0.5))
    for kind in KIND_NAMES:
        for label in labels_of(kind):
            r = R.gan_loss(pl["logits"], kind, label)
            got = H.dot_gan_loss_fwd(pl["feat"].cuda(), pl["w"].cuda(), None, R.KINDS[kind], label)
            same_nonfinite(got[1], r["p"].float(), f"{kind} {label} logit {v}: p")
            same_nonfinite(got[2], r["loss"].float(), f"{kind} {label} logit {v}: loss")
            same_nonfinite(got[3], r["glogit"].float(), f"{kind} {label} logit {v}: dlogit")


# ------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("shape", [(17, 260), (33, 2048), (5, 3)], ids=str)
def test_backward(Fn, ref, shape):
    B, Kdim = shape
    x = R.head_inputs(shape)
    for kind in KIND_NAMES:
        label = 0.9
        r = ref(shape, kind, label)
        assert not bool(r["tie"].any())
        f, w, b = (x[k].cuda().requires_grad_() for k in ("feat", "w", "bias"))
        logit, p, loss = Fn.dot_gan_loss(f, w, b, R.KINDS[kind], label)
        assert not logit.requires_grad and not p.requires_grad and loss.requires_grad
        loss.backward()
        what = f"DotGanLossFn {shape} {kind}"
        check(f.grad, r["gfeat"], r["gfeat_mag"], R.k_for("gfeat", Kdim), what + " gfeat")
        check(w.grad.reshape(-1), r["gw"], r["gw_mag"], R.k_for("gw", Kdim, B), what + " gw")
        check(b.grad, r["gb"], r["gb_mag"], R.k_for("gb", Kdim, B), what + " gb")


def test_two_uses_of_one_head_accumulate(Fn, ref):
    """Real, then fake, before ONE backward under the accumulate context: the parameter gradients are the sum."""
    shape = (17, 260)
    x = R.head_inputs(shape)
    x2 = R.head_inputs((17, 256))["feat"]
    x2 = torch.cat([x2, x2[:, :4]], 1)
    for name in ("logistic", "hinge", "lsgan"):
        kr, kf = Fn.GAN_LOSSES[(name, "real")], Fn.GAN_LOSSES[(name, "fake")]
        names = {v: k for k, v in R.KINDS.items()}
        ra = R.dot_gan_loss(x["feat"], x["w"], x["bias"], names[kr], 0.9, 34)
        rb = R.dot_gan_loss(x2, x["w"], x["bias"], names[kf], 0.1, 34)
        assert not bool(ra["tie"].any() or rb["tie"].any())
        grads = {}
        for mode in ("accumulate", "autograd"):
            f1, f2, w, b = (t.cuda().requires_grad_() for t in (x["feat"], x2, x["w"], x["bias"]))
            if mode == "accumulate":
                with Fn.accumulate_param_grads():
                    la = Fn.dot_gan_loss(f1, w, b, kr, 0.9, 34)[2]
                    lb = Fn.dot_gan_loss(f2, w, b, kf, 0.1, 34)[2]
                    torch.autograd.backward([la, lb])
            else:
                la = Fn.dot_gan_loss(f1, w, b, kr, 0.9, 34)[2]
                lb = Fn.dot_gan_loss(f2, w, b, kf, 0.1, 34)[2]
                torch.autograd.backward([la, lb])
            grads[mode] = (f1.grad, f2.grad, w.grad, b.grad)
        g = grads["accumulate"]
        what = f"two uses, {name}"
        check(g[0], ra["gfeat"], ra["gfeat_mag"], R.k_for("gfeat", 260), what + " gfeat real")
        check(g[1], rb["gfeat"], rb["gfeat_mag"], R.k_for("gfeat", 260), what + " gfeat fake")
        check(g[2].reshape(-1), ra["gw"] + rb["gw"], ra["gw_mag"] + rb["gw_mag"], R.k_for("gw", 260, 17), what + " gw")
        check(g[3], ra["gb"] + rb["gb"], ra["gb_mag"] + rb["gb_mag"], R.k_for("gb", 260, 17), what + " gb")
        for a, b_ in zip(g, grads["autograd"]):       # floating-point addition is commutative: autograd's sum, bit for bit
            assert torch.equal(a, b_), what


# -------------------------------------------------------------------------------------------------------- routes
def test_unfused_route_on_the_linear_layers_logits(H, Fn, ref):
    """F.gan_loss on the logits of HipLinear: within the fused route's bounds; on the fused route's own logits, its bits."""
    from disentangle_mlp_amd import model as M
    shape = (33, 2048)
    x = R.head_inputs(shape)
    lin = M.HipLinear(2048, 1).cuda()
    with torch.no_grad():
        lin.weight.copy_(x["w"]), lin.bias.copy_(x["bias"])
    for kind in KIND_NAMES:
        for label in labels_of(kind):
            r = ref(shape, kind, label)
            f = x["feat"].cuda().requires_grad_()
            logit = lin(f).squeeze(-1)
            p, loss = Fn.gan_loss(logit, R.KINDS[kind], label)
            assert not p.requires_grad
            loss.backward()
            what = f"unfused {kind} t={label}"
            check(p, r["p"], r["p_mag"], R.k_for("p", 2048), what + " p")
            check(loss.reshape(1), r["loss"].reshape(1), r["loss_mag"].reshape(1), R.k_for("loss", 2048), what + " loss")
            check(f.grad, r["gfeat"], r["gfeat_mag"], R.k_for("gfeat", 2048), what + " gfeat")
            fused = H.dot_gan_loss_fwd(x["feat"].cuda(), x["w"].cuda(), x["bias"].cuda(), R.KINDS[kind], label)
            pv, lv, gv = H.gan_loss(fused[0], R.KINDS[kind], label)
            assert torch.equal(pv, fused[1]) and torch.equal(gv, fused[3]), what + ": the same logits, the same bits"
            check(lv.reshape(1), r["loss"].reshape(1), r["loss_mag"].reshape(1), R.k_for("loss", 2048), what + " vector loss")
    # gscale, and a label on the device
    s = fused[0]
    rv = R.gan_loss(s, "lsgan", 0.1, 50, gscale=0.75)
    pv, lv, gv = H.gan_loss(s, R.KINDS["lsgan"], torch.tensor([0.1], device="cuda"), divisor=50, gscale=0.75)
    check(gv, rv["glogit"], rv["glogit_mag"], R.K["v_glogit"], "gan_loss lsgan gscale 0.75 glogit")
    check(lv.reshape(1), rv["loss"].reshape(1), rv["loss_mag"].reshape(1), R.K["v_loss"], "gan_loss lsgan loss")


# --------------------------------------------------------------------------------------------------- determinism
def test_two_runs_identical_bits(H):
    shape = (33, 2048)
    x = {k: v.cuda() for k, v in R.head_inputs(shape).items()}
    for kind in KIND_NAMES:
        a = H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], R.KINDS[kind], 0.9)
        ga = H.dot_sigmoid_bce_bwd(a[3], torch.tensor(0.75, device="cuda"), x["feat"], x["w"])
        b = H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], R.KINDS[kind], 0.9)
        gb = H.dot_sigmoid_bce_bwd(b[3], torch.tensor(0.75, device="cuda"), x["feat"], x["w"])
        assert all(torch.equal(u, v) for u, v in zip(a + ga, b + gb)), kind


# ------------------------------------------------------------------------------------------------- graph capture
def test_capture_with_a_device_label_replays_the_eager_bits(H):
    shape = (33, 2048)
    x = {k: v.cuda() for k, v in R.head_inputs(shape).items()}
    g1 = torch.tensor(0.75, device="cuda")
    lab = torch.tensor([0.9], device="cuda")
    for kind in ("logistic", "lsgan"):
        code = R.KINDS[kind]
        H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], code, lab)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], code, lab)
            grads = H.dot_sigmoid_bce_bwd(out[3], g1, x["feat"], x["w"])
        for value in (0.9, 0.1, 0.9):
            lab.fill_(value)
            graph.replay()
            torch.cuda.synchronize()
            eager = H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], code, value)
            egrads = H.dot_sigmoid_bce_bwd(eager[3], g1, x["feat"], x["w"])
            assert all(torch.equal(u, v) for u, v in zip(out + grads, eager + egrads)), (kind, value)


def test_argument_checks(H):
    x = {k: v.cuda() for k, v in R.head_inputs((5, 3)).items()}
    with pytest.raises(RuntimeError, match="kind"):
        H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], 5, 0.9)
    with pytest.raises(RuntimeError, match="kind"):
        H.gan_loss(x["feat"][:, 0].contiguous(), -1, 0.9)
    with pytest.raises(RuntimeError, match="does not match"):
        H.dot_gan_loss_fwd(x["feat"], x["w"][:, :2].contiguous(), x["bias"], 0, 0.9)
    with pytest.raises(RuntimeError, match="one fp32 value"):
        H.dot_gan_loss_fwd(x["feat"], x["w"], x["bias"], 0, torch.zeros(2, device="cuda"))
