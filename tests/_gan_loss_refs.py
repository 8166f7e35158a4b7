"""References for the adversarial losses on the logit (csrc/gan_loss.hip) and the seeded inputs
the CPU and the GPU tests share.  A plain module: nothing here touches a GPU.  Conventions: tests/_loss_refs.py.

Per kind, with logit s and label t (the hinge kinds ignore t):

    logistic     l = (1 - t) s + max(-s, 0) + log1p(exp(-|s|))      dl/ds = sigmoid(s) - t
    lsgan        l = (s - t)^2 / 2                                   dl/ds = s - t
    hinge_real   l = max(0, 1 - s)                                   dl/ds = -1 where 1 - s > 0, else 0
    hinge_fake   l = max(0, 1 + s)                                   dl/ds = +1 where 1 + s > 0, else 0
    hinge_gen    l = -s                                              dl/ds = -1

`terms` restates them in ``dtype`` (fp64: the reference; fp32: the honest restatement) with dl/ds written out -- a NaN
logit gives a NaN gradient for every kind, which autograd through relu or a negation would not -- and
tests/test_gan_loss_cpu.py holds value and gradient to torch's own binary_cross_entropy_with_logits, mse_loss / 2 and
relu under autograd.  `dot_gan_loss` is the fused head: logit = feat . w + bias, p = sigmoid(logit), the loss (terms
added in fp64, divided by the divisor), dlogit = dl/ds / divisor, and gfeat, gw, gb by autograd through torch's own
forms.

Magnitudes.  The logit's is sum_j |feat_j w_j| + |bias|.  Every other output is a function g of the logit, so its error
has two sources: evaluating g (judged against g's own magnitude: for the logistic term the sum of the absolute values
of its addends) and the logit's error carried through g (|g'(s)| x the logit's magnitude).  ``<name>_mag`` is the sum of
the two, and FP32_WORST is measured against it with an fp32 logit, so k = K[name] = 4 x FP32_WORST[name] bounds both
(`k_for`); the chain bound `logit_k` is used for the logit alone.  A hinge row whose logit lies within its own
error bound of the tie is marked in ``tie``: there the gradient's side is undecided (the planted-logit tests decide it
on exact logits) and the per-element check of dlogit leaves the row out.
"""
import functools
import math

import torch

from _loss_refs import U, _c, _sum64, f32, randn, worst_ratio  # noqa: F401  (re-exported for the tests)

KINDS = {"logistic": 0, "lsgan": 1, "hinge_real": 2, "hinge_fake": 3, "hinge_gen": 4}      # VG_GAN_* of include/vaegan_hip.h
USES_LABEL = ("logistic", "lsgan")
LABELS = (0.0, 0.1, 0.9, 1.0)

# Worst |fp32 restatement - fp64| / magnitude, in units of 2^-24, as tests/test_gan_loss_cpu.py measures it over every
# input set below (it prints the table).  K = 4 x that, as in _loss_refs: the factor covers expf / log1pf of the device
# differing from the host's by a couple of ulp, and the device's 1 / divisor being a rounded fp32 factor.
FP32_WORST = {"logit": 1.4, "p": 1.2, "dlogit": 1.8, "loss": 1.2, "gfeat": 2.0, "gw": 3.8, "gb": 1.6,      # the fused head
              "v_p": 2.0, "v_glogit": 2.6, "v_loss": 3.0}                                                  # the logit vector
K = {name: 4.0 * v for name, v in FP32_WORST.items()}


def logit_k(Kdim):
    """The kernel's own bound for the logit, in units of 2^-24 of sum |feat_j w_j| + |bias|: a lane's chain of fused
    multiply-adds (four per 16-byte load, ceil(K / 256) loads; the scalar loop's ceil(K / 64) is never longer), the six
    additions of the 64-lane shuffle sum, the bias, and one for the first-order form of (1 + u)^n - 1."""
    return 4 * math.ceil(Kdim / 256) + 6 + 1 + 1


def k_for(name, Kdim=None, B=None):
    """The GPU's per-element k for output ``name`` of the fused head: K[name] = 4 x the fp32 restatement's own ratio,
    whatever the sizes -- the magnitudes already carry the logit's error through each function, and FP32_WORST was
    measured against those magnitudes with an fp32 logit.  The chain bound `logit_k` is for the logit alone."""
    return K[name]


def sigmoid_stable(s):
    e = torch.exp(-s.abs())
    return torch.where(s >= 0, 1 / (1 + e), e / (1 + e))


def terms(s, t, kind):
    """Row terms of ``kind`` at logits ``s`` (any float dtype), label ``t`` (a float): a dict of p, l, dl and, in fp64,
    the magnitudes l_mag / dl_mag / p_mag (evaluation only) and the sensitivities l_sens / dl_sens / p_sens = |d . / ds|."""
    a = s.abs()
    e = torch.exp(-a)
    p = torch.where(s >= 0, 1 / (1 + e), e / (1 + e))
    sd, pd = s.detach().double(), p.detach().double()
    one = torch.ones_like(sd)
    tiny = 2.0 ** -149 / U      # fp32's subnormal spacing, as a magnitude: exp(-104) is below it, and p rounds to 0
    if kind == "logistic":
        neg = torch.where(s < 0, -s, torch.zeros_like(s))
        l = (1 - t) * s + neg + torch.log1p(e)
        dl = p - t
        l_mag = abs(1 - t) * sd.abs() + neg.detach().double() + torch.log1p(e.detach().double()) + tiny
        dl_mag, l_sens, dl_sens = pd + abs(t) + tiny, (pd - t).abs(), pd * (1 - pd)
    elif kind == "lsgan":
        d = s - t
        l, dl = 0.5 * d * d, d
        l_mag, dl_mag = 0.5 * (sd.abs() + abs(t)) ** 2, sd.abs() + abs(t)
        l_sens, dl_sens = (sd - t).abs(), one
    elif kind == "hinge_gen":
        l, dl = -s, -torch.ones_like(s)
        l_mag, dl_mag, l_sens, dl_sens = sd.abs(), one, one, 0 * one
    else:
        sign = -1.0 if kind == "hinge_real" else 1.0
        d = 1 + sign * s
        l = torch.where(d < 0, torch.zeros_like(d), d)
        dl = torch.where(d > 0, sign * torch.ones_like(s), torch.zeros_like(s))
        l_mag, dl_mag, l_sens, dl_sens = 1 + sd.abs(), dl.detach().double().abs(), one, 0 * one
    dl = torch.where(torch.isnan(s), s, dl)       # the rule of include/vaegan_hip.h: a NaN logit, a NaN gradient
    return dict(p=p, l=l, dl=dl, l_mag=l_mag, dl_mag=dl_mag, l_sens=l_sens, dl_sens=dl_sens, p_mag=pd + tiny, p_sens=pd * (1 - pd))


def torch_loss(s, t, kind, div):
    """The same loss in torch's OWN forms (sum over the rows / div), for autograd and for the CPU test's comparison."""
    tn = torch.nn.functional
    if kind == "logistic":
        return tn.binary_cross_entropy_with_logits(s, torch.full_like(s, t), reduction="sum") / div
    if kind == "lsgan":
        return 0.5 * tn.mse_loss(s, torch.full_like(s, t), reduction="sum") / div
    if kind == "hinge_gen":
        return (-s).sum() / div
    return torch.relu(1 - s if kind == "hinge_real" else 1 + s).sum() / div


def gan_loss(logit, kind, target, divisor=None, gscale=1.0, dtype=torch.float64):
    """ops.gan_loss: the losses on a logit vector.  Magnitudes are those of the evaluation alone (the logit is given)."""
    s = _c(logit, dtype)
    t = f32(target)
    div = float(divisor if divisor is not None else s.numel())
    r = terms(s, t, kind)
    c = f32(gscale) / div
    return dict(p=r["p"], p_mag=r["p_mag"], loss=_sum64(r["l"]) / div, loss_mag=r["l_mag"].sum() / div,
                glogit=c * r["dl"], glogit_mag=abs(c) * r["dl_mag"] + 2.0 ** -149 / U)


def dot_gan_loss(feat, w, bias, kind, target, divisor=None, dtype=torch.float64, grads=True):
    """ops.dot_gan_loss_fwd and, with ``grads``, the backward at an upstream gradient of 1."""
    f, wv = _c(feat, dtype), _c(w, dtype).reshape(-1)
    b = _c(bias, dtype) if bias is not None else torch.zeros(1, dtype=dtype)
    t = f32(target)
    B, Kdim = f.shape
    div = float(divisor if divisor is not None else B)
    s = f @ wv + b
    smag = f.double().abs() @ wv.double().abs() + b.double().abs()
    r = terms(s, t, kind)
    out = dict(logit=s, logit_mag=smag, p=r["p"], p_mag=r["p_mag"] + r["p_sens"] * smag,
               loss=_sum64(r["l"]) / div, loss_mag=(r["l_mag"] + r["l_sens"] * smag).sum() / div,
               dlogit=r["dl"] / div, dlogit_mag=(r["dl_mag"] + r["dl_sens"] * smag) / div + 2.0 ** -149 / U)
    if kind in ("hinge_real", "hinge_fake"):
        d = 1 - s.double() if kind == "hinge_real" else 1 + s.double()
        out["tie"] = d.abs() <= logit_k(Kdim) * U * smag
    else:
        out["tie"] = torch.zeros(B, dtype=torch.bool)
    if grads:
        fl, wl, bl = f.clone().requires_grad_(), wv.clone().requires_grad_(), b.clone().requires_grad_()
        torch_loss(fl @ wl + bl, t, kind, div).backward()
        dm = out["dlogit_mag"]
        out.update(gfeat=fl.grad, gfeat_mag=dm[:, None] * wv.double().abs()[None, :],
                   gw=wl.grad, gw_mag=(dm[:, None] * f.double().abs()).sum(0), gb=bl.grad, gb_mag=dm.sum().reshape(1))
    return out


# ------------------------------------------------------------------------------------- seeded inputs, by case
# B: 16 rows per workgroup -- one row, a partial workgroup, a full one, a second one with one row, a third
EDGE_B, EDGE_B_K = (1, 15, 16, 17, 33), (260, 2048)
# K: the scalar loop (1, 3, 70, 255), the 16-byte loop below one stride of 256 (4), at it (256), past it with a tail (260)
# and eight strides (2048: the head's size)
EDGE_K, EDGE_K_B = (1, 3, 4, 70, 255, 256, 260, 2048), 17
SHAPES = tuple(sorted({(b, k) for b in EDGE_B for k in EDGE_B_K} | {(EDGE_K_B, k) for k in EDGE_K}))

# exact logits to plant: 0, the hinge ties and their fp32 neighbours, where fp32's sigmoid rounds to 1 (17), and the
# saturated / underflowing range of the issue's table
NEAR_ONE = (1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23)
PLANTED = (0.0, 1.0, -1.0, NEAR_ONE[0], NEAR_ONE[1], -NEAR_ONE[0], -NEAR_ONE[1], 17.0, -17.0, 40.0, -40.0, 104.0, -104.0)


@functools.lru_cache(maxsize=None)
def head_inputs(shape):
    """Features of order one (what a LeakyReLU leaves: a fifth of the negative side), a weight that puts the logits at
    order one -- both sides of 0 and of the hinge's +-1 -- and a bias."""
    B, Kdim = shape
    feat = torch.nn.functional.leaky_relu(randn(B, Kdim, seed=2400 + B), 0.2)
    w = randn(1, Kdim, seed=2401 + Kdim) * (1.5 / math.sqrt(Kdim))
    return dict(feat=feat, w=w, bias=torch.tensor([0.25]))


def planted_inputs(values=PLANTED, Kdim=8):
    """Rows whose logit IS the planted fp32 number: a one-hot weight and a zero bias (every other product is an exact 0)."""
    vals = torch.tensor(values, dtype=torch.float32)
    feat = torch.zeros(len(values), Kdim)
    feat[:, 3] = vals
    feat[:, 5] = 123.0           # against a zero weight
    w = torch.zeros(1, Kdim)
    w[0, 3] = 1.0
    return dict(feat=feat, w=w, bias=torch.zeros(1), logits=vals)
