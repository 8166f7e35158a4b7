"""References for the loss / elementwise kernels (csrc/losses.hip, channel_sum of csrc/bn.hip) and the seeded inputs
the CPU and the GPU tests share.  A plain module: nothing here touches a GPU.

One function per operation, in torch on the CPU, straight from the formulas in the header of losses.hip and in
oracle/steps.py.  Every function takes fp32 tensors (what the kernels get), computes in ``dtype`` (fp64: the reference;
fp32: the same expressions as an honest fp32 evaluation, which is where the GPU tolerances come from -- see
tests/test_losses_cpu.py) and returns a dict of outputs, gradients (torch.autograd on leaves of ``dtype``) and, under
``<name>_mag``, the magnitude each of them is judged against: the same expression with every term replaced by its
absolute value; for a sum, the sum of |term|.  Errors are judged per element, |got - ref| <= k 2^-24 magnitude.

Sums: the kernels add fp32 terms in fp64 (channel_sum, the loss scalars, the total KL) -- restated here as
``_sum64``: terms in ``dtype``, added in fp64, rounded to ``dtype`` -- except the per-row KL, which a wavefront adds in
fp32 (restated with a plain sum in ``dtype``).
"""
import functools

import torch

U = 2.0 ** -24                      # unit roundoff of fp32: the unit of every per-element bound
KINDS = {"lrelu": 0, "tanh": 1, "sigmoid": 2}      # VG_EW_* of include/vaegan_hip.h

# Worst |fp32 restatement - fp64| / magnitude over every input set below, in units of 2^-24, as
# tests/test_losses_cpu.py measured it (its docstring has the table).  K = 4 x that: the GPU's per-element tolerance
# (the factor covers expf / logf / tanhf of the device differing from the host's by a couple of ulp).
FP32_WORST = {
    "act_bwd": 2.3, "scale_by_scalar": 1.0, "sqdiff_ga": 1.8,
    "bias_act_y": 2.0, "bias_act_gx": 10.3, "bias_act_gb": 3.6, "channel_sum": 0.7,
    "rkl_z": 2.6, "rkl_rows": 3.0, "rkl_gmu": 2.0, "rkl_glv": 2.5, "bce_gp": 3.2,
}
K = {op: 4.0 * v for op, v in FP32_WORST.items()}
REL_KL = REL_SQDIFF = 2e-6          # reduced scalars: the figures of test_loss_kats
REL_BCE = 1e-5


def f32(v):
    """A Python float as the kernel receives it (ctypes c_float)."""
    return float(torch.tensor(v, dtype=torch.float32))


def _c(t, dtype):
    return None if t is None else t.detach().to("cpu", dtype)


def _sum64(t, dim=None):
    s = t.double().sum() if dim is None else t.double().sum(dim)
    return s.to(t.dtype)


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def act(v, kind):
    if kind == "lrelu":
        return torch.nn.functional.leaky_relu(v, 0.2)
    return torch.tanh(v) if kind == "tanh" else torch.sigmoid(v)


# ------------------------------------------------------------------------------------------------ the operations
def act_bwd(gy, y, kind, dtype=torch.float64):
    """gx from the saved OUTPUT y: LeakyReLU g or 0.2 g by the sign of y, tanh g (1 - y^2), sigmoid g y (1 - y)."""
    g, y = _c(gy, dtype), _c(y, dtype)
    if kind == "lrelu":
        gx = torch.where(y > 0, g, 0.2 * g)
        mag = gx.abs()
    elif kind == "tanh":
        gx, mag = g * (1 - y * y), g.abs() * (1 + y * y)
    else:
        gx, mag = g * y * (1 - y), g.abs() * y.abs() * (1 + y.abs())
    return dict(gx=gx, gx_mag=mag.double())


def scale_by_scalar(g, s, dtype=torch.float64):
    out = _c(g, dtype) * _c(s, dtype)
    return dict(out=out, out_mag=out.abs().double())


def sqdiff(a, b, scale, gscale=1.0, dtype=torch.float64):
    """loss = scale sum (a - b)^2;  ga = gscale d loss / d a = (gscale 2 scale) (a - b), the factor an fp32 product."""
    a, b = _c(a, dtype).requires_grad_(), _c(b, dtype)
    d = a - b
    loss = scale * _sum64(d * d)
    (ga,) = torch.autograd.grad(loss, a)
    gs = f32(gscale)
    return dict(loss=loss.detach(), ga=gs * ga, ga_mag=(abs(gs) * 2 * scale * (a.abs() + b.abs())).detach().double())


def bias_act(x, bias, kind, gy=None, dtype=torch.float64):
    """y = act(x + bias[c]) on (B, C, HW); with gy: gx and gb = sum over (B, HW) of gx, by autograd."""
    x = _c(x, dtype).requires_grad_()
    b = _c(bias, dtype).requires_grad_() if bias is not None else None
    v = x if b is None else x + b.view(1, -1, 1)
    y = act(v, kind)
    av = x.detach().abs().double() + (0 if b is None else b.detach().abs().double().view(1, -1, 1))
    yd = y.detach().double()
    if kind == "lrelu":
        y_mag = torch.where(v.detach().double() > 0, av, 0.2 * av)
    elif kind == "tanh":
        y_mag = torch.tanh(av)
    else:       # the relative condition of the sigmoid in its argument is at most |v| <= |x| + |b|; it never exceeds 1
        y_mag = torch.clamp(yd * (1 + av), max=1.0)
    out = dict(y=y.detach(), y_mag=y_mag)
    if gy is not None:
        g = _c(gy, dtype)
        grads = torch.autograd.grad(y, [x] if b is None else [x, b], g)
        out["gx"] = grads[0]
        out["gx_mag"] = act_bwd(g, yd, kind)["gx_mag"]
        if b is not None:
            out["gb"] = grads[1]
            out["gb_mag"] = out["gx_mag"].sum((0, 2))
    return out


def channel_sum(g, dtype=torch.float64):
    g = _c(g, dtype)
    g = g.reshape(g.shape[0], g.shape[1], -1)
    return dict(out=_sum64(g, (0, 2)), out_mag=g.abs().double().sum((0, 2)))


def reparam_kl(mu, lv, eps, beta, gz=None, gkl=None, dtype=torch.float64):
    """z = mu + eps e^(lv/2), rows[b] = -1/2 sum_j (1 + lv - mu^2 - e^lv), kl = beta sum_b rows[b]; with gz and / or
    gkl (upstream gradients of z and of the KL scalar) the gradients of z . gz + gkl kl, by autograd."""
    mu, lv, eps = _c(mu, dtype).requires_grad_(), _c(lv, dtype).requires_grad_(), _c(eps, dtype)
    z = mu + eps * torch.exp(0.5 * lv)
    rows = -0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp(), 1)
    kl = beta * _sum64(rows)
    md, ld, ed = mu.detach().double(), lv.detach().double(), eps.double()
    out = dict(z=z.detach(), kl=kl.detach(), rows=rows.detach(),
               z_mag=md.abs() + ed.abs() * torch.exp(0.5 * ld),
               rows_mag=0.5 * torch.sum(1 + ld.abs() + md * md + ld.exp(), 1))
    if gz is not None or gkl is not None:
        gzd = torch.zeros_like(md) if gz is None else _c(gz, torch.float64)
        kb = 0.0 if gkl is None else abs(float(gkl)) * beta
        total = 0
        if gz is not None:
            total = total + (z * _c(gz, dtype)).sum()
        if gkl is not None:
            total = total + _c(gkl, dtype) * kl
        out["gmu"], out["glv"] = torch.autograd.grad(total, [mu, lv])
        out["gmu_mag"] = kb * md.abs() + gzd.abs()
        out["glv_mag"] = (gzd * ed).abs() * 0.5 * torch.exp(0.5 * ld) + kb * 0.5 * (ld.exp() + 1)
    return out


def bce(p, target, divisor=None, gscale=1.0, dtype=torch.float64):
    """nn.BCELoss against a constant label: the logs clamped at -100, the gradient's denominator p (1 - p) at 1e-12
    (ATen's binary_cross_entropy and its backward); the mean runs over ``divisor``.  Written out, not through
    F.binary_cross_entropy, which refuses a probability outside [0, 1] (a NaN included) where the kernel and
    log().clamp(min=-100) answer NaN; tests/test_losses_cpu.py holds the two together on [0, 1]."""
    p = _c(p, dtype)
    t = f32(target)
    div = float(divisor if divisor is not None else p.numel())
    lp, l1p = torch.log(p).clamp(min=-100.0), torch.log(1 - p).clamp(min=-100.0)
    loss = _sum64(-(t * lp + (1 - t) * l1p)) / div
    den = (p * (1 - p)).clamp(min=f32(1e-12))          # ATen's EPSILON is the fp32 number, in its fp64 kernel too
    c = f32(gscale) / div
    # + fp32's subnormal spacing under the division: (gscale / divisor) (p - t) underflows for the planted p = 2^-149
    mag = (abs(c) * (p.abs() + abs(t)) + 2.0 ** -149 / U) / den.abs()
    return dict(loss=loss, gp=c * (p - t) / den, gp_mag=mag.double())


def dot_sigmoid_bce(feat, w, bias, target, dtype=torch.float64):
    """The fused head: p = sigmoid(feat . w + bias), its mean BCE and dlogit = dBCE/dp p (1 - p)."""
    f, w, b = _c(feat, dtype), _c(w, dtype).reshape(-1), _c(bias, dtype)
    p = torch.sigmoid(f @ w + b)
    r = bce(p, target, dtype=dtype)
    return dict(p=p, loss=r["loss"], dlogit=r["gp"] * p * (1 - p))


def bn_act(x, gamma, beta, act_name, eps=1e-5, momentum=0.1, dtype=torch.float64):
    """Train-mode BatchNorm + activation from its definition (running statistics from 0 / 1), every output."""
    x, gamma, beta = _c(x, dtype), _c(gamma, dtype), _c(beta, dtype)
    x3 = x.reshape(x.shape[0], x.shape[1], -1)
    n = x3.shape[0] * x3.shape[2]
    mean = x3.mean((0, 2))
    var = ((x3 - mean.view(1, -1, 1)) ** 2).mean((0, 2))
    invstd = 1 / torch.sqrt(var + eps)
    pre = (x3 - mean.view(1, -1, 1)) * (invstd * gamma).view(1, -1, 1) + beta.view(1, -1, 1)
    y = {"none": lambda t: t, "relu": torch.relu, "lrelu": lambda t: torch.nn.functional.leaky_relu(t, 0.2)}[act_name](pre)
    return dict(y=y.reshape(x.shape), mean=mean, invstd=invstd, rm=momentum * mean,
                rv=(1 - momentum) + momentum * var * (n / (n - 1) if n > 1 else 1.0))


def affine_act(x, scale, shift, act_name, dtype=torch.float64):
    x, scale, shift = _c(x, dtype), _c(scale, dtype), _c(shift, dtype)
    x3 = x.reshape(x.shape[0], x.shape[1], -1)
    pre = x3 * scale.view(1, -1, 1) + shift.view(1, -1, 1)
    y = {"none": lambda t: t, "relu": torch.relu, "lrelu": lambda t: torch.nn.functional.leaky_relu(t, 0.2)}[act_name](pre)
    return dict(y=y.reshape(x.shape))


# ------------------------------------------------------------------------------------- seeded inputs, by case
# one whole sweep of the capped grid (2048 workgroups x 256 threads x 4) + one more group of 256 x 4 + a 3-element tail;
# also past the 1024 partial sums of the squared-difference kernel
FLAT_BIG = 2048 * 256 * 4 + 256 * 4 + 3
FLAT_SIZES = (1, 3, 4, 5, 255, 1023, 1024, 1027, FLAT_BIG)

BIAS_SHAPES = ((1, 1, 1), (2, 3, 1), (3, 7, 1), (3, 2048, 1), (2, 3, 4), (2, 5, 8), (2, 3, 5), (5, 3, 6), (2, 3, 4096))
BIAS_FORMS = ("none", "decades", "small")
CSUM_SHAPES = ((1, 1, 1), (5, 3, 1), (128, 2048, 1), (3, 7, 5), (2, 130, 12), (4, 3, 4096), (3, 4100, 4))

RKL_B, RKL_D = (1, 5, 16, 17, 300), (1, 63, 64, 65, 128, 200)
RKL_SHAPES = tuple(sorted({(b, d) for b in RKL_B for d in (65, 128)} | {(b, d) for b in (1, 17) for d in RKL_D}))

BCE_B = (1, 63, 64, 65, 256, 257, 1000)
BCE_LABELS = (0.0, 0.1, 0.9, 1.0)
BCE_PLANTED = (0.0, 1.0, 2.0 ** -149, 1.0 - 2.0 ** -24, 0.5)


@functools.lru_cache(maxsize=None)
def flat_inputs(n):
    """gy, a pre-activation x (the saved outputs are act(x) in fp32), and the pair (a, b) of the squared difference."""
    return dict(gy=randn(n, seed=100), x=2 * randn(n, seed=101), a=randn(n, seed=102), b=randn(n, seed=103))


def bias_values(C, form):
    """'decades': 10^c (c + 1) -- neighbouring channels a factor of ten apart, so no wrong channel index passes -- as
    long as that is an fp32 number (C <= 37); the 2048-channel shape repeats the seven decades with a mantissa
    1 + c / 4096 that no other channel has.  tanh and sigmoid saturate at such a bias, so 'small' adds distinct values
    of order one, (c mod 16 - 7.5) / 4 + c / (16 C), which those two tell apart."""
    if form == "none":
        return None
    c = torch.arange(C, dtype=torch.float64)
    if form == "small":
        return ((c % 16 - 7.5) / 4 + c / (16 * C)).float()
    if C <= 37:
        return (10.0 ** c * (c + 1)).float()
    return (10.0 ** (c % 7) * (1 + c / 4096)).float()


@functools.lru_cache(maxsize=None)
def bias_inputs(shape):
    B, C, HW = shape
    return dict(x=2 * randn(B, C, HW, seed=110), gy=randn(B, C, HW, seed=111))


@functools.lru_cache(maxsize=None)
def csum_input(shape):
    return 1e3 + randn(*shape, seed=120)          # a large common offset: an fp32 accumulator would show


@functools.lru_cache(maxsize=None)
def rkl_inputs(shape):
    """logvar spans +-8; one row (the middle one) is mu = 0, logvar = 0: its KL is exactly 0."""
    B, D = shape
    mu, eps, gz = randn(B, D, seed=130), randn(B, D, seed=131), randn(B, D, seed=132)
    lv = (torch.rand(B, D, generator=torch.Generator().manual_seed(133)) * 16 - 8)
    lv.view(-1)[0], lv.view(-1)[-1] = -8.0, 8.0
    zero_row = B // 2
    if B > 1:
        mu[zero_row], lv[zero_row] = 0.0, 0.0
    return dict(mu=mu, lv=lv, eps=eps, gz=gz, gkl=torch.tensor(0.75), zero_row=zero_row if B > 1 else None)


@functools.lru_cache(maxsize=None)
def bce_input(B):
    """sigmoid(4 randn) with the saturated / exact values planted from the middle on (as many as fit)."""
    p = torch.sigmoid(4 * randn(B, seed=140))
    planted = list(range(B // 2, min(B // 2 + len(BCE_PLANTED), B)))
    for i, v in zip(planted, BCE_PLANTED):
        p[i] = v
    return p, planted


def worst_ratio(got, ref, mag):
    """max |got - ref| / magnitude in units of 2^-24 (0 where both the error and the magnitude are 0)."""
    err = (got.detach().cpu().double() - ref.double()).abs()
    mag = mag.double().expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / mag)
    return float(r.max() / U) if r.numel() else 0.0
