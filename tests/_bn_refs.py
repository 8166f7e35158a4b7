"""References for the BatchNorm kernels (csrc/bn.hip) and the seeded inputs the CPU and the GPU tests share.
A plain module: nothing here touches a GPU.

One function per entry point, in torch on the CPU, from the formulas in the header of bn.hip.  Every function takes
fp32 tensors (what the kernels get) and computes in ``dtype``:

  fp64  the reference.  Mean and variance by the two-pass formula (sum of (x - m)^2), everything else in fp64.
  fp32  the kernel's precision mix, restated: fp32 terms added in fp64 for the sums; mu, is, sc = gamma * is and
        sh = beta - mu * sc rounded to fp32; pre = x * sc + sh;  gx = sc * (g - c1 - ((x - mu) * is) * c2) with the
        product g * ((x - mu) * is) in fp32.  tests/test_bn_cpu.py measures how far this is from the reference; the
        GPU tolerances K come from that table (FP32_WORST), never from the kernel.

Every output comes with ``<name>_mag``, the magnitude it is judged against: the same expression with each term
replaced by its absolute value (y: |x sc| + |sh|; gx: |sc| (|g| + |c1| + |xhat c2|); shift: |beta| + |mu sc|; a sum:
the sum of |term|).  Errors are judged per element, |got - ref| <= K 2^-24 magnitude (+ an allowance, below).  An
ill-conditioned channel (|mean| >> std) is thereby held to what its inputs allow, a well-conditioned one to a few ulp.

The kink of ReLU / LeakyReLU: where |pre_ref| <= K["y"] 2^-24 pre_mag an honest evaluation may land on either side of
0.  bn_bwd returns that set as ``kink``: gx is not judged there, dbeta gets an allowance of the sum of |g| over the
channel's kink elements, dgamma of the sum of |g xhat|, and gx elsewhere in the channel |sc| times what that changes
c1 by plus |xhat| times what it changes c2 by.  The inputs are chosen so that the set is all but empty
(tests/test_bn_cpu.py asserts it: at most 1e-5 of a case's elements, none below 100 000 elements).

BatchNorm of one value per channel (count 1): the variance is 0, and the running variance takes the biased 0 (the
kernel's documented behaviour; F.batch_norm refuses the case).
"""
import functools

import torch

from _loss_refs import U, f32, randn, worst_ratio      # noqa: F401  (the unit 2^-24 and the helpers are shared)

ACTS = {"none": 0, "relu": 1, "lrelu": 2}      # VG_ACT_*
EPS = 1e-5

# Worst |fp32 restatement - fp64| / magnitude per output over every case below, in units of 2^-24, as
# tests/test_bn_cpu.py measured it (its docstring has the table), rounded up.  K = max(4 x that, 2): the GPU's
# per-element tolerance.  The factor 4 is for the order of the sums and fused multiply-adds, the floor of 2 for an
# output whose restatement happens to be exact.
FP32_WORST = {
    "y": 3.0, "mean": 1.0, "invstd": 1.0, "scale": 1.9, "shift": 3.3, "running_mean": 2.3, "running_var": 2.1,
    "gx": 11.0, "dgamma": 2.4, "dbeta": 1.6,
}
K = {name: max(4.0 * v, 2.0) for name, v in FP32_WORST.items()}


# ------------------------------------------------------------------ the host-side decisions of bn.hip, restated
NS_MAX, ONE_NT = 64, 1024


def make_slicing(B, C, HW):
    """(slices per channel, elements per slice) of the sums pass."""
    total = B * HW
    ns = min(max(2048 // C, 1), NS_MAX)
    per = max(-(-total // ns), 1024)
    per = (per + 3) // 4 * 4
    return -(-total // per), per


def make_apply_slicing(B, C, HW):
    total = B * HW
    ns = max(4096 // C, 1)
    per = max(-(-total // ns), 4096)
    per = (per + 3) // 4 * 4
    return -(-total // per), per


def bwd_path(B, C, HW, aligned=True):
    """'1d', 'one<2>', 'one<8>' or 'two': what vg_bn_act_bwd launches."""
    if HW == 1:
        return "1d"
    total = B * HW
    if HW % 4 == 0 and aligned and 4 <= total <= ONE_NT * 4 * 8 and C >= 128:
        return "one<2>" if total <= ONE_NT * 4 * 2 else "one<8>"
    return "two"


def finalize_regime(nslots):
    return "small" if nslots <= 64 else "wide" if nslots <= 4096 else "split"


# --------------------------------------------------------------------------------------------------- the cases
# shape -> (slices of the sums pass, slices of the apply pass, backward path)
TWO_PASS = {
    (10, 5, 21, 21): (5, 2, "two"),          # scalar loops, both passes sliced, ragged last slices
    (50, 3, 10, 10): (5, 2, "two"),          # vector loops, plane not a power of two
    (1, 3, 2, 2): (1, 1, "two"),             # one vector per channel
    (3, 7, 5, 1): (1, 1, "two"),             # 15 elements per channel
    (17, 3, 64, 64): (64, 17, "two"),        # the 64-slice cap
    (2, 2304, 2, 2): (1, 1, "one<2>"),       # 2048 / C < 1; backward: the one pass with two active lanes
    (8, 127, 4, 4): (1, 1, "two"),           # one channel short of the one pass
}
ONE_PASS = {
    (1, 128, 2, 2): (1, 1, "one<2>"),        # 4 per channel: the minimum
    (1025, 128, 2, 2): (5, 2, "one<2>"),     # 4100: ragged in <2>
    (32, 128, 16, 16): (8, 2, "one<2>"),     # 8192: the last shape of <2>
    (683, 128, 3, 4): (9, 3, "one<8>"),      # 8196: the first of <8>, ragged, division path
    (128, 128, 16, 16): (16, 8, "one<8>"),   # 32768: the last shape of the one pass
    (2731, 128, 3, 4): (16, 9, "two"),       # 32772: two passes again
}
SHAPES_2D = {**TWO_PASS, **ONE_PASS}
SHAPES_1D = tuple((B, C) for B in (1, 2, 7, 8, 9, 13) for C in (1, 31, 32, 33, 70)) + ((128, 33),)
MISALIGNED_SHAPES = ((50, 3, 10, 10), (32, 128, 16, 16), (1, 3, 2, 2))

# slot count -> the two channel counts it runs with
SLOT_CASES = {
    1: (1, 33), 7: (7, 32), 8: (8, 70), 9: (9, 31), 63: (1, 33), 64: (7, 70),
    65: (8, 9), 127: (31, 7), 128: (32, 1), 129: (33, 70), 1000: (9, 32), 4095: (7, 33), 4096: (8, 31),
    4097: (1, 33), 4160: (32, 70), 5000: (9, 31), 16384: (7, 70),
}
SLOT_K = 4          # values per slot

# seeds: case -> seed; a case whose first seed put an element on the kink (see the module docstring) got the next one
SEED_BUMP = {}


def case_seed(shape):
    return 1000 + 7 * (sum((i + 1) * 131 * d for i, d in enumerate(shape)) % 9973) + SEED_BUMP.get(tuple(shape), 0)


N_FAMILIES = 6


def channel_family(c, shift):
    return (c + shift) % N_FAMILIES


def _family_values(fam, n, g):
    """n values of a channel of family ``fam`` and its (gamma, beta), fp64."""
    r = torch.randn(n, generator=g, dtype=torch.float64)
    u = torch.rand(3, generator=g, dtype=torch.float64)
    gamma = 1.0 + 0.2 * (float(u[0]) - 0.5)
    sign = 1.0 if float(u[1]) < 0.5 else -1.0
    beta = sign * (0.2 + 0.1 * float(u[2]))              # away from 0: a channel of one value has pre = beta
    if fam == 0:
        v = 2 * r + 0.5
    elif fam == 1:                                        # |mean| / std around 50; pre crosses 0 three sigma out
        v, beta = 50 + r, 3 * gamma
    elif fam == 2:                                        # values around 1e3; alone in a channel (B = 1), such a value
        v = 1e3 * (1 + 0.3 * r)                           # has |x sc| = 3e5: pre = beta has to stand clear of 2^-24 of that
        beta = sign * (2.0 + float(u[2]))
    elif fam == 3:                                        # values around 1e-4: variance far below eps
        v = 1e-4 * (2 + r)
    elif fam == 4:                                        # constant: variance 0, invstd = 1 / sqrt(eps)
        v = torch.full((n,), 1.7, dtype=torch.float64)
    else:                                                 # gamma < 0 with a large beta
        v, gamma, beta = r - 0.3, -(1.5 + 0.2 * (float(u[0]) - 0.5)), 4.0
    if fam in (0, 2, 3, 4) and float(v.mean()) * gamma * beta > 0:
        beta = -beta          # sh = beta - mu sc does not cancel: y is judged against |x sc| + |sh|, which would hide it
    return v, gamma, beta


@functools.lru_cache(maxsize=None)
def bn_inputs(shape):
    """x, gy of ``shape`` ((B, C, H, W) or (B, C)), gamma, beta, and starting running statistics; channel c is of
    family (c + shift) % 6, the shift by case so that the three-channel cases do not all see the same three."""
    B, C = shape[0], shape[1]
    HW = 1
    for d in shape[2:]:
        HW *= d
    n = B * HW
    seed = case_seed(shape)
    g = torch.Generator().manual_seed(seed)
    shift = seed % N_FAMILIES
    x = torch.empty(C, n, dtype=torch.float64)
    gamma, beta = torch.empty(C, dtype=torch.float64), torch.empty(C, dtype=torch.float64)
    for c in range(C):
        x[c], gamma[c], beta[c] = _family_values(channel_family(c, shift), n, g)
    x = x.view(C, B, HW).permute(1, 0, 2).reshape(shape).contiguous().float()
    # the upstream gradient: N(0, 1) around +-0.5 by channel.  Centred on 0 it would leave c1 = sum(g) / n near 0 by
    # cancellation, and gx's magnitude, which knows |c1| but not sum |g| / n, would then understate what c1's own
    # rounding does to an element whose g is small too: the fp32 restatement reaches 50 x 2^-24 there, and K with it
    off = torch.where(torch.arange(C) % 2 == 0, 0.5, -0.5).view((1, C) + (1,) * (len(shape) - 2))
    gy = torch.randn(shape, generator=g) + off
    rm0 = torch.randn(C, generator=g)
    rv0 = 0.5 + torch.rand(C, generator=g)
    return dict(x=x, gy=gy, gamma=gamma.float(), beta=beta.float(), rm0=rm0, rv0=rv0, shift=shift)


def slot_sums(v, k=SLOT_K):
    """v: (C, n) fp32 values; slot j of channel c holds the fp32 sums of v[c, j*k:(j+1)*k] and of their fp32-rounded
    squares, added pairwise -- what a convolution epilogue writes, sum and sum of squares consistent (as
    _fp32_slot_sums of tests/test_bounds_gpu.py).  Returns stats[nslots][C][2] on the CPU."""
    def tree(a):
        while a.shape[-1] > 1:
            if a.shape[-1] % 2:
                a = torch.cat([a, torch.zeros_like(a[..., :1])], -1)
            a = a[..., 0::2] + a[..., 1::2]
        return a[..., 0]
    a = v.float().reshape(v.shape[0], -1, k)
    return torch.stack([tree(a), tree(a * a)], -1).permute(1, 0, 2).contiguous()


@functools.lru_cache(maxsize=None)
def slot_inputs(nslots, C):
    """stats[nslots][C][2] built from values of the channel families, the count, gamma / beta, running statistics,
    and ``clamped``: a channel whose sum-of-squares slots are scaled down to half of count * mean^2, so that
    s2 / n < m^2 and the variance clamp is what answers."""
    n = nslots * SLOT_K
    seed = case_seed((nslots, C, 77))
    g = torch.Generator().manual_seed(seed)
    shift = seed % N_FAMILIES
    v = torch.empty(C, n, dtype=torch.float64)
    gamma, beta = torch.empty(C, dtype=torch.float64), torch.empty(C, dtype=torch.float64)
    for c in range(C):
        v[c], gamma[c], beta[c] = _family_values(channel_family(c, shift), n, g)
    stats = slot_sums(v.float())
    clamped = C - 1
    s1, s2 = stats[:, clamped, 0].double().sum(), stats[:, clamped, 1].double().sum()
    assert float(s1) != 0.0
    stats[:, clamped, 1] = (stats[:, clamped, 1].double() * (0.5 * s1 * s1 / n / s2)).float()
    return dict(stats=stats, count=float(n), gamma=gamma.float(), beta=beta.float(), rm0=torch.randn(C, generator=g),
                rv0=0.5 + torch.rand(C, generator=g), clamped=clamped)


# ------------------------------------------------------------------------------------------------ the operations
def _c(t, dtype):
    return None if t is None else t.detach().to("cpu", dtype)


def _cv(t):
    return t.view(1, -1, 1)


def _act(pre, act):
    if act == "relu":
        return torch.relu(pre)
    return torch.nn.functional.leaky_relu(pre, 0.2) if act == "lrelu" else pre


def _coefficients(m, var, abs_mean, n, gamma, beta, eps, momentum, rm0, rv0, dtype):
    """mean / invstd / scale / shift / running statistics from the fp64 mean ``m`` and variance ``var`` of n values;
    abs_mean: the mean of |term| (the magnitude of the mean)."""
    out = {}
    eps = f32(eps)
    mu = m.to(dtype)
    is_ = (1.0 / torch.sqrt(var + eps)).to(dtype)
    gm, bt = _c(gamma, dtype), _c(beta, dtype)
    sc = gm * is_
    sh = bt - mu * sc
    out.update(mean=mu, mean_mag=abs_mean.double(), invstd=is_, invstd_mag=is_.abs().double(),
               scale=sc, scale_mag=sc.abs().double(), shift=sh, shift_mag=bt.abs().double() + (mu * sc).abs().double())
    mom = torch.tensor(f32(momentum), dtype=dtype)
    keep = torch.tensor(1.0, dtype=dtype) - mom
    unb = (var * n / (n - 1) if n > 1 else var).to(dtype)          # a count of 1: the biased variance, 0
    if rm0 is not None:
        r = _c(rm0, dtype)
        out.update(running_mean=keep * r + mom * mu, running_mean_mag=((keep * r).abs() + (mom * mu).abs()).double())
    if rv0 is not None:
        r = _c(rv0, dtype)
        out.update(running_var=keep * r + mom * unb, running_var_mag=((keep * r).abs() + (mom * unb).abs()).double())
    return out


def bn_coefficients_from_x(x, gamma, beta, eps=EPS, momentum=0.1, rm0=None, rv0=None, dtype=torch.float64):
    """vg_bn_stats: the coefficients of a train-mode BatchNorm from a pass over x.  The sums are fp64 in the kernel
    (x^2 is exact there), so mean and variance are fp64 in both precisions; the variance is the two-pass one."""
    x3 = x.detach().to("cpu", torch.float64).reshape(x.shape[0], x.shape[1], -1)
    n = x3.shape[0] * x3.shape[2]
    m = x3.mean((0, 2))
    var = ((x3 - _cv(m)) ** 2).mean((0, 2))
    return _coefficients(m, var, x3.abs().mean((0, 2)), n, gamma, beta, eps, momentum, rm0, rv0, dtype)


def bn_coefficients_from_slots(stats, count, gamma, beta, eps=EPS, momentum=0.1, rm0=None, rv0=None,
                               dtype=torch.float64):
    """vg_bn_finalize_stats: the same from stats[nslots][C][2], fp32 partial (sum, sum of squares).  The reference is
    the fp64 sum of the slots themselves; only E[x^2] - m^2 can be had from them, clamped at 0 as documented."""
    s = stats.detach().to("cpu", torch.float64)
    m = s[..., 0].sum(0) / count
    var = torch.clamp(s[..., 1].sum(0) / count - m * m, min=0.0)
    return _coefficients(m, var, s[..., 0].abs().sum(0) / count, count, gamma, beta, eps, momentum, rm0, rv0, dtype)


def bn_fwd(x, gamma, beta, act, eps=EPS, momentum=0.1, rm0=None, rv0=None, dtype=torch.float64):
    """vg_bn_act_fwd: y = act(x sc + sh) and the saved / running statistics."""
    out = bn_coefficients_from_x(x, gamma, beta, eps, momentum, rm0, rv0, dtype)
    x3 = _c(x, dtype).reshape(x.shape[0], x.shape[1], -1)
    sc, sh = _cv(out["scale"]), _cv(out["shift"])
    pre = x3 * sc + sh
    out["y"] = _act(pre, act).reshape(x.shape)
    out["y_mag"] = ((x3 * sc).abs() + sh.abs()).double().reshape(x.shape)
    return out


def bn_bwd(gy, x, gamma, beta, mean, invstd, act, dtype=torch.float64):
    """vg_bn_act_bwd from the saved fp32 mean / invstd (inputs, taken as they are):
    g = act'(pre) gy, dbeta = sum g, dgamma = sum g xhat, gx = sc (g - dbeta / n - xhat dgamma / n)."""
    shape = x.shape
    x3, g3 = (_c(t, dtype).reshape(shape[0], shape[1], -1) for t in (x, gy))
    n = x3.shape[0] * x3.shape[2]
    mu, is_ = _c(mean, dtype), _c(invstd, dtype)
    sc = _c(gamma, dtype) * is_
    sh = _c(beta, dtype) - mu * sc
    pre = x3 * _cv(sc) + _cv(sh)
    if act == "none":
        g = g3
    else:
        g = torch.where(pre > 0, g3, (0.0 if act == "relu" else 0.2) * g3)
    xhat = (x3 - _cv(mu)) * _cv(is_)
    t = g * xhat
    s1, s2 = g.double().sum((0, 2)), t.double().sum((0, 2))          # terms in ``dtype``, added in fp64
    c1, c2 = (s1 / n).to(dtype), (s2 / n).to(dtype)
    gx = _cv(sc) * (g - _cv(c1) - xhat * _cv(c2))
    out = dict(gx=gx.reshape(shape), dbeta=s1.to(dtype), dgamma=s2.to(dtype),
               gx_mag=(_cv(sc).abs() * (g.abs() + _cv(c1).abs() + (xhat * _cv(c2)).abs())).double().reshape(shape),
               dbeta_mag=g.abs().double().sum((0, 2)), dgamma_mag=t.abs().double().sum((0, 2)))
    # the kink set and what it allows
    if act == "none":
        kink = torch.zeros(x3.shape, dtype=torch.bool)
    else:
        pre_mag = (x3 * _cv(sc)).abs() + _cv(sh).abs()
        kink = pre.abs().double() <= K["y"] * U * pre_mag.double()
    ga, xa = g3.abs().double(), xhat.abs().double()
    allow_b = (ga * kink).sum((0, 2))
    allow_g = (ga * xa * kink).sum((0, 2))
    allow_x = _cv(sc).abs().double() * (_cv(allow_b) / n + xa * _cv(allow_g) / n)
    allow_x = torch.where(kink, torch.full_like(allow_x, float("inf")), allow_x)
    out.update(kink=kink.reshape(shape), dbeta_allow=allow_b, dgamma_allow=allow_g, gx_allow=allow_x.reshape(shape))
    return out


def ratio(got, ref, mag, allow=None):
    """max over elements of (|got - ref| - allowance)+ / magnitude, in units of 2^-24 (0 where nothing is left of the
    error, whatever the magnitude)."""
    err = (got.detach().cpu().double() - ref.double()).abs()
    if allow is not None:
        err = torch.clamp(err - allow.double(), min=0.0)
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    mag = mag.double().expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / mag)
    return float(r.max() / U) if r.numel() else 0.0
