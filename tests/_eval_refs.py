"""fp64 reference for the chains of tests/_chain_refs.py with every BatchNorm in EVAL mode (running statistics), for
tests/test_eval_functions_gpu.py and tests/test_eval_mode_cpu.py.  A plain module: nothing here touches a GPU.

Shapes, parameters and route tables are those of _chain_refs (imported, not restated); only the BatchNorm differs:
F.batch_norm(training=False) on the case's non-trivial running buffers, which therefore never move.  A case that runs
without running buffers in train mode gets seeded ones here.  In eval mode the bias of a convolution that feeds a
BatchNorm is NOT cancelled: its gradient is an ordinary quantity and is compared like every other.
"""
import torch
import torch.nn.functional as F

from _chain_refs import (make_inputs, FWD_CASES, T_RING, T_THIN, LAST_BN_CASES, BN1D, check_routes,      # noqa: F401
                         rel_err)

CONV_TOL, BN_TOL = 3e-6, 2e-5          # the ceilings of tests/test_fused_functions_gpu.py
MARGIN = 2.0 ** -14
ACTS = {"none": 0, "relu": 1, "lrelu": 2}
CASES = FWD_CASES + (T_RING, T_THIN) + LAST_BN_CASES + (BN1D,)


# Seeds: the running statistics put the pre-activations elsewhere than the batch statistics of _chain_refs' seeds do, so
# the near-zero condition (no fp64 pre-activation within MARGIN * max |pre| of its channel from zero) is met by seeds of
# this table's own, searched on the CPU (first seed >= 100 with 1.5 x MARGIN to spare); (case, uses) -> seed.
SEEDS = {("fwd_s2_relu", 1): 103, ("fwd_s2_lrelu", 1): 103, ("fwd_s2_lrelu", 2): 107, ("fwd_s2_none", 1): 100,
         ("fwd_s1_relu", 1): 101, ("fwd_s1_lrelu", 1): 101, ("fwd_s1_none", 1): 101, ("convT_ring", 1): 101,
         ("convT_thin", 1): 131, ("last_bn_conv", 1): 101, ("last_bn_convT", 1): 106, ("bn1d", 1): 100}


def is_bn(L):
    return hasattr(L, "act")


def eval_inputs(case, uses=1):
    """`make_inputs` of the case (with ``uses`` inputs through the same layers), running buffers filled in where the
    train-mode case has none."""
    case = case._replace(uses=uses, seed=SEEDS[(case.name, uses)])
    inp = make_inputs(case)
    g = torch.Generator().manual_seed(7000 + case.seed)
    for L, p in zip(case.layers, inp["params"]):
        if is_bn(L) and p["rm"] is None:
            p["rm"] = 0.3 * torch.randn(L.c, generator=g)
            p["rv"] = 0.5 + torch.rand(L.c, generator=g)
    return inp


def _act(z, act):
    return z if act == "none" else (F.relu(z) if act == "relu" else F.leaky_relu(z, 0.2))


def chain_forward(layers, x, params, pres=None):
    t = x
    for i, (L, p) in enumerate(zip(layers, params)):
        if is_bn(L):
            z = F.batch_norm(t, p["rm"], p["rv"], p["gamma"], p["beta"], False, 0.0, L.eps)
            if pres is not None:
                pres.append(z.detach())
            t = _act(z, L.act)
        elif L.transposed:
            t = F.conv_transpose2d(t, p["w"], p["b"], stride=L.stride, padding=2, output_padding=L.stride - 1)
        else:
            t = F.conv2d(t, p["w"], p["b"], stride=L.stride, padding=2)
    return t


def run(case, inp, dtype=torch.float64):
    """Every use of the layers, loss = sum <y, gy>, one backward.  Returns dict(ys, gxs, grads: per layer {w, b} /
    {gamma, beta}, margin: min over BatchNorms and channels of min |pre| / max |pre|)."""
    params = []
    for p in inp["params"]:
        params.append({k: (v.detach().to(dtype).requires_grad_(k in ("w", "b", "gamma", "beta")) if v is not None else None)
                       for k, v in p.items()})
    xs = [x.detach().to(dtype).requires_grad_() for x in inp["xs"]]
    ys, pres, loss = [], [], 0.0
    for x, gy in zip(xs, inp["gys"]):
        y = chain_forward(case.layers, x, params, pres)
        ys.append(y.detach())
        loss = loss + (y * gy.to(dtype)).sum()
    loss.backward()
    worst = float("inf")
    for pre in pres:
        a = pre.abs().transpose(0, 1).reshape(pre.shape[1], -1)
        worst = min(worst, float((a.min(1).values / a.max(1).values).min()))
    return dict(ys=ys, gxs=[x.grad for x in xs],
                grads=[{k: p[k].grad for k in p if k in ("w", "b", "gamma", "beta")} for p in params], margin=worst)


def quantities(case, res):
    """Flat {name: (tensor, ceiling)}: y 3e-6; everything whose gradient passed through a BatchNorm backward 2e-5, the
    parameters of a chain's last convolution 3e-6."""
    has_bn = any(is_bn(L) for L in case.layers)
    q = {}
    for u, y in enumerate(res["ys"]):
        q[f"y{u}"] = (y, CONV_TOL)
        q[f"gx{u}"] = (res["gxs"][u], BN_TOL if has_bn else CONV_TOL)
    for i, L in enumerate(case.layers):
        after = case.layers[i + (0 if is_bn(L) else 1):]
        tol = BN_TOL if any(is_bn(M) for M in after) else CONV_TOL
        for k, v in res["grads"][i].items():
            q[f"g{k}.{i}"] = (v, tol)
    return q
