"""What the torch restatements of the four objectives fused with the reparameterisation -- tests/_tc_refs.py, _dip_refs.py,
_mmd_refs.py, _klc_refs.py -- have in common to the letter; each re-exports what it uses, so a test imports its own
objective's module and nothing else.  What differs between two of them in more than a docstring (the MMD inputs draw a
prior sample, the KL-capacity inputs scale their dimensions) stays in its module."""
import torch


def make_inputs(B, D, seed=0):
    """mu ~ N(0,1); logvar ~ N(-1, 1.5^2) clamped to [-6, 2]; eps ~ N(0,1); gz ~ N(0,1) (a decoder's gradient); fp32."""
    g = torch.Generator().manual_seed(1000 * B + D + seed)
    mu = torch.randn(B, D, generator=g)
    lv = (torch.randn(B, D, generator=g) * 1.5 - 1.0).clamp_(-6.0, 2.0)
    eps = torch.randn(B, D, generator=g)
    gz = torch.randn(B, D, generator=g)
    return dict(mu=mu, lv=lv, eps=eps, gz=gz)


def gz_grads(lv, eps, gz, dtype=torch.float64):
    """The decoder's gradient through z = mu + eps exp(lv / 2): (gmu, glv)."""
    lv, eps, gz = (t.detach().to(dtype) for t in (lv, eps, gz))
    return gz, gz * eps * 0.5 * torch.exp(0.5 * lv)


def expected_grads(ref, lv, eps, gz=None, gloss=None, dtype=torch.float64):
    """What an objective's backward entry (vg_reparam_<objective>_bwd) writes for the upstream pair (gz or None, gloss as a float or None)."""
    gmu = torch.zeros_like(ref["gmu_loss"])
    glv = torch.zeros_like(ref["glv_loss"])
    if gloss is not None:
        gmu, glv = gmu + gloss * ref["gmu_loss"], glv + gloss * ref["glv_loss"]
    if gz is not None:
        a, b = gz_grads(lv, eps, gz, dtype)
        gmu, glv = gmu + a, glv + b
    return gmu, glv


def rel_err(got, ref):
    """max |got - ref| over the reference's largest magnitude."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def bound(ref32, ref64):
    """The project's convention (conftest.check_state, SURVEY KAT-0): max(1e-6, 5 x the fp32 restatement's own error)."""
    return max(1e-6, 5.0 * rel_err(ref32, ref64))
