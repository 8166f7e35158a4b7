"""CPU: the restatement of tests/_latent_refs.py against closed forms (it is the reference of the GPU tests), the C ABI of
csrc/agg_posterior.hip as far as the host alone can tell, and the argument checks of metrics.py / ops.agg_posterior_lse."""
import ctypes
import math
import os
import re

import pytest
import torch

import _latent_refs as L
from conftest import ROOT


def test_unit_posteriors_closed_form():
    """mu = 0, logvar = 0 in every row: q(z) is the prior, every log-sum-exp is log N + a standard normal's log-density,
    and the mutual information and total correlation vanish to fp64 rounding."""
    N, D = 50, 6
    mu, lv = torch.zeros(N, D), torch.zeros(N, D)
    z = torch.randn(N, D, generator=torch.Generator().manual_seed(3))
    lj, ld = L.lse(z, mu, lv)
    logn = -0.5 * (L.LOG_2PI + z.double() ** 2)
    assert torch.allclose(ld, math.log(N) + logn, rtol=0, atol=1e-12)
    assert torch.allclose(lj, math.log(N) + logn.sum(1), rtol=0, atol=1e-12)
    dec = L.elbo_decomposition(mu, lv, z)
    assert abs(float(dec["mi"])) < 1e-12 and abs(float(dec["tc"])) < 1e-12
    assert abs(float(dec["kl"])) < 1e-15 and int(dec["active_units"]) == 0
    assert abs(float(dec["dwkl"])) < 1e-12       # q(z_d) = p(z_d)


@pytest.mark.parametrize("shape", [(40, 40, 5), (17, 33, 9)])
def test_parts_sum_to_the_sampled_kl(shape):
    """MI + TC + DWKL = mean[log q(z|x) - log p(z)] identically: the two aggregate terms cancel."""
    M, N, D = shape
    i = L.make_inputs(M, N, D)
    dec = L.elbo_decomposition(i["mu"], i["lv"], i["z"], rows=torch.arange(M) % N)
    total = dec["mi"] + dec["tc"] + dec["dwkl"]
    assert abs(float(total - dec["identity"])) <= 1e-12 * max(1.0, abs(float(dec["identity"])))


def _planted(N=400, D=4):
    g = torch.Generator().manual_seed(11)
    labels = (torch.arange(N) % 2).to(torch.int64)
    mu = torch.randn(N, D, generator=g)
    lv = torch.full((N, D), -1.0)
    mu[:, 0] = torch.where(labels == 1, 3.0, -3.0)
    lv[:, 0] = -4.0
    z = mu + torch.randn(N, D, generator=g) * torch.exp(0.5 * lv)
    return mu, lv, z, labels


def test_planted_factor_is_found():
    """mu_0 = +-3 by a two-valued label, logvar_0 = -4, the other three dimensions independent of it: dimension 0 carries
    the whole bit (I = H(v) = log 2 up to the overlap of two Gaussians 6 apart at sigma 0.14: none), the others nothing
    but the estimator's noise."""
    mu, lv, z, labels = _planted()
    for dtype in (torch.float64, torch.float32):
        out = L.mig(mu, lv, z, labels, dtype=dtype)
        assert out["mi_matrix"].shape == (4, 1)
        assert int(out["mi_matrix"][:, 0].argmax()) == 0
        assert float(out["mig"]) >= 0.9, float(out["mig"])
        assert float(out["mi_matrix"][0, 0]) <= math.log(2.0) + 1e-6


def test_mig_subsampled_points_and_two_factors():
    mu, lv, z, labels = _planted()
    three = (torch.arange(400) % 3).to(torch.int64)            # independent of every dimension
    out = L.mig(mu, lv, z, torch.stack([labels, three], dim=1), n_eval_per_value=50)
    assert out["mi_matrix"].shape == (4, 2) and out["mig_per_factor"].shape == (2,)
    assert float(out["mig_per_factor"][0]) >= 0.9
    assert float(out["mi_matrix"][:, 1].abs().max()) < 0.1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vaegan_hip.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib_path():
    from disentangle_mlp_amd import build
    return build.build(verbose=False)


def test_entries_are_declared_bound_and_exported(lib_path):
    from disentangle_mlp_amd import _lib, ops
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    want = {"vg_agg_posterior_splits": (I, [I] * 4),
            "vg_agg_posterior_workspace_bytes": (Z, [I] * 4),
            "vg_agg_posterior_lse": (I, [P] * 5 + [I] * 4 + [P, Z, P])}
    text = _header()
    lib = ctypes.CDLL(lib_path)
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(lib, name) is not None, name
    for define, value in (("VG_AGG_POINT_TILE", ops.AGG_POINT_TILE), ("VG_AGG_ROW_TILE", ops.AGG_ROW_TILE)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % define, text).group(1)) == value


def test_host_side_plan(lib_path):
    """What needs no device: rejected sizes have no workspace and no split count, the workspace grows with the splits, a
    split count above the number of row tiles is clamped, `splits = 0` is a function of the sizes."""
    from disentangle_mlp_amd import _lib, ops
    lib = ctypes.CDLL(lib_path)
    for name in ("vg_agg_posterior_splits", "vg_agg_posterior_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    size, splits = lib.vg_agg_posterior_workspace_bytes, lib.vg_agg_posterior_splits
    for bad in ((0, 5, 5, 1), (5, 0, 5, 1), (5, 5, 0, 1), (5, 5, 1025, 1), (5, (1 << 24) + 1, 5, 1), (5, 5, 5, -1)):
        assert size(*bad) == 0 and splits(*bad) == 0, bad
    assert size(5, 5, 1024, 1) > 0 and size(1, 1, 1, 0) > 0
    R = ops.AGG_ROW_TILE
    assert splits(10, R + 1, 3, 7) == 2 and splits(10, R, 3, 7) == 1
    assert splits(10, 5 * R, 3, 4) == 3                       # ranges of 2 tiles: the fourth would be empty
    assert splits(10, 7 * R, 3, 7) == 7
    assert size(10, 7 * R, 3, 7) > size(10, 7 * R, 3, 1)
    assert size(10, R + 1, 3, 7) == size(10, R + 1, 3, 2)
    assert splits(10, 100 * R, 3, 0) == splits(10, 100 * R, 3, 0) >= 1


def test_mig_refuses_what_has_no_gap():
    from disentangle_mlp_amd import metrics
    mu, lv = torch.randn(12, 3), torch.zeros(12, 3)
    with pytest.raises(ValueError, match="single value"):
        metrics.mig(mu, lv, torch.zeros(12, dtype=torch.int64))
    with pytest.raises(ValueError, match="single value"):
        metrics.mig(mu, lv, torch.stack([torch.arange(12) % 2, torch.ones(12, dtype=torch.int64)], dim=1)[:, 1:])
    with pytest.raises(ValueError, match="two latent dimensions"):
        metrics.mig(mu[:, :1], lv[:, :1], torch.arange(12) % 2)
    with pytest.raises(ValueError, match="integer"):
        metrics.mig(mu, lv, torch.randn(12))


def test_op_refuses_cpu_tensors():
    from disentangle_mlp_amd import ops
    z, mu, lv = torch.zeros(3, 4), torch.zeros(5, 4), torch.zeros(5, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.agg_posterior_lse(z, mu, lv)
