"""CPU: the C ABI of the DIP-VAE kernels (vg_reparam_dip_*: declared, bound, exported, arguments validated before any
launch), `ops.reparam_dip_fwd` / `functional.reparam_dip` without a CPU path, the trainers' argument checks, and the torch
restatement the GPU tests compare against (tests/_dip_refs.py) checked against itself: the closed-form gradient the
kernels implement against autograd, the centred covariance against E[mu mu^T] - E[mu] E[mu]^T, and the fp32 evaluation
against the fp64 one."""
import ctypes

import pytest
import torch

import _dip_refs as R
from test_cabi_cpu import declared_symbols

NEW = ["vg_reparam_dip_bwd", "vg_reparam_dip_bwd_dev", "vg_reparam_dip_fwd", "vg_reparam_dip_fwd_dev",
       "vg_reparam_dip_workspace_bytes"]


@pytest.fixture(scope="module")
def lib():
    from disentangle_mlp_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_header_and_binding_list_the_new_entries():
    from disentangle_mlp_amd import _lib
    assert set(NEW) <= set(declared_symbols()) and set(NEW) <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 7                                  # entries are only added


def test_library_exports_the_new_entries(lib):
    from disentangle_mlp_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert getattr(raw, name) is not None, name
    assert lib.vg_reparam_dip_workspace_bytes(128, 128) > 0 and lib.vg_reparam_dip_workspace_bytes(1024, 1024) > 0
    assert lib.vg_reparam_dip_workspace_bytes(0, 128) == 0 and lib.vg_reparam_dip_workspace_bytes(128, 1025) == 0


def _fwd_args(B=4, D=8, **over):
    """Host addresses standing in for device pointers: every call below must return before a launch."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    a = dict(mu=p, lv=p, eps=p, z=p, out4=p, cov=p, mean=p, B=B, D=D, variant=1, beta=6.0, lambda_od=10.0, lambda_d=100.0,
             ws=p, ws_bytes=1 << 30, stream=None)
    a.update(over)
    return buf, a


def _bwd_args(B=4, D=8, **over):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    a = dict(gz=p, mu=p, lv=p, eps=p, cov=p, mean=p, gloss=p, variant=2, beta=6.0, lambda_od=10.0, lambda_d=100.0, gmu=p,
             glv=p, B=B, D=D, ws=p, ws_bytes=1 << 30, stream=None)
    a.update(over)
    return buf, a


_ids = dict(ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))


@pytest.mark.parametrize("over", [dict(mu=None), dict(lv=None), dict(eps=None), dict(z=None), dict(out4=None),
                                  dict(cov=None), dict(mean=None), dict(ws=None), dict(B=0), dict(D=1025), dict(B=1025),
                                  dict(D=0), dict(variant=0), dict(variant=3), dict(beta=None)], **_ids)
def test_forward_rejects_bad_arguments_before_any_launch(lib, over):
    dev = "beta" in over                                          # NULL beta_dev: the _dev entry only
    keep, a = _fwd_args(**over)
    if not dev:
        assert lib.vg_reparam_dip_fwd(*a.values()) == -1
        a["beta"] = ctypes.addressof(keep)                        # a beta word: the same refusal from the _dev twin
    assert lib.vg_reparam_dip_fwd_dev(*a.values()) == -1


@pytest.mark.parametrize("over", [dict(mu=None), dict(lv=None), dict(eps=None), dict(cov=None), dict(mean=None),
                                  dict(gmu=None), dict(glv=None), dict(ws=None), dict(B=0), dict(D=1025), dict(variant=0),
                                  dict(variant=3), dict(beta=None)], **_ids)
def test_backward_rejects_bad_arguments_before_any_launch(lib, over):
    dev = "beta" in over
    keep, a = _bwd_args(**over)
    if not dev:
        assert lib.vg_reparam_dip_bwd(*a.values()) == -1
        a["beta"] = ctypes.addressof(keep)
    assert lib.vg_reparam_dip_bwd_dev(*a.values()) == -1


def test_a_small_workspace_is_refused(lib):
    need = lib.vg_reparam_dip_workspace_bytes(4, 8)
    for args, fn, fn_dev in ((_fwd_args, lib.vg_reparam_dip_fwd, lib.vg_reparam_dip_fwd_dev),
                             (_bwd_args, lib.vg_reparam_dip_bwd, lib.vg_reparam_dip_bwd_dev)):
        keep, a = args(ws_bytes=need - 1)
        assert fn(*a.values()) == -2
        a["beta"] = ctypes.addressof(keep)
        assert fn_dev(*a.values()) == -2


def test_ops_and_functional_refuse_cpu_tensors(lib):
    from disentangle_mlp_amd import functional as F, ops
    t = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reparam_dip_fwd(t, t, t, 6.0, 10.0, 100.0, "i")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reparam_dip_bwd(None, t, t, t, t, t.double(), None, 6.0, 10.0, 100.0, "ii")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.reparam_dip(t, t, t, 6.0, 10.0, 100.0)
    with pytest.raises(ValueError, match="variant"):
        F.reparam_dip(t, t, t, 6.0, 10.0, 100.0, variant="iii")


def test_trainer_arguments():
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(TypeError, match="GANTrainer has no KL term: dip_vae does not apply"):
        T.GANTrainer(device="cpu", dip_vae=("i", 10.0, 100.0))
    with pytest.raises(TypeError, match="triple"):
        T.VAETrainer(device="cpu", dip_vae=10.0)
    for bad in (("iii", 1.0, 1.0), (1, 1.0, 1.0), ("i", -1.0, 1.0), ("ii", 1.0, -0.5), ("i", float("inf"), 1.0),
                ("ii", 1.0, float("nan"))):
        with pytest.raises(ValueError, match="dip_vae"):
            T.VAETrainer(device="cpu", dip_vae=bad)
    for cls in (T.VAETrainer, T.BetaVAEGANTrainer):
        with pytest.raises(ValueError, match="dip_vae and tc_decomposition"):
            cls(device="cpu", dip_vae=("i", 10.0, 100.0), tc_decomposition=(1.0, 1.0), dataset_size=100)
    plain, keyed = T.VAETrainer(device="cpu"), T.VAETrainer(device="cpu", dip_vae=("ii", 10, 0))
    assert plain.dip_vae is None and keyed.dip_vae == ("ii", 10.0, 0.0)
    keys = {plain._host_state_key(), keyed._host_state_key()}
    for other in (("i", 10, 0), ("ii", 9, 0), ("ii", 10, 1)):    # variant and both lambdas are frozen kernel arguments
        keys.add(T.VAETrainer(device="cpu", dip_vae=other)._host_state_key())
    assert len(keys) == 5
    assert set(plain.checkpoint(0)) == set(keyed.checkpoint(0))   # the option adds no checkpoint state
    assert T.BetaVAEGANTrainer(device="cpu", dip_vae=("i", 10, 100)).dip_vae == ("i", 10.0, 100.0)


# ---- the restatement against itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES + [("i", 0.0, 0.0)], ids=str)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_closed_form_gradient_is_autograd_s(shape, case):
    i = R.make_inputs(*shape)
    ref = R.reparam_dip(i["mu"], i["lv"], i["eps"], R.BETA, *case)
    gmu, glv = R.closed_form_grads(i["mu"], i["lv"], R.BETA, *case)
    assert R.rel_err(gmu, ref["gmu_loss"]) <= 1e-12 and R.rel_err(glv, ref["glv_loss"]) <= 1e-12


@pytest.mark.parametrize("variant", ["i", "ii"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_centred_covariance_is_the_moment_form(shape, variant):
    i = R.make_inputs(*shape)
    mu, lv = i["mu"].double(), i["lv"].double()
    a, b = R.covariance(mu, lv, variant), R.covariance_uncentred(mu, lv, variant)
    assert float((a - b).abs().max()) <= 1e-12 * max(float(a.abs().max()), 1.0)
    if shape[0] == 1 and variant == "i":
        assert float(a.abs().max()) == 0.0                        # a single sample has no spread


@pytest.mark.parametrize("case", R.CASES, ids=str)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_fp32_restatement_is_a_usable_yardstick(shape, case):
    """The bound of the GPU tests is 5 x the fp32 restatement's own error (floor 1e-6): on these inputs that error stays
    under 1e-5 for every compared tensor (largest seen: 2.3e-6, gmu at (256, 128) variant I), far from the 1e-3 a wrong
    term would show."""
    i = R.make_inputs(*shape)
    r64 = R.reparam_dip(i["mu"], i["lv"], i["eps"], R.BETA, *case)
    r32 = R.reparam_dip(i["mu"], i["lv"], i["eps"], R.BETA, *case, dtype=torch.float32)
    for k in R.COMPARED:
        assert R.rel_err(r32[k], r64[k]) <= 1e-5, (k, R.rel_err(r32[k], r64[k]))
