"""CPU: the C ABI of the beta-TCVAE kernels (vg_reparam_tc_*: declared, bound, exported, arguments validated before any
launch), `ops.reparam_tc_fwd` without a CPU path, the trainers' argument checks, and the torch restatement the GPU tests
compare against (tests/_tc_refs.py) checked against itself: the identity mi + tc + dwkl = sum_i (lqzx_i - lpz_i),
gradients that do not depend on the dataset size, and the closed-form gradient the kernels implement against autograd."""
import ctypes

import pytest
import torch

import _tc_refs as R
from test_cabi_cpu import declared_symbols

NEW = ["vg_reparam_tc_bwd", "vg_reparam_tc_bwd_dev", "vg_reparam_tc_fwd", "vg_reparam_tc_fwd_dev",
       "vg_reparam_tc_workspace_bytes"]


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
    assert lib.vg_reparam_tc_workspace_bytes(128, 128) > 0
    assert lib.vg_reparam_tc_workspace_bytes(0, 128) == 0 and lib.vg_reparam_tc_workspace_bytes(128, 1025) == 0


def _fwd_args(B=4, D=8, **over):
    """Host addresses standing in for device pointers: every call below must return before a launch."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    a = dict(mu=p, lv=p, eps=p, z=p, out4=p, lse_joint=p, lse_dim=p, B=B, D=D, alpha=1.0, beta=6.0, gamma=1.0, log_bn=13.0,
             ws=p, ws_bytes=1 << 30, stream=None)
    a.update(over)
    return buf, a


def _bwd_args(B=4, D=8, **over):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    a = dict(gz=p, mu=p, lv=p, eps=p, z=p, lse_joint=p, lse_dim=p, gloss=p, alpha=1.0, beta=6.0, gamma=1.0, gmu=p, glv=p,
             B=B, D=D, ws=p, ws_bytes=1 << 30, stream=None)
    a.update(over)
    return buf, a


@pytest.mark.parametrize("over", [dict(mu=None), dict(lv=None), dict(eps=None), dict(z=None), dict(out4=None),
                                  dict(lse_joint=None), dict(lse_dim=None), dict(ws=None), dict(B=0), dict(D=1025),
                                  dict(B=1025), dict(D=0), dict(beta=None)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_forward_rejects_bad_arguments_before_any_launch(lib, over):
    dev = "beta" in over                                          # NULL beta_dev: the _dev entry only
    keep, a = _fwd_args(**over)
    if not dev:
        assert lib.vg_reparam_tc_fwd(*a.values()) == -1
        a["beta"] = ctypes.addressof(keep)                        # a beta word: the same refusal from the _dev twin
    assert lib.vg_reparam_tc_fwd_dev(*a.values()) == -1


@pytest.mark.parametrize("over", [dict(mu=None), dict(lv=None), dict(eps=None), dict(z=None), dict(lse_joint=None),
                                  dict(lse_dim=None), dict(gmu=None), dict(glv=None), dict(ws=None), dict(B=0),
                                  dict(D=1025), dict(beta=None)],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_backward_rejects_bad_arguments_before_any_launch(lib, over):
    dev = "beta" in over
    keep, a = _bwd_args(**over)
    if not dev:
        assert lib.vg_reparam_tc_bwd(*a.values()) == -1
        a["beta"] = ctypes.addressof(keep)
    assert lib.vg_reparam_tc_bwd_dev(*a.values()) == -1


def test_a_small_workspace_is_refused(lib):
    _, a = _fwd_args(ws_bytes=lib.vg_reparam_tc_workspace_bytes(4, 8) - 1)
    assert lib.vg_reparam_tc_fwd(*a.values()) == -2
    _, a = _bwd_args(ws_bytes=lib.vg_reparam_tc_workspace_bytes(4, 8) - 1)
    assert lib.vg_reparam_tc_bwd(*a.values()) == -2


def test_ops_refuse_cpu_tensors(lib):
    from disentangle_mlp_amd import functional as F, ops
    t = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reparam_tc_fwd(t, t, t, 6.0, 1.0, 1.0, 13.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.reparam_tc(t, t, t, 6.0, dataset_size=100)
    with pytest.raises(ValueError, match="dataset_size"):
        F.reparam_tc(t, t, t, 6.0)


def test_trainer_arguments():
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(TypeError, match="has no KL term"):
        T.GANTrainer(device="cpu", tc_decomposition=(1.0, 1.0))
    with pytest.raises(TypeError, match="pair"):
        T.VAETrainer(device="cpu", tc_decomposition=1.0)
    with pytest.raises(ValueError, match="dataset_size"):
        T.VAETrainer(device="cpu", tc_decomposition=(1.0, 1.0), dataset_size=0)
    tr = T.VAETrainer(device="cpu", tc_decomposition=(1, 2))
    assert tr.tc_decomposition == (1.0, 2.0) and tr.dataset_size is None
    with pytest.raises(ValueError, match="dataset_size"):        # before anything runs
        tr.step(torch.zeros(2, 3, 64, 64))
    assert tr.iteration == 0
    plain, keyed = T.VAETrainer(device="cpu"), T.VAETrainer(device="cpu", tc_decomposition=(1, 2), dataset_size=50)
    assert plain.tc_decomposition is None and plain._host_state_key() != keyed._host_state_key()
    assert keyed._host_state_key() != T.VAETrainer(device="cpu", tc_decomposition=(1, 2), dataset_size=51)._host_state_key()
    assert set(plain.checkpoint(0)) == set(keyed.checkpoint(0))   # the option adds no checkpoint state

    class Loader:
        dataset = range(321)

        def __iter__(self):
            return iter(())

    tr._dataset_size_from(Loader())
    assert tr.dataset_size == 321
    keyed._dataset_size_from(Loader())
    assert keyed.dataset_size == 50                               # a given one stays


# ---- the restatement against itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7), (17, 65)], ids=str)
@pytest.mark.parametrize("weights", R.WEIGHTS, ids=str)
def test_restatement_identity_and_dataset_size(shape, weights):
    i = R.make_inputs(*shape)
    a = R.reparam_tc(i["mu"], i["lv"], i["eps"], *weights, dataset_size=R.DATASET_SIZE)
    b = R.reparam_tc(i["mu"], i["lv"], i["eps"], *weights, dataset_size=1000)
    for r in (a, b):                                              # mi + tc + dwkl = sum_i (lqzx_i - lpz_i), for every N
        total = float(r["mi"] + r["tc"] + r["dwkl"])
        assert abs(total - float(r["identity"])) <= 1e-11 * max(abs(float(r["identity"])), 1.0)
    assert float(a["identity"]) == float(b["identity"])
    assert float(a["tc"]) != float(b["tc"]) or shape[0] == 1      # N moves the values of the parts ...
    for k in ("gmu_loss", "glv_loss"):                            # ... and no gradient
        assert R.rel_err(a[k], b[k]) <= 1e-13, k


@pytest.mark.parametrize("shape", [(5, 7), (17, 65)], ids=str)
@pytest.mark.parametrize("weights", R.WEIGHTS + [(1.0, 1.0, 1.0)], ids=str)
def test_closed_form_gradient_is_autograd_s(shape, weights):
    i = R.make_inputs(*shape)
    ref = R.reparam_tc(i["mu"], i["lv"], i["eps"], *weights)
    gmu, glv = R.closed_form_grads(i["mu"], i["lv"], i["eps"], *weights)
    assert R.rel_err(gmu, ref["gmu_loss"]) <= 1e-12 and R.rel_err(glv, ref["glv_loss"]) <= 1e-12


def test_fp32_restatement_is_a_usable_yardstick():
    """The bound of the GPU tests is 5 x the fp32 restatement's own error (floor 1e-6): on these inputs that error is
    1e-8 ... 1e-6, far from the 1e-3 a wrong term would show."""
    i = R.make_inputs(17, 65)
    r64 = R.reparam_tc(i["mu"], i["lv"], i["eps"], *R.WEIGHTS[0])
    r32 = R.reparam_tc(i["mu"], i["lv"], i["eps"], *R.WEIGHTS[0], dtype=torch.float32)
    for k in ("z", "loss", "mi", "tc", "dwkl", "gmu_loss", "glv_loss"):
        assert R.rel_err(r32[k], r64[k]) <= 1e-5, (k, R.rel_err(r32[k], r64[k]))
