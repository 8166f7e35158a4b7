"""CPU: the C ABI of the InfoVAE / WAE-MMD kernels (vg_reparam_mmd_*: declared, bound, exported, arguments validated
before any launch), `ops.reparam_mmd_fwd` / `functional.reparam_mmd` without a CPU path, the trainers' argument checks,
and the torch restatement the GPU tests compare against (tests/_mmd_refs.py) checked against itself: the closed-form
gradient the kernels implement against autograd, and the fp32 evaluation's `mmd` against the fp64 one over the sum of its
terms -- the condition behind the bound of the GPU tests."""
import ctypes

import pytest
import torch

import _mmd_refs as R
from test_cabi_cpu import declared_symbols

NEW = ["vg_reparam_mmd_bwd", "vg_reparam_mmd_bwd_dev", "vg_reparam_mmd_fwd", "vg_reparam_mmd_fwd_dev",
       "vg_reparam_mmd_workspace_bytes"]


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
    assert lib.vg_reparam_mmd_workspace_bytes(128, 128) > 0 and lib.vg_reparam_mmd_workspace_bytes(1024, 1024) > 0
    for shape in ((1, 128), (0, 128), (128, 1025)):               # the U-statistic has no value at B = 1
        assert lib.vg_reparam_mmd_workspace_bytes(*shape) == 0, shape


_HS = (ctypes.c_float * 8)(1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0)


def _fwd_args(B=4, D=8, **over):
    """Host addresses standing in for device pointers: every call below must return before a launch."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    a = dict(mu=p, lv=p, eps=p, zp=p, z=p, out4=p, w=p, B=B, D=D, kind=2, beta=6.0, lambda_mmd=1000.0,
             hs=ctypes.addressof(_HS), n=7, ws=p, ws_bytes=1 << 30, stream=None)
    a.update(over)
    return buf, a


def _bwd_args(B=4, D=8, **over):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    a = dict(gz=p, mu=p, lv=p, eps=p, z=p, zp=p, w=p, gloss=p, beta=6.0, lambda_mmd=1000.0, gmu=p, glv=p, B=B, D=D, ws=p,
             ws_bytes=1 << 30, stream=None)
    a.update(over)
    return buf, a


_ids = dict(ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
_BAD_HS = {"zero": (1.0, 0.0), "negative": (-2.0,), "inf": (1.0, float("inf")), "nan": (float("nan"),)}


@pytest.mark.parametrize("over", [dict(mu=None), dict(lv=None), dict(eps=None), dict(zp=None), dict(z=None), dict(out4=None),
                                  dict(w=None), dict(hs=None), dict(ws=None), dict(B=1), dict(B=0), dict(B=1025),
                                  dict(D=0), dict(D=1025), dict(kind=0), dict(kind=3), dict(n=0), dict(n=9),
                                  dict(bad_hs="zero"), dict(bad_hs="negative"), dict(bad_hs="inf"), dict(bad_hs="nan"),
                                  dict(lambda_mmd=-1.0), dict(lambda_mmd=float("inf")), dict(lambda_mmd=float("nan")),
                                  dict(short_ws=1), dict(beta=None)], **_ids)
def test_forward_rejects_bad_arguments_before_any_launch(lib, over):
    over = dict(over)
    dev = "beta" in over                                          # NULL beta_dev: the _dev entry only
    held = None
    if "bad_hs" in over:
        values = _BAD_HS[over.pop("bad_hs")]
        held = (ctypes.c_float * len(values))(*values)
        over.update(hs=ctypes.addressof(held), n=len(values))
    if "short_ws" in over:
        over.pop("short_ws")
        over["ws_bytes"] = lib.vg_reparam_mmd_workspace_bytes(4, 8) - 1
    keep, a = _fwd_args(**over)
    if not dev:
        assert lib.vg_reparam_mmd_fwd(*a.values()) == -1
        a["beta"] = ctypes.addressof(keep)                        # a beta word: the same refusal from the _dev twin
    assert lib.vg_reparam_mmd_fwd_dev(*a.values()) == -1


@pytest.mark.parametrize("over", [dict(mu=None), dict(lv=None), dict(eps=None), dict(z=None), dict(zp=None), dict(w=None),
                                  dict(gmu=None), dict(glv=None), dict(ws=None), dict(B=1), dict(B=0), dict(B=1025),
                                  dict(D=0), dict(D=1025), dict(lambda_mmd=-1.0), dict(lambda_mmd=float("inf")),
                                  dict(lambda_mmd=float("nan")), dict(short_ws=1), dict(beta=None)], **_ids)
def test_backward_rejects_bad_arguments_before_any_launch(lib, over):
    over = dict(over)
    dev = "beta" in over
    if "short_ws" in over:
        over.pop("short_ws")
        over["ws_bytes"] = lib.vg_reparam_mmd_workspace_bytes(4, 8) - 1
    keep, a = _bwd_args(**over)
    if not dev:
        assert lib.vg_reparam_mmd_bwd(*a.values()) == -1
        a["beta"] = ctypes.addressof(keep)
    assert lib.vg_reparam_mmd_bwd_dev(*a.values()) == -1


def test_ops_and_functional_refuse_cpu_tensors(lib):
    from disentangle_mlp_amd import functional as F, ops
    t = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reparam_mmd_fwd(t, t, t, t, 6.0, 1000.0, "imq", None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reparam_mmd_bwd(None, t, t, t, t, t, torch.zeros(2, 4, 4), None, 6.0, 1000.0, "rbf", None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.reparam_mmd(t, t, t, t, 6.0, 1000.0)
    with pytest.raises(ValueError, match="kernel"):
        F.reparam_mmd(t, t, t, t, 6.0, 1000.0, kernel="laplace")
    with pytest.raises(ValueError, match="bandwidths"):
        F.reparam_mmd(t, t, t, t, 6.0, 1000.0, bandwidths=(1.0, -1.0))
    assert ops.mmd_bandwidths("rbf", 128) == (256.0,)             # WAE's convention with sigma_p^2 = 1
    assert ops.mmd_bandwidths("imq", 128) == R.default_bandwidths("imq", 128) and len(ops.mmd_bandwidths("imq", 128)) == 7
    assert ops.mmd_bandwidths("rbf", 128, [128.0 * 128.0]) == (16384.0,)      # Zhao's own choice, passed by the caller


def test_trainer_arguments():
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(TypeError, match="GANTrainer has no KL term: mmd_vae does not apply"):
        T.GANTrainer(device="cpu", mmd_vae=("imq", 1000.0))
    with pytest.raises(TypeError, match="mmd_vae must be"):
        T.VAETrainer(device="cpu", mmd_vae=10.0)
    with pytest.raises(TypeError, match="mmd_vae must be"):
        T.VAETrainer(device="cpu", mmd_vae=("imq", 1.0, (1.0,), 2.0))
    for bad in (("laplace", 1.0), (1, 1.0), ("imq", -1.0), ("rbf", float("inf")), ("rbf", float("nan")), ("imq", 1.0, ()),
                ("imq", 1.0, tuple(range(1, 10))), ("rbf", 1.0, (1.0, 0.0)), ("rbf", 1.0, (-2.0,)),
                ("rbf", 1.0, (float("inf"),)), ("imq", 1.0, (float("nan"),))):
        with pytest.raises(ValueError, match="mmd_vae"):
            T.VAETrainer(device="cpu", mmd_vae=bad)
    for cls in (T.VAETrainer, T.BetaVAEGANTrainer):
        # one rule for every clash: the table's keywords, then the two that met
        with pytest.raises(ValueError, match=r"mmd_vae, dip_vae and tc_decomposition.*\(got mmd_vae and tc_decomposition\)"):
            cls(device="cpu", mmd_vae=("imq", 1000.0), tc_decomposition=(1.0, 1.0), dataset_size=100)
        with pytest.raises(ValueError, match=r"mmd_vae, dip_vae and tc_decomposition.*\(got mmd_vae and dip_vae\)"):
            cls(device="cpu", mmd_vae=("imq", 1000.0), dip_vae=("i", 10.0, 100.0))
        with pytest.raises(ValueError, match=r"mmd_vae, dip_vae and tc_decomposition.*\(got dip_vae and tc_decomposition\)"):
            cls(device="cpu", dip_vae=("i", 10.0, 100.0), tc_decomposition=(1.0, 1.0), dataset_size=100)
        with pytest.raises(ValueError, match=r"\(got dip_vae and tc_decomposition\)"):      # all three: the first clash in table order
            cls(device="cpu", mmd_vae=("imq", 1000.0), dip_vae=("i", 10.0, 100.0), tc_decomposition=(1.0, 1.0), dataset_size=100)
        with pytest.raises(TypeError, match="pair"):      # a malformed earlier keyword is reported before the clash
            cls(device="cpu", mmd_vae=("imq", 1000.0), tc_decomposition=1.0)
    plain, keyed = T.VAETrainer(device="cpu"), T.VAETrainer(device="cpu", mmd_vae=("imq", 1000))
    assert plain.mmd_vae is None and keyed.mmd_vae == ("imq", 1000.0, None)
    assert plain._latents == ("eps",) and keyed._latents == ("eps", "prior")      # one more draw, last
    assert T.VAETrainer._latents == ("eps",)
    keys = {plain._host_state_key(), keyed._host_state_key()}
    for other in (("rbf", 1000), ("imq", 999), ("imq", 1000, (1.0, 2.0)), ("imq", 1000, [1.0, 3.0])):
        keys.add(T.VAETrainer(device="cpu", mmd_vae=other)._host_state_key())      # frozen kernel arguments, all of them
    assert len(keys) == 6
    assert set(plain.checkpoint(0)) == set(keyed.checkpoint(0))   # the option adds no checkpoint state
    gan = T.BetaVAEGANTrainer(device="cpu", beta=0.0, mmd_vae=("rbf", 10, [4.0]))      # beta = 0: a WAE
    assert gan.mmd_vae == ("rbf", 10.0, (4.0,)) and gan._latents == ("noise", "eps2", "eps3", "prior")
    with pytest.raises(TypeError, match="prior= belongs to mmd_vae"):
        plain.step(torch.zeros(2, 3, 64, 64), prior=torch.zeros(2, 128))


# ---- the restatement against itself -----------------------------------------------------------------------------------
def _extra_cases(D):
    return R.CASES + [("rbf", (float(D * D),), R.LAMBDA, 6.0)]     # Zhao's own bandwidth as well


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_closed_form_gradient_is_autograd_s(shape):
    i = R.make_inputs(*shape)
    for kernel, hs, lam, beta in _extra_cases(shape[1]):
        ref = R.reparam_mmd(i["mu"], i["lv"], i["eps"], i["zp"], beta, kernel, lam, hs)
        gmu, glv = R.closed_form_grads(i["mu"], i["lv"], i["eps"], i["zp"], beta, kernel, lam, hs)
        e = R.rel_err(gmu, ref["gmu_loss"]), R.rel_err(glv, ref["glv_loss"])
        print(f"{shape} {kernel} {hs} beta {beta}: closed form against autograd {e[0]:.3e} {e[1]:.3e}")
        assert max(e) <= 1e-12, (kernel, hs, beta, e)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_fp32_restatement_is_a_usable_yardstick(shape):
    """The bound of `mmd` in the GPU tests is max(1e-6, 5 x the fp32 restatement's error) OVER THE SUM OF ITS TERMS: the
    restatement itself has to meet the floor with room, |error| / (|kzz| + |kpp| + 2 |kzp|) <= 1e-6 / 5.  Largest seen
    over these shapes and cases: 8.9e-8.  (Relative to mmd itself the same error reaches 7.7e-6 here and grows without
    limit as mmd goes to 0 against its terms: a bound over the value would test the yardstick, not the kernel.)"""
    i = R.make_inputs(*shape)
    for kernel, hs, lam, beta in R.CASES:
        r64 = R.reparam_mmd(i["mu"], i["lv"], i["eps"], i["zp"], beta, kernel, lam, hs)
        r32 = R.reparam_mmd(i["mu"], i["lv"], i["eps"], i["zp"], beta, kernel, lam, hs, dtype=torch.float32)
        e = R.scalar_err(r32["mmd"], r64["mmd"], r64["mmd_terms"])
        own = R.scalar_err(r32["mmd"], r64["mmd"], r64["mmd"].abs())
        print(f"{shape} {kernel} beta {beta}: fp32 mmd error over its terms {e:.3e}, over its value {own:.3e}")
        assert e <= 1e-6 / 5, (kernel, beta, e)
