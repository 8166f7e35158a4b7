"""CPU: the references of tests/_gan_loss_refs.py held to torch's own forms, the fp32 restatement measured against fp64
(where the GPU's tolerances come from), the record of the defect the feature answers, and the host logic.

Table of (ii), worst |fp32 - fp64| / magnitude in units of 2^-24 over every shape, kind and label of the GPU tests, as
this test prints it (pytest -s) -- recorded in R.FP32_WORST with a little headroom:

    fused head     logit 1.35   p 1.14   dlogit 1.75   loss 1.13   gfeat 1.92   gw 3.76   gb 1.50
    logit vector   p 1.92   glogit 2.50   loss 2.90      (the planted logits 0, +-1 and neighbours, +-17, +-40, +-104 included)
"""
import pytest
import torch

import _gan_loss_refs as R
import _loss_refs as L

LOGITS = (0.0, 1.0, -1.0, 17.0, -17.0, 40.0, -40.0, 104.0, -104.0)


# (i) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(R.KINDS))
@pytest.mark.parametrize("label", R.LABELS)
def test_fp64_restatement_is_torchs_own(kind, label):
    """Value and gradient, logit by logit: binary_cross_entropy_with_logits, mse_loss / 2, relu, each under autograd."""
    s = torch.tensor(LOGITS + R.NEAR_ONE + tuple(-v for v in R.NEAR_ONE), dtype=torch.float64)
    t = R.f32(label)
    r = R.terms(s, t, kind)
    for i in range(s.numel()):
        si = s[i:i + 1].clone().requires_grad_()
        own = R.torch_loss(si, t, kind, 1.0)
        own.backward()
        own = own.detach()
        scale = max(float(r["l_mag"][i]), 1e-300)
        assert abs(float(r["l"][i]) - float(own)) <= 4 * 2.0 ** -53 * scale, (kind, label, float(s[i]), float(r["l"][i]), float(own))
        gscale = max(float(r["dl_mag"][i]), 1e-300)
        assert abs(float(r["dl"][i]) - float(si.grad)) <= 4 * 2.0 ** -53 * gscale, (kind, label, float(s[i]), float(r["dl"][i]), float(si.grad))
    assert torch.allclose(r["p"], torch.sigmoid(s), rtol=1e-15, atol=0)
    if kind in ("hinge_real", "hinge_fake"):        # the ties: no gradient, as relu'(0) = 0
        tie = 1.0 if kind == "hinge_real" else -1.0
        assert float(R.terms(torch.tensor([tie], dtype=torch.float64), t, kind)["dl"]) == 0.0


@pytest.mark.parametrize("kind", sorted(R.KINDS))
def test_nonfinite_classes_of_the_restatement(kind):
    """+-inf: the class torch's own form has, value and gradient.  NaN: a NaN loss and -- the rule this package states --
    a NaN gradient for every kind (autograd through relu or a negation gives a finite one)."""
    for label in R.LABELS:
        for v in (float("inf"), float("-inf")):
            s = torch.tensor([v], dtype=torch.float64)
            r = R.terms(s, R.f32(label), kind)
            si = s.clone().requires_grad_()
            own = R.torch_loss(si, R.f32(label), kind, 1.0)
            own.backward()
            for got, ref in ((r["l"], own.detach().reshape(1)), (r["dl"], si.grad)):
                assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isinf(got), torch.isinf(ref)), \
                    (kind, label, v, got, ref)
        r = R.terms(torch.tensor([float("nan")], dtype=torch.float64), R.f32(label), kind)
        assert bool(torch.isnan(r["l"]).all() and torch.isnan(r["dl"]).all() and torch.isnan(r["p"]).all()), (kind, label)


# (ii) -----------------------------------------------------------------------------------------------------------
def test_fp32_restatement_against_fp64():
    worst = {name: 0.0 for name in R.FP32_WORST}

    def take(name, got, ref, mag, keep=None):
        if keep is not None:
            got, ref, mag = got[keep], ref[keep], mag[keep]
        worst[name] = max(worst[name], R.worst_ratio(got, ref, mag))

    for shape in R.SHAPES:
        x = R.head_inputs(shape)
        for kind in sorted(R.KINDS):
            for label in (R.LABELS if kind in R.USES_LABEL else (0.9,)):
                for div in (None, 3 * shape[0]):
                    r64 = R.dot_gan_loss(x["feat"], x["w"], x["bias"], kind, label, div)
                    r32 = R.dot_gan_loss(x["feat"], x["w"], x["bias"], kind, label, div, dtype=torch.float32)
                    ok = ~r64["tie"]
                    take("logit", r32["logit"], r64["logit"], r64["logit_mag"])
                    take("p", r32["p"], r64["p"], r64["p_mag"])
                    take("loss", r32["loss"], r64["loss"], r64["loss_mag"])
                    take("dlogit", r32["dlogit"], r64["dlogit"], r64["dlogit_mag"], ok)
                    if bool(ok.all()):
                        for g in ("gfeat", "gw", "gb"):
                            take(g, r32[g], r64[g], r64[g + "_mag"])
                    # the logit vector route: the losses alone, on the fp32 logits
                    v64 = R.gan_loss(r32["logit"], kind, label, div, gscale=0.75)
                    v32 = R.gan_loss(r32["logit"], kind, label, div, gscale=0.75, dtype=torch.float32)
                    take("v_p", v32["p"], v64["p"], v64["p_mag"])
                    take("v_glogit", v32["glogit"], v64["glogit"], v64["glogit_mag"])
                    take("v_loss", v32["loss"], v64["loss"], v64["loss_mag"])
    # ... and on the planted logits, where the functions are at their extremes
    pl = R.planted_inputs()
    for kind in sorted(R.KINDS):
        for label in (R.LABELS if kind in R.USES_LABEL else (0.9,)):
            v64 = R.gan_loss(pl["logits"], kind, label)
            v32 = R.gan_loss(pl["logits"], kind, label, dtype=torch.float32)
            take("v_p", v32["p"], v64["p"], v64["p_mag"])
            take("v_glogit", v32["glogit"], v64["glogit"], v64["glogit_mag"])
            take("v_loss", v32["loss"], v64["loss"], v64["loss_mag"])
    print("worst fp32-vs-fp64 ratios, units of 2^-24:", {k: round(v, 2) for k, v in worst.items()})
    for name, v in worst.items():
        assert v <= R.FP32_WORST[name], (name, v, R.FP32_WORST[name])
        assert v >= 0.25 * R.FP32_WORST[name] or R.FP32_WORST[name] <= 1.0, \
            (name, v, "the recorded figure is far above what is measured: the GPU's tolerance would be loose")


# (iii) ----------------------------------------------------------------------------------------------------------
def test_record_of_the_defect():
    """The fused BCE head in fp32 (its restatement, operation for operation): dlogit is EXACTLY 0 at s = +40, whatever
    the label, and at most 1e-5 at s = -40 with label 0.9; the logistic loss keeps |sigmoid(s) - t| >= 0.09 at both."""
    one = torch.ones(1, 1)
    for s, t, bound in ((40.0, 0.1, 0.0), (40.0, 0.9, 0.0), (-40.0, 0.9, 1e-5)):
        feat = torch.tensor([[s]])
        old = L.dot_sigmoid_bce(feat, one, torch.zeros(1), t, dtype=torch.float32)["dlogit"]
        assert abs(float(old)) <= bound, (s, t, float(old))
        for dtype in (torch.float32, torch.float64):
            new = R.dot_gan_loss(feat, one, torch.zeros(1), "logistic", t, dtype=dtype, grads=False)["dlogit"]
            assert abs(float(new)) >= 0.09, (s, t, dtype, float(new))


# (iv) -----------------------------------------------------------------------------------------------------------
def test_loss_table_and_names():
    from disentangle_mlp_amd import functional as F
    from disentangle_mlp_amd import ops
    assert sorted(F.GAN_LOSSES) == sorted((n, r) for n in ("logistic", "hinge", "lsgan") for r in ("real", "fake", "gen"))
    assert {F.GAN_LOSSES[("logistic", r)] for r in F.GAN_ROLES} == {R.KINDS["logistic"]}
    assert {F.GAN_LOSSES[("lsgan", r)] for r in F.GAN_ROLES} == {R.KINDS["lsgan"]}
    assert [F.GAN_LOSSES[("hinge", r)] for r in ("real", "fake", "gen")] == \
        [R.KINDS["hinge_real"], R.KINDS["hinge_fake"], R.KINDS["hinge_gen"]]
    assert (ops.GAN_LOGISTIC, ops.GAN_LSGAN, ops.GAN_HINGE_REAL, ops.GAN_HINGE_FAKE, ops.GAN_HINGE_GEN) == \
        tuple(R.KINDS[k] for k in ("logistic", "lsgan", "hinge_real", "hinge_fake", "hinge_gen"))
    with pytest.raises(ValueError, match="logistic.*hinge.*lsgan"):
        F.gan_loss_kind("wasserstein", "real")
    with pytest.raises(ValueError, match="role"):
        F.gan_loss_kind("hinge", "critic")


def test_header_constants_match():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    got = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define\s+VG_GAN_(\w+)\s+(\d+)", text)}
    assert got == R.KINDS


def test_ops_refuse_cpu_tensors_and_bad_kinds():
    from disentangle_mlp_amd import _lib, build, ops
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.vg_dot_gan_loss_workspace_bytes(17) == 17 * 8 and lib.vg_dot_gan_loss_workspace_bytes(0) == 0
    # rejected arguments return VG_ERR_BAD_ARG before any launch
    assert lib.vg_dot_gan_loss_fwd(None, None, None, 0, 0.9, None, None, None, None, None, 4, 8, 4.0, None, 0, None) == -1
    assert lib.vg_gan_loss(None, 0, 0.9, None, None, None, None, 4, 4.0, 1.0, None) == -1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dot_gan_loss_fwd(torch.zeros(2, 4), torch.zeros(1, 4), torch.zeros(1), 0, 0.9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gan_loss(torch.zeros(4), 0, 0.9)


def test_trainer_keyword_host_logic():
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(TypeError, match="no discriminator"):
        T.VAETrainer(device="cpu", gan_loss="logistic")
    for cls in (T.BetaVAEGANTrainer, T.GANTrainer):
        with pytest.raises(ValueError, match="logistic.*hinge.*lsgan"):
            cls(device="cpu", gan_loss="wgan")
        plain = cls(device="cpu")
        assert plain._gan_loss is None
        key = plain._host_state_key()
        assert not any(isinstance(e, tuple) and e and e[0] == "gan_loss" for e in key), key
        keys = {key}
        for name in ("logistic", "hinge", "lsgan"):
            tr = cls(device="cpu", gan_loss=name)
            k = tr._host_state_key()
            assert k[:len(key)] == key and k[len(key):] == (("gan_loss", name),), (name, k)
            keys.add(k)
            assert sorted(tr.checkpoint(0)) == sorted(plain.checkpoint(0)), "no checkpoint key"
        assert len(keys) == 4
        # same seed, same initial weights: the keyword draws nothing
        for a, b in zip(plain.netD.state_dict().values(), cls(device="cpu", gan_loss="hinge").netD.state_dict().values()):
            assert torch.equal(a, b)
    # composes with the augmentation's key element, each in its place
    both = T.GANTrainer(device="cpu", diff_augment="color", gan_loss="hinge")._host_state_key()
    assert both[-1] == ("gan_loss", "hinge") and both[-2] == T.GANTrainer(device="cpu", diff_augment="color")._host_state_key()[-1]
