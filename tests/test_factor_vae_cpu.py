"""CPU: ``factor_vae`` (FactorVAE) -- the keyword is parsed and refused as documented, the critic is
one more part of the trainer that leaves every other weight, latent and checkpoint key alone, the restatements of
tests/_factor_refs.py are consistent with themselves, and the header, the binding and the library agree on the new entry
points.  No GPU."""
import ctypes
import math
import re

import pytest
import torch

import _factor_refs as R
from conftest import ROOT
from test_cabi_cpu import declared_symbols

NAN, INF = float("nan"), float("inf")
NEW = ("vg_permute_dims", "vg_factor_tc_workspace_bytes", "vg_factor_tc_fwd", "vg_factor_tc_bwd", "vg_factor_tc_fwd_dev",
       "vg_factor_tc_bwd_dev", "vg_factor_critic_loss")
SMALL = dict(width=64, depth=2)


# ---- the keyword ---------------------------------------------------------------------------------------------------------------
def test_parser_errors():
    from disentangle_mlp_amd import trainer as T
    for bad in ("much", (1.0,), (1.0, SMALL, 3), (1.0, 64), (1.0, [64, 2]), (1.0, dict(hidden=64)), [1.0],
                ("g", SMALL), (1.0, dict(width=64.0)), (1.0, dict(depth="2")), (1.0, dict(width=True)), (1.0, dict(lr="x")),
                (1.0, dict(betas=0.5)), (1.0, dict(betas=(0.5,))), (1.0, dict(betas=(0.5, 0.9, 0.99))), {}):
        with pytest.raises(TypeError, match="factor_vae"):
            T.VAETrainer(device="cpu", factor_vae=bad)
    for bad in (-1.0, NAN, INF, -INF, (NAN, SMALL), lambda it: -1.0, lambda it: NAN, (1.0, dict(width=0)), (1.0, dict(depth=0)),
                (1.0, dict(depth=-2)), (1.0, dict(lr=0.0)), (1.0, dict(lr=-1e-4)), (1.0, dict(lr=NAN)), (1.0, dict(lr=INF)),
                (1.0, dict(betas=(1.0, 0.9))), (1.0, dict(betas=(0.5, -0.1))), (1.0, dict(betas=(NAN, 0.9)))):
        with pytest.raises(ValueError, match="factor_vae"):
            T.VAETrainer(device="cpu", factor_vae=bad)


def test_keyword_values_and_views():
    from disentangle_mlp_amd import trainer as T
    plain = T.VAETrainer(device="cpu")
    keyed = T.VAETrainer(device="cpu", factor_vae=(6.4, SMALL))
    assert plain.factor_vae is None and plain.gamma is None and not hasattr(plain, "critic")
    assert keyed.gamma == 6.4 and keyed.factor_vae == (6.4, dict(width=64, depth=2, lr=1e-4, betas=(0.5, 0.9)))
    assert T.FACTOR_CRITIC_DEFAULTS == dict(width=1000, depth=6, lr=1e-4, betas=(0.5, 0.9))      # Kim & Mnih's
    assert keyed.kl_control is None and keyed.tc_decomposition is None and keyed.capacity is None
    with pytest.raises(AttributeError):
        keyed.factor_vae = 3.0
    with pytest.raises(TypeError, match="factor_vae"):
        plain.set_gamma(1.0)
    keyed.set_gamma(3)
    assert keyed.gamma == 3.0 and keyed.factor_vae[0] == 3.0
    for bad in (-1.0, NAN, INF):
        with pytest.raises(ValueError, match="gamma"):
            keyed.set_gamma(bad)
    zero = T.VAETrainer(device="cpu", factor_vae=0)
    assert zero.gamma == 0.0 and zero.critic.width == 1000 and zero.critic.depth == 6
    # a schedule: evaluated at iteration 0, then at the start of every step; beta stays the trainer's own word
    sched = T.BetaVAEGANTrainer(device="cpu", beta=4.0, factor_vae=(lambda it: 0.5 * it, SMALL))
    assert sched.gamma == 0.0 and sched.beta == 4.0 and not sched.device_hyper       # (a CPU trainer cannot carry the word)
    sched.iteration = 3
    sched._begin_step()
    assert sched.gamma == 1.5
    assert "iteration" in sched.checkpoint(0) and "iteration" not in keyed.checkpoint(0)
    # the optimizer of the critic: its own lr and betas, no scheduler, no weight decay; `set_lr` leaves it alone unless named
    t = T.VAETrainer(device="cpu", lr=3e-3, weight_decay=0.01, lr_scheduler=lambda o: torch.optim.lr_scheduler.StepLR(o, 1),
                     factor_vae=(1.0, dict(width=64, depth=2, lr=2e-4, betas=(0.4, 0.8))))
    g = t.optimizer_critic.param_groups[0]
    assert (g["lr"], g["betas"], g["weight_decay"]) == (2e-4, (0.4, 0.8), 0.0) and t.optimizer.param_groups[0]["weight_decay"] == 0.01
    assert list(t.lr_schedulers) == ["optimizer"]
    t.set_lr(1e-2)
    assert t.optimizer.param_groups[0]["lr"] == 1e-2 and g["lr"] == 2e-4
    t.set_lr(5e-4, which="optimizer_critic")
    assert t.optimizer.param_groups[0]["lr"] == 1e-2 and g["lr"] == 5e-4


def test_mutual_exclusion_with_the_other_objectives():
    from disentangle_mlp_amd import trainer as T
    others = dict(tc_decomposition=(1.0, 1.0), dip_vae=("i", 10.0, 100.0), mmd_vae=("imq", 100.0), kl_control=(2.0, 0.05))
    for cls in (T.VAETrainer, T.BetaVAEGANTrainer):
        for k, v in others.items():
            with pytest.raises(ValueError, match=f"each replace the KL term.*got factor_vae and {k}"):
                cls(device="cpu", factor_vae=(1.0, SMALL), dataset_size=100, **{k: v})


def test_gan_trainer_refuses_it():
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(TypeError, match="GANTrainer has no KL term: factor_vae does not apply"):
        T.GANTrainer(device="cpu", factor_vae=1.0)


# ---- the critic as one more part ---------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_existing_weights_and_the_global_stream_are_unchanged():
    from disentangle_mlp_amd import trainer as T
    plain, keyed = T.VAETrainer(device="cpu", seed=5), T.VAETrainer(device="cpu", seed=5, factor_vae=(1.0, SMALL))
    assert _same(plain.model.state_dict(), keyed.model.state_dict())
    plain, keyed = T.BetaVAEGANTrainer(device="cpu", seed=7), T.BetaVAEGANTrainer(device="cpu", seed=7, factor_vae=(1.0, SMALL))
    assert _same(plain.netEG.state_dict(), keyed.netEG.state_dict()) and _same(plain.netD.state_dict(), keyed.netD.state_dict())
    # what the global CPU generator gives next does not depend on the keyword either
    T.VAETrainer(device="cpu", seed=5)
    a = torch.rand(4)
    T.VAETrainer(device="cpu", seed=5, factor_vae=(1.0, SMALL))
    assert torch.equal(a, torch.rand(4))


def test_critic_initialisation_follows_the_seed_alone():
    from disentangle_mlp_amd import model as M, trainer as T
    a = T.VAETrainer(device="cpu", seed=5, factor_vae=(1.0, SMALL)).critic
    torch.manual_seed(1234)                                            # (the global stream plays no part)
    b = T.VAETrainer(device="cpu", seed=5, factor_vae=(2.0, SMALL)).critic
    c = T.VAETrainer(device="cpu", seed=6, factor_vae=(1.0, SMALL)).critic
    d = T.BetaVAEGANTrainer(device="cpu", seed=5, factor_vae=(1.0, SMALL)).critic
    assert _same(a.state_dict(), b.state_dict()) and _same(a.state_dict(), d.state_dict())
    assert not any(torch.equal(v, c.state_dict()[k]) for k, v in a.state_dict().items())
    assert isinstance(a, M.LatentCritic) and isinstance(a, torch.nn.Sequential)
    assert list(a.state_dict()) == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"]
    assert [tuple(v.shape) for v in a.state_dict().values()] == [(64, 128), (64,), (64, 64), (64,), (2, 64), (2,)]
    for m in a:
        if hasattr(m, "weight"):                                       # torch's Linear default: U(+-1/sqrt(fan_in))
            bound, w, b = m.in_features ** -0.5, m.weight.detach(), m.bias.detach()
            assert float(w.abs().max()) <= bound and float(b.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a(torch.zeros(4, 128))
    for bad in ((0, 64, 2), (128, 0, 2), (128, 64, 0)):
        with pytest.raises(ValueError, match="LatentCritic"):
            M.LatentCritic(*bad)


def test_parts_optimizers_and_capture_key():
    from disentangle_mlp_amd import trainer as T
    plain = T.BetaVAEGANTrainer(device="cpu")
    keyed = T.BetaVAEGANTrainer(device="cpu", factor_vae=(1.0, SMALL))
    assert [p.net for p in plain._parts] == ["netEG", "netD"] and T.BetaVAEGANTrainer._parts == plain._parts
    assert [p.net for p in keyed._parts] == ["netEG", "netD", "critic"]
    assert list(keyed._optimizers()) == ["optimizerEG", "optimizerD", "optimizer_critic"]
    assert [n for n, _, _ in keyed._guarded_optimizers()] == ["netEG", "netD", "critic"]
    assert keyed._checkpoint_optimizer_keys["optimizer_critic"] == "latent_critic_optimizer"
    assert keyed.flat_critic is None and keyed._flats() == []
    assert keyed._objective_key() == ("factor_vae", (64, 2, 1e-4, (0.5, 0.9)))
    # width, depth, the critic's lr and betas are frozen arguments of the key; gamma is not
    keys = {plain._host_state_key(), keyed._host_state_key()}
    for other in (dict(width=32, depth=2), dict(width=64, depth=3), dict(lr=2e-4, **SMALL), dict(betas=(0.5, 0.99), **SMALL)):
        keys.add(T.BetaVAEGANTrainer(device="cpu", factor_vae=(1.0, other))._host_state_key())
    assert len(keys) == 6
    assert T.BetaVAEGANTrainer(device="cpu", factor_vae=(7.0, SMALL))._host_state_key() == keyed._host_state_key()
    data = torch.zeros(8, 3, 64, 64)
    for o in keyed._optimizers().values():
        o.state_generation = 0                                         # (HipAdam's: torch.optim.Adam, a CPU trainer's, has none)
    k1 = keyed._capture_key(data, (0.9, 0.1, 8))
    keyed.set_gamma(2.0)
    assert keyed._capture_key(data, (0.9, 0.1, 8)) != k1              # a frozen value, as beta ...
    keyed.device_hyper = True
    k2 = keyed._capture_key(data, (0.9, 0.1, 8))
    keyed.set_gamma(3.0)
    assert keyed._capture_key(data, (0.9, 0.1, 8)) == k2              # ... unless it lives in a device word


def test_drawn_inputs_order_names_and_streams():
    from disentangle_mlp_amd import trainer as T
    plain, keyed = T.VAETrainer(device="cpu", seed=5), T.VAETrainer(device="cpu", seed=5, factor_vae=(1.0, SMALL))
    assert [tuple(d) for d in keyed._drawn()] == [("eps", "normal", "latent_generator"), ("permute", "uniform", "permute_generator")]
    assert [d.name for d in plain._drawn()] == ["eps"] and not hasattr(plain, "permute_generator")
    full = T.BetaVAEGANTrainer(device="cpu", seed=5, factor_vae=(1.0, SMALL), diff_augment="color")
    assert [(d.name, d.dist) for d in full._drawn()] == [("noise", "normal"), ("eps2", "normal"), ("eps3", "normal"),
                                                         ("augment", "uniform"), ("permute", "uniform")]
    mmd = T.VAETrainer(device="cpu", seed=5, mmd_vae=("imq", 1.0))
    assert [d.name for d in mmd._drawn()] == ["eps", "prior"]         # (another objective's input is untouched)
    # the latents are bit for bit what they are without the keyword; the uniforms differ from rank to rank
    a, b = plain._draw((None,), 4), keyed._draw((None, None), 4)
    assert len(b) == 2 and torch.equal(a[0], b[0]) and b[1].shape == (4, 128)
    assert float(b[1].min()) >= 0.0 and float(b[1].max()) < 1.0
    assert torch.equal(plain._draw((None,), 4)[0], keyed._draw((None, None), 4)[0])
    seeds = {T._permute_generator("cpu", 5, r).initial_seed() for r in (0, 1)}
    seeds |= {T._latent_generator("cpu", 5, r).initial_seed() for r in (0, 1)}
    seeds |= {T._augment_generator("cpu", 5, r).initial_seed() for r in (0, 1)}
    assert len(seeds) == 6
    u = keyed.draw_permute(5)
    assert u.shape == (5, 128) and u.dtype == torch.float32
    with pytest.raises(TypeError, match="factor_vae"):
        plain.draw_permute(5)
    with pytest.raises(TypeError, match="permute= belongs to factor_vae, which is off"):
        plain.step(torch.zeros(2, 3, 64, 64), permute=u)
    for bad in (torch.zeros(4, 128), torch.zeros(5, 127), torch.zeros(5, 128, dtype=torch.float64)):
        with pytest.raises(ValueError, match="permute must be a float32 tensor of shape"):
            keyed._with_permute((None,), bad, 5)
    assert keyed._with_permute((None,), u, 5)[1] is u


def test_checkpoint_keys_and_loading_without_them():
    from disentangle_mlp_amd import trainer as T
    plain = T.BetaVAEGANTrainer(device="cpu", seed=5)
    keyed = T.BetaVAEGANTrainer(device="cpu", seed=5, factor_vae=(1.0, SMALL))
    assert set(keyed.checkpoint(0)) == set(plain.checkpoint(0)) | {"latent_critic", "latent_critic_optimizer"}
    assert list(keyed.checkpoint(0)["latent_critic"]) == list(keyed.critic.state_dict())
    v = T.VAETrainer(device="cpu", factor_vae=(1.0, SMALL))
    assert set(v.checkpoint(0)) == set(T.VAETrainer(device="cpu").checkpoint(0)) | {"latent_critic", "latent_critic_optimizer"}
    # a checkpoint written without the keyword loads and leaves a fresh critic, as a missing EMA key does
    fresh = {k: t.clone() for k, t in keyed.critic.state_dict().items()}
    assert keyed.load(plain.checkpoint(3)) == 3 and _same(fresh, keyed.critic.state_dict())
    # ... and one written with it restores the critic
    other = T.BetaVAEGANTrainer(device="cpu", seed=6, factor_vae=(1.0, SMALL))
    assert not _same(other.critic.state_dict(), fresh)
    other.load(keyed.checkpoint(4))
    assert _same(other.critic.state_dict(), fresh) and _same(other.netEG.state_dict(), keyed.netEG.state_dict())
    plain.load(keyed.checkpoint(5))                                    # the other way round: the extra keys are ignored


# ---- the restatements against themselves -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (17, 5), (64, 9)], ids=str)
def test_restated_permutation_is_a_permutation_per_column(shape):
    g = torch.Generator().manual_seed(shape[0])
    z, u = torch.randn(*shape, generator=g), torch.rand(*shape, generator=g)
    r = R.ranks(u)
    for d in range(shape[1]):
        assert sorted(r[:, d].tolist()) == list(range(shape[0]))
    zp = R.permute_dims(z, u)
    assert torch.equal(zp.sort(0).values, z.sort(0).values)
    assert torch.equal(zp, z.gather(0, torch.argsort(u, dim=0, stable=True)))


def test_restated_permutation_breaks_ties_by_row_index():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(33, 4, generator=g)
    assert torch.equal(R.permute_dims(z, torch.full((33, 4), 0.25)), z)             # constant: the identity
    u = torch.floor(torch.rand(33, 4, generator=g) * 4) / 4                         # four values: mostly ties
    r = R.ranks(u)
    for d in range(4):
        for v in u[:, d].unique():
            rows = (u[:, d] == v).nonzero().flatten()
            assert r[rows, d].tolist() == sorted(r[rows, d].tolist())               # equal uniforms keep their order
    assert torch.equal(R.permute_dims(z, u), z.gather(0, torch.argsort(u, dim=0, stable=True)))


@pytest.mark.parametrize("rows", [2, 18, 130])
def test_restated_cross_entropy_is_the_softplus_form(rows):
    logits = torch.cat([R.make_logits(rows // 2, 0), R.make_logits(rows // 2, 1)])
    for div in (None, 2.0 * rows):
        ref = R.critic_loss(logits, div)
        loss, glogits = R.cross_entropy_form(logits, div)
        assert R.rel_err(ref["loss"], loss) <= 1e-14 and R.rel_err(ref["glogits"], glogits) <= 1e-14
        assert math.isfinite(float(ref["loss"])) and bool(torch.isfinite(ref["glogits"]).all())
    ref = R.critic_loss(logits)
    assert torch.equal(ref["glogits"][:, 0], -ref["glogits"][:, 1])
    if rows >= 18:                                                     # the saturated rows: exactly 0 and exactly 1 / divisor
        assert ref["glogits"][7, 0] == 0.0 and ref["glogits"][8, 0] == -1.0 / rows and ref["glogits"][6, 1] == 1.0 / rows
    # the tie of row 0 (GAPS[0] == 0) is wrong whichever half it sits in
    own_gap = torch.where(torch.arange(rows) < rows // 2, logits[:, 0] - logits[:, 1], logits[:, 1] - logits[:, 0])
    assert float(own_gap[0]) == 0.0 and ref["acc"] == float((own_gap > 0).sum()) / rows


def test_restated_factor_tc_gradient_is_constant():
    logits = R.make_logits(65)
    ref = R.factor_tc(logits, 123.5, R.BETA, R.GAMMA)
    assert torch.equal(ref["glogits"][:, 0], torch.full((65,), R.GAMMA * R.GLOSS, dtype=torch.float64))
    assert torch.equal(ref["glogits"][:, 1], -ref["glogits"][:, 0]) and float(ref["gkl"]) == R.BETA * R.GLOSS
    assert float(ref["loss"]) == R.BETA * 123.5 + R.GAMMA * float(ref["tc"])


# ---- functional: no CPU path -------------------------------------------------------------------------------------------------------
def test_ops_and_functional_refuse_cpu_tensors():
    from disentangle_mlp_amd import functional as F, ops
    z, logits, kl = torch.zeros(4, 8), torch.zeros(4, 2), torch.zeros(())
    for call in (lambda: ops.permute_dims(z, z), lambda: F.permute_dims(z, z), lambda: ops.factor_tc_fwd(logits, kl, 1.0, 1.0),
                 lambda: ops.factor_tc_bwd(logits, kl, 1.0, 1.0), lambda: F.factor_tc(logits, kl, 1.0, 1.0),
                 lambda: ops.factor_critic_loss(logits), lambda: F.factor_critic_loss(logits)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_symbols():
    from disentangle_mlp_amd import _lib, build, ops
    declared = declared_symbols()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES
    raw = ctypes.CDLL(build.build(verbose=False))
    for name in NEW:
        assert getattr(raw, name) is not None
    assert _lib.load().vg_version() == _lib.ABI_VERSION == 7          # only added: the version stays
    header = open(f"{ROOT}/include/vaegan_hip.h").read()
    assert int(re.search(r"#define\s+VG_PERMUTE_MAX_BATCH\s+(\d+)", header).group(1)) == ops.PERMUTE_MAX_BATCH >= 1024


def test_host_side_validation():
    from disentangle_mlp_amd import _lib, ops
    lib = _lib.load()
    a = 4096                                                          # made-up addresses: every call below is refused on the host
    top = ops.PERMUTE_MAX_BATCH
    assert lib.vg_permute_dims(None, a, 2 * a, 8, 8, None) == -1 and lib.vg_permute_dims(a, None, 2 * a, 8, 8, None) == -1
    assert lib.vg_permute_dims(a, 2 * a, None, 8, 8, None) == -1
    assert lib.vg_permute_dims(a, 2 * a, a, 8, 8, None) == -1 and lib.vg_permute_dims(a, 2 * a, 2 * a, 8, 8, None) == -1   # in place
    for B, D in ((0, 8), (8, 0), (-1, 8), (top + 1, 8)):
        assert lib.vg_permute_dims(a, 2 * a, 3 * a, B, D, None) == -1, (B, D)
    assert lib.vg_factor_tc_workspace_bytes(128, 2) == 0
    assert lib.vg_factor_tc_fwd(None, a, a, 8, 1.0, 1.0, None, 0, None) == -1
    assert lib.vg_factor_tc_fwd(a, None, a, 8, 1.0, 1.0, None, 0, None) == -1
    assert lib.vg_factor_tc_fwd(a, a, None, 8, 1.0, 1.0, None, 0, None) == -1
    assert lib.vg_factor_tc_fwd(a, a, a, 0, 1.0, 1.0, None, 0, None) == -1
    assert lib.vg_factor_tc_fwd_dev(a, a, a, 8, None, a, None, 0, None) == -1
    assert lib.vg_factor_tc_fwd_dev(a, a, a, 8, a, None, None, 0, None) == -1
    assert lib.vg_factor_tc_bwd(None, 1.0, 1.0, a, a, 8, None, 0, None) == -1
    assert lib.vg_factor_tc_bwd(a, 1.0, 1.0, None, a, 8, None, 0, None) == -1
    assert lib.vg_factor_tc_bwd(a, 1.0, 1.0, a, None, 8, None, 0, None) == -1
    assert lib.vg_factor_tc_bwd(a, 1.0, 1.0, a, a, 0, None, 0, None) == -1
    assert lib.vg_factor_tc_bwd_dev(a, None, a, a, a, 8, None, 0, None) == -1
    assert lib.vg_factor_tc_bwd_dev(a, a, None, a, a, 8, None, 0, None) == -1
    assert lib.vg_factor_critic_loss(None, a, a, a, 8, 16.0, None) == -1
    assert lib.vg_factor_critic_loss(a, None, a, a, 8, 16.0, None) == -1
    assert lib.vg_factor_critic_loss(a, 2 * a, a, 3 * a, 8, 16.0, None) == -1          # in place
    assert lib.vg_factor_critic_loss(a, 2 * a, 3 * a, 4 * a, 0, 16.0, None) == -1
    for div in (0.0, -1.0, NAN, INF):
        assert lib.vg_factor_critic_loss(a, 2 * a, 3 * a, 4 * a, 8, div, None) == -1, div
