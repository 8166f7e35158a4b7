"""GPU: the fused InfoVAE / WAE-MMD kernels (csrc/reparam_mmd.hip) against the fp64 restatement of tests/_mmd_refs.py, and
through `functional.ReparamMMDFn`, `VAE.forward_with_mmd` and the trainers' ``mmd_vae``.

Bound of every parity check, per tensor: max error over the reference's largest magnitude <= max(1e-6, 5 x the same
figure of the restatement evaluated in fp32) -- the project's convention (conftest.check_state, SURVEY KAT-0).  For the
scalars `mmd` and `loss`, differences of O(1) terms, the error is taken over the SUM OF THE MAGNITUDES of the terms
(|kzz| + |kpp| + 2 |kzp|; |beta kl| + B lambda that) instead: tests/test_reparam_mmd_cpu.py asserts that the restatement
alone meets the 1e-6 floor of that bound with a factor of five to spare.  Each check prints its figures before it asserts
(``pytest -s``).

Shapes: the smallest legal batch, partial wavefronts, D off every multiple of 64 and B off every multiple of the 32-wide
pair tile and of the 16-row backward block, one tile and several (mirrored ones included), more than one 64-column chunk,
B above and below D -- and once each (1024, 32) and (32, 1024): every tile slot, every chunk."""
import math

import pytest
import torch

import _mmd_refs as R
from conftest import BN_SHADOWED, GRADNORM_TOL, LOSS_TOL, gap

pytestmark = pytest.mark.gpu

GLOSS = 0.75
MODES = ("gz+gloss", "gloss", "gz")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


_cache = {}


def _refs(key, inputs, case):
    """(fp64, fp32) restatement of one case: computed once, shared, never modified."""
    k = (key, case)
    if k not in _cache:
        kernel, hs, lam, beta = case
        _cache[k] = tuple(R.reparam_mmd(inputs["mu"], inputs["lv"], inputs["eps"], inputs["zp"], beta, kernel, lam, hs, dtype=dt)
                          for dt in (torch.float64, torch.float32))
    return _cache[k]


def _forward(H, i, case, beta=None):
    kernel, hs, lam, case_beta = case
    mu, lv, eps, zp = (i[k].cuda() for k in ("mu", "lv", "eps", "zp"))
    z, out4, w = H.reparam_mmd_fwd(mu, lv, eps, zp, case_beta if beta is None else beta, lam, kernel, hs)
    return dict(mu=mu, lv=lv, eps=eps, zp=zp, z=z, out4=out4, w=w)


def _backward(H, f, case, gz, gloss, beta=None):
    kernel, hs, lam, case_beta = case
    return H.reparam_mmd_bwd(gz, f["mu"], f["lv"], f["eps"], f["z"], f["zp"], f["w"], gloss,
                             case_beta if beta is None else beta, lam, kernel, hs)


def _check(what, got, r32, r64):
    e, b = R.rel_err(got, r64), R.bound(r32, r64)
    print(f"{what}: error {e:.3e}  bound {b:.3e}  (fp32 restatement {R.rel_err(r32, r64):.3e})")
    assert torch.isfinite(torch.as_tensor(got)).all(), what
    assert e <= b, (what, e, b)


def _check_scalar(what, name, got, r32, r64):
    """`mmd` / `loss`: the error over the sum of the magnitudes of the terms."""
    e, b = R.scalar_err(got, r64[name], r64[name + "_terms"]), R.scalar_bound(r32, r64, name)
    print(f"{what} {name}: {float(got):.8g} (fp64 {float(r64[name]):.8g}) error over its terms {e:.3e}  bound {b:.3e}  "
          f"(fp32 restatement {R.scalar_err(r32[name], r64[name], r64[name + '_terms']):.3e})")
    assert math.isfinite(float(got)), (what, name)
    assert e <= b, (what, name, e, b)


def _check_forward(what, f, r64, r32):
    _check(f"{what} z", f["z"], r32["z"], r64["z"])
    out4 = f["out4"].cpu()
    _check_scalar(what, "loss", out4[0], r32, r64)
    _check(f"{what} kl", out4[1], r32["kl"], r64["kl"])
    _check_scalar(what, "mmd", out4[2], r32, r64)
    _check(f"{what} kzz", out4[3], r32["kzz"], r64["kzz"])
    assert torch.equal(_bits(f["w"][0]), _bits(f["w"][0].t()))    # the zz slopes are symmetric to the bit ...
    assert float(f["w"][0].diagonal().abs().max()) == 0.0         # ... with a zero diagonal


def _check_backward(H, what, f, i, case, r64, r32, modes=MODES):
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    for mode in modes:
        a = gz if "gz" in mode else None
        b = gloss if "gloss" in mode else None
        gmu, glv = _backward(H, f, case, a, b)
        want = [R.expected_grads(r, i["lv"], i["eps"], i["gz"] if a is not None else None, GLOSS if b is not None else None,
                                 dtype=dt) for r, dt in ((r64, torch.float64), (r32, torch.float32))]
        _check(f"{what} gmu [{mode}]", gmu, want[1][0], want[0][0])
        _check(f"{what} glv [{mode}]", glv, want[1][1], want[0][1])


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


def _kl_z(H, f):
    return H.reparam_kl_fwd(f["mu"], f["lv"], f["eps"], 6.0)[0]


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", R.CASES, ids=str)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_parity_with_the_fp64_restatement(H, shape, case):
    i = R.make_inputs(*shape)
    r64, r32 = _refs(shape, i, case)
    f = _forward(H, i, case)
    what = f"{shape} {case}"
    _check_forward(what, f, r64, r32)
    assert torch.equal(_bits(f["z"]), _bits(_kl_z(H, f)))         # z: the bits of reparam_kl_fwd
    _check_backward(H, what, f, i, case, r64, r32)


@pytest.mark.parametrize("shape", R.EDGE_SHAPES, ids=str)
def test_parity_at_the_edges_of_the_contract(H, shape):
    """(1024, 32): all 2080 tile slots, 64 row blocks and 16 chunks of j in the backward; (32, 1024): 16 chunks of
    columns, every KL slot.  The fp64 restatement's [B, B, D] stays at 0.27 GB."""
    case = R.CASES[1]
    i = R.make_inputs(*shape)
    r64, r32 = _refs(shape, i, case)
    f = _forward(H, i, case)
    _check_forward(f"{shape} {case}", f, r64, r32)
    _check_backward(H, f"{shape} {case}", f, i, case, r64, r32, modes=("gz+gloss",))
    _cache.clear()                                                # (the largest references: not kept)


# ------------------------------------------------------------------ 2. identical rows: every distance is exactly 0
@pytest.mark.parametrize("case", R.CASES[:2], ids=str)
def test_identical_rows(H, case):
    i = {k: v[:1].repeat(8, 1).contiguous() for k, v in R.make_inputs(8, 16).items()}
    r64, r32 = _refs("same-rows", i, case)
    f = _forward(H, i, case)
    _check_forward("same rows", f, r64, r32)
    n = len(R.default_bandwidths(case[0], 16))
    assert float(f["out4"][3]) == float(n)                        # d = 0 from the differences: k = 1 per bandwidth, exactly
    _check_backward(H, "same rows", f, i, case, r64, r32)
    gmu, glv = _backward(H, f, case, None, torch.full((), GLOSS, device="cuda"))
    assert torch.isfinite(gmu).all() and torch.isfinite(glv).all()


# ------------------------------------------------------------------ 3. a posterior far from the prior
def test_a_posterior_far_from_the_prior_stays_finite(H):
    """mu + 30 at (64, 128), rbf with h = 2 D: d(z, zp) is about 900 D, exp(-450) underflows to 0 in fp32.  kzp = 0, its
    slopes are 0 and nothing turns into 0 * inf."""
    case = R.CASES[0]
    i = dict(R.make_inputs(64, 128))
    i["mu"] = i["mu"] + 30.0
    r64, r32 = _refs("far", i, case)
    f = _forward(H, i, case)
    assert float(f["w"][1].abs().max()) == 0.0                    # the zp kernel underflowed as a whole
    assert torch.isfinite(f["out4"]).all() and torch.isfinite(f["w"]).all()
    _check_forward("far", f, r64, r32)
    _check_backward(H, "far", f, i, case, r64, r32)


# ------------------------------------------------------------------ 4. lambda 0: the plain KL
@pytest.mark.parametrize("kernel", ["rbf", "imq"])
@pytest.mark.parametrize("shape", [(17, 65), (128, 128)], ids=str)
def test_zero_lambda_gives_the_plain_kl(H, shape, kernel):
    i = R.make_inputs(*shape)
    beta = 6.0
    case = (kernel, None, 0.0, beta)
    r64, r32 = _refs(shape, i, case)
    f = _forward(H, i, case)
    z, kl, _ = H.reparam_kl_fwd(f["mu"], f["lv"], f["eps"], beta)
    assert torch.equal(_bits(f["z"]), _bits(z))
    _check_scalar(f"{shape}", "loss", f["out4"][0].cpu(), r32, r64)
    e = R.rel_err(f["out4"][0].cpu(), kl.cpu().double().reshape(()))
    print(f"{shape} {kernel} loss against reparam_kl_fwd: {e:.3e}")
    assert e <= R.bound(r32["loss"], r64["loss"])
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    gmu, glv = _backward(H, f, case, gz, gloss)
    kmu, klv = H.reparam_kl_bwd(gz, f["mu"], f["lv"], f["eps"], gloss, beta)
    want = [R.expected_grads(r, i["lv"], i["eps"], i["gz"], GLOSS, dtype=dt) for r, dt in ((r64, torch.float64), (r32, torch.float32))]
    for name, got, ref, n in (("gmu", gmu, kmu, 0), ("glv", glv, klv, 1)):
        _check(f"{shape} {name}", got, want[1][n], want[0][n])
        e, b = R.rel_err(got, ref), R.bound(want[1][n], want[0][n])
        print(f"{shape} {kernel} {name} against reparam_kl_bwd: {e:.3e}  bound {b:.3e}")
        assert e <= b


# ------------------------------------------------------------------ 5. beta as a float / as a device word; run to run
@pytest.mark.parametrize("shape", [(5, 7), (128, 128), (130, 200)], ids=str)
def test_beta_word_and_repeated_runs_give_the_same_bits(H, shape):
    i = R.make_inputs(*shape)
    case = R.CASES[1]
    word = torch.full((1,), case[3], dtype=torch.float32, device="cuda")
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    runs = []
    for beta in (case[3], word, case[3]):
        f = _forward(H, i, case, beta=beta)
        gmu, glv = _backward(H, f, case, gz, gloss, beta=beta)
        runs.append([f["z"], f["out4"], f["w"], gmu, glv])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(_bits(a), _bits(b))
    word.fill_(2.0)                                               # the word is read at every launch
    f = _forward(H, i, case, beta=word)
    assert not torch.equal(f["out4"][0], runs[0][1][0]) and torch.equal(_bits(f["out4"][1:]), _bits(runs[0][1][1:]))
    assert torch.equal(_bits(f["z"]), _bits(runs[0][0])) and torch.equal(_bits(f["w"]), _bits(runs[0][2]))
    with pytest.raises(RuntimeError, match="one fp32 element"):
        _forward(H, i, case, beta=torch.ones(2, device="cuda"))


# ------------------------------------------------------------------ 6. autograd plumbing
def test_function_equals_the_direct_calls_and_the_parts_take_no_gradient(H):
    from disentangle_mlp_amd import functional as Fn
    i = R.make_inputs(17, 65)
    case = R.CASES[0]
    kernel, hs, lam, beta = case
    f = _forward(H, i, case)
    gz = i["gz"].cuda()
    mu, lv = f["mu"].clone().requires_grad_(True), f["lv"].clone().requires_grad_(True)
    zp = f["zp"].clone().requires_grad_(True)
    z, loss, parts = Fn.reparam_mmd(mu, lv, f["eps"], zp, beta, lam, kernel, hs)
    assert loss.requires_grad and z.requires_grad and not parts.requires_grad and parts.shape == (3,)
    assert torch.equal(_bits(z), _bits(f["z"])) and torch.equal(_bits(loss), _bits(f["out4"][0]))
    assert torch.equal(_bits(parts), _bits(f["out4"][1:]))
    (GLOSS * loss + (z * gz).sum()).backward()
    gmu, glv = _backward(H, f, case, gz, torch.full((), GLOSS, device="cuda"))
    assert torch.equal(_bits(mu.grad), _bits(gmu)) and torch.equal(_bits(lv.grad), _bits(glv))
    assert zp.grad is None                                        # the prior's draws take no gradient
    # one output alone: the other term is absent, not zero-filled
    for use, (a, b) in (("loss", (None, torch.ones((), device="cuda"))), ("z", (gz, None))):
        mu.grad = lv.grad = None
        z, loss, _ = Fn.reparam_mmd(mu, lv, f["eps"], f["zp"], beta, lam, kernel, hs)
        (loss if use == "loss" else (z * gz).sum()).backward()
        gmu, glv = _backward(H, f, case, a, b)
        assert torch.equal(_bits(mu.grad), _bits(gmu)) and torch.equal(_bits(lv.grad), _bits(glv)), use
    # beta as a tensor is the word itself; the default kernel is imq with WAE's bandwidths
    word = torch.full((1,), beta, device="cuda")
    z, loss, _ = Fn.reparam_mmd(mu, lv, f["eps"], f["zp"], word, lam, kernel, hs)
    assert torch.equal(_bits(loss), _bits(f["out4"][0]))
    f2 = _forward(H, i, R.CASES[1])
    _, loss, _ = Fn.reparam_mmd(mu, lv, f["eps"], f["zp"], beta, lam)
    assert torch.equal(_bits(loss), _bits(f2["out4"][0]))


# ------------------------------------------------------------------ 7. VAETrainer
def _same_outputs_and_weights(ta, tb, oa, ob, what):
    from test_grad_clip_trainer_gpu import _assert_same, _weights
    assert oa.keys() == ob.keys()
    for k in oa:
        assert torch.equal(_bits(oa[k].float()), _bits(ob[k].float())), (what, k)
    _assert_same(_weights(ta), _weights(tb))


def test_vae_trainer_step_against_the_fp64_oracle():
    from disentangle_mlp_amd import trainer as T
    from oracle import modules as omod, steps as osteps
    beta, kernel, lam = 6.0, "imq", 1000.0
    b = osteps.synthetic_batch(8)
    names = None
    ref = {}
    for dt in (torch.float64, torch.float32):
        torch.manual_seed(999)                                    # VAETrainer's recipe: the VAE alone (new_vae.py:33-37)
        net = omod.VAE(omod.OracleOpt())
        net.apply(omod.weights_init)
        net = net.to(dt)
        net.train()
        data, eps, prior = b["data"].to(dt), b["eps2"].to(dt), b["eps3"].to(dt)
        mu, logvar = net.encode(data)
        z = net.reparameterize(mu, logvar, eps)
        mse = osteps.recon_loss(net.decode(z), data)
        o = R.objective(mu, logvar, z, prior, beta, kernel, lam)
        (mse + o["loss"]).backward()
        names = [k for k, _ in net.named_parameters() if k not in BN_SHADOWED["eg"]]
        gn = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for k, p in net.named_parameters() if k in names))
        ref[dt] = dict(mse=mse.item(), kld=o["loss"].item(), kl=o["kl"].item(), mmd=o["mmd"].item(),
                       mmd_kzz=o["kzz"].item(), gradnorm=gn)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    tr = T.VAETrainer(beta=beta, mmd_vae=(kernel, lam))
    seen = {}

    def hook(phase, net):
        seen[phase] = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for k, p in net.named_parameters() if k in names))

    out = tr.step(b["data"].cuda(), b["eps2"].cuda(), grad_hook=hook, prior=b["eps3"].cuda())
    assert set(out) == {"mse", "kld", "kl", "mmd", "mmd_kzz"}
    for k in out:
        tol = max(LOSS_TOL["mse" if k == "mse" else "kld"], 5 * gap(r32[k], r64[k]))
        print(f"{k}: {float(out[k]):.8g}  oracle fp64 {r64[k]:.8g}  fp32 {r32[k]:.8g}  tol {tol:.1e}")
        assert gap(float(out[k]), r64[k]) <= tol, (k, float(out[k]), r64[k])
    # the step differentiates at the initial weights, as phase "D" does: no optimizer step in front of it
    tol = max(GRADNORM_TOL["D"], 5 * gap(r32["gradnorm"], r64["gradnorm"]))
    print(f"gradient norm: {seen['VAE']:.8g}  oracle fp64 {r64['gradnorm']:.8g}  fp32 {r32['gradnorm']:.8g}  tol {tol:.1e}")
    assert gap(seen["VAE"], r64["gradnorm"]) <= tol


# ------------------------------------------------------------------ 8. captured = eager
def test_vae_trainer_captured_steps_equal_eager_steps():
    from disentangle_mlp_amd import trainer as T
    from test_grad_clip_trainer_gpu import _batch
    x, lat = _batch(8)
    kw = dict(beta=6.0, mmd_vae=("imq", 1000.0))
    tg, te = T.VAETrainer(graph=True, capturable=True, **kw), T.VAETrainer(graph=False, **kw)
    for it in range(4):
        og = {k: v.clone() for k, v in tg.step(x, lat[0], prior=lat[1]).items()}
        oe = {k: v.clone() for k, v in te.step(x, lat[0], prior=lat[1]).items()}
        assert len(oe) == 5
        _same_outputs_and_weights(tg, te, og, oe, it)
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs


# ------------------------------------------------------------------ 9. BetaVAEGANTrainer, beta on a schedule
def test_vaegan_trainer_with_a_beta_schedule_replays_one_graph():
    from disentangle_mlp_amd import trainer as T
    from test_grad_clip_trainer_gpu import _batch
    from test_schedules_gpu import _beta_warmup
    x, lat = _batch()
    prior = torch.randn(x.shape[0], 128, generator=torch.Generator().manual_seed(12)).cuda()
    count = {"n": 0}
    real = T._CapturedIteration.replay

    def replay(self, *args, **kw):
        count["n"] += 1
        return real(self, *args, **kw)

    lam = 1000.0
    kw = dict(beta_schedule=_beta_warmup, mmd_vae=("rbf", lam))
    tg, te = T.BetaVAEGANTrainer(graph=True, **kw), T.BetaVAEGANTrainer(graph=False, **kw)
    T._CapturedIteration.replay = replay
    try:
        for it in range(6):
            og = {k: v.clone() for k, v in tg.step(x, *lat, prior=prior).items()}
            oe = {k: v.clone() for k, v in te.step(x, *lat, prior=prior).items()}
            assert set(oe) == {"errD_real", "errD_fake", "D_x_sum", "errG_fake", "errG_recon", "sim", "mse_dec", "kld",
                               "mse_enc", "kl", "mmd", "mmd_kzz"}
            _same_outputs_and_weights(tg, te, og, oe, it)
            assert tg.beta == te.beta == _beta_warmup(it)
    finally:
        T._CapturedIteration.replay = real
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs
    assert count["n"] == 4                                        # every iteration after the two warm-up ones
    # the weighted loss is what the parts say, with that iteration's beta: four fp32 roundings -- of kl, of mmd, of the
    # loss, each formed in fp64, and one to spare -- relative to the terms' magnitudes.  mmd's own rounding is relative to
    # mmd (it is stored as one fp32 number), so its term enters with |B lambda mmd|.
    B = x.shape[0]
    terms = [_beta_warmup(5) * float(og["kl"]), B * lam * float(og["mmd"])]
    assert abs(float(og["kld"]) - sum(terms)) <= 4 * 2.0 ** -24 * (sum(abs(t) for t in terms) + abs(float(og["kld"])))


# ------------------------------------------------------------------ 10. the prior's draw
def test_the_prior_is_drawn_from_the_trainer_s_stream_after_the_other_latents():
    from disentangle_mlp_amd import trainer as T
    from test_grad_clip_trainer_gpu import _batch
    x, lat = _batch(8)
    kw = dict(beta=6.0, mmd_vae=("imq", 1000.0), graph=False)
    # eps given: the prior is the stream's next draw
    a, b, stream = T.VAETrainer(**kw), T.VAETrainer(**kw), T.VAETrainer(**kw)
    oa = a.step(x, lat[0])
    ob = b.step(x, lat[0], prior=stream.draw_latents(8))
    _same_outputs_and_weights(a, b, oa, ob, "eps given")
    # nothing given: eps first, the prior last (the streams of a and of `stream` are one draw on; b's is where it began)
    eps, prior = stream.draw_latents(8), stream.draw_latents(8)
    oa = a.step(x)
    ob = b.step(x, eps, prior=prior)
    _same_outputs_and_weights(a, b, oa, ob, "nothing given")
    # inside a capture the draw goes straight into the static buffer: the same values
    g, e = T.VAETrainer(**{**kw, "graph": True, "capturable": True}), T.VAETrainer(**kw)
    for it in range(4):
        og = {k: v.clone() for k, v in g.step(x, lat[0]).items()}
        oe = {k: v.clone() for k, v in e.step(x, lat[0]).items()}
        _same_outputs_and_weights(g, e, og, oe, ("drawn under a graph", it))
    assert len(g._graphs) == 1


# ------------------------------------------------------------------ 11. the option left off
def test_without_the_option_the_trainers_are_what_they_were(monkeypatch):
    from disentangle_mlp_amd import model as M, ops, trainer as T
    from test_grad_clip_trainer_gpu import _batch

    def never(*a, **k):
        raise AssertionError("the MMD objective ran without mmd_vae")

    monkeypatch.setattr(M.VAE, "forward_with_mmd", never)
    monkeypatch.setattr(ops, "reparam_mmd_fwd", never)
    x, lat = _batch()
    for cls, args, keys in ((T.BetaVAEGANTrainer, (x, *lat), 9), (T.VAETrainer, (x, lat[0]), 2)):
        for graph, steps in ((True, 3), (False, 1)):              # (the third step of a shape is the captured one)
            a, b = cls(graph=graph), cls(graph=graph, mmd_vae=None)      # the parent's signature / the new argument at its default
            assert a._latents == b._latents == cls._latents
            for it in range(steps):
                oa = {k: v.clone() for k, v in a.step(*args).items()}
                ob = {k: v.clone() for k, v in b.step(*args).items()}
                assert len(oa) == keys
                _same_outputs_and_weights(a, b, oa, ob, (cls.__name__, graph, it))
            assert len(a._graphs) == len(b._graphs) == (1 if graph else 0)
            assert set(a.checkpoint(0)) == set(b.checkpoint(0))
