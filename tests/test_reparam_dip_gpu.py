"""GPU: the fused DIP-VAE kernels (csrc/reparam_dip.hip) against the fp64 restatement of tests/_dip_refs.py, and through
`functional.ReparamDIPFn`, `VAE.forward_with_dip` and the trainers' ``dip_vae``.

Bound of every parity check, per tensor: max error over the reference's largest magnitude <= max(1e-6, 5 x the same
figure of the restatement evaluated in fp32) -- the project's convention (conftest.check_state, SURVEY KAT-0).  Each
check prints its figures before it asserts (``pytest -s``).

Shapes: a single sample (C = 0 in variant I), partial wavefronts, D off every multiple of 64 and of the 32-wide
covariance tile, one tile and several (mirrored ones included), more rows than one 64-row chunk of the covariance pass and
than one 16-row block of the backward, B above and below D, (3, 600): ten strips, 190 tiles, idle wavefronts -- and once
(1024, 1024), the largest the kernels take."""
import math

import pytest
import torch

import _dip_refs as R
from conftest import BN_SHADOWED, GRADNORM_TOL, LOSS_TOL, gap

pytestmark = pytest.mark.gpu

GLOSS = 0.75
MODES = ("gz+gloss", "gloss", "gz")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


_cache = {}


def _refs(key, inputs, case, beta=R.BETA):
    """(fp64, fp32) restatement of one case: computed once, shared, never modified."""
    k = (key, case, beta)
    if k not in _cache:
        _cache[k] = tuple(R.reparam_dip(inputs["mu"], inputs["lv"], inputs["eps"], beta, *case, dtype=dt)
                          for dt in (torch.float64, torch.float32))
    return _cache[k]


def _forward(H, i, case, beta=R.BETA):
    variant, lod, ld = case
    mu, lv, eps = (i[k].cuda() for k in ("mu", "lv", "eps"))
    z, out4, cov, mean = H.reparam_dip_fwd(mu, lv, eps, beta, lod, ld, variant)
    return dict(mu=mu, lv=lv, eps=eps, z=z, out4=out4, cov=cov, mean=mean)


def _backward(H, f, case, gz, gloss, beta=R.BETA):
    variant, lod, ld = case
    return H.reparam_dip_bwd(gz, f["mu"], f["lv"], f["eps"], f["cov"], f["mean"], gloss, beta, lod, ld, variant)


def _check(what, got, r32, r64):
    e, b = R.rel_err(got, r64), R.bound(r32, r64)
    print(f"{what}: error {e:.3e}  bound {b:.3e}  (fp32 restatement {R.rel_err(r32, r64):.3e})")
    assert torch.isfinite(torch.as_tensor(got)).all(), what
    assert e <= b, (what, e, b)


def _check_forward(what, f, r64, r32):
    _check(f"{what} z", f["z"], r32["z"], r64["z"])
    out4 = f["out4"].cpu()
    for n, name in enumerate(("loss", "kl", "od", "dg")):
        _check(f"{what} {name}", out4[n], r32[name], r64[name])
    _check(f"{what} cov", f["cov"], r32["cov"], r64["cov"])
    assert torch.equal(_bits(f["cov"]), _bits(f["cov"].t()))      # G is symmetric to the bit


def _check_backward(H, what, f, i, case, r64, r32, modes=MODES, beta=R.BETA):
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    for mode in modes:
        a = gz if "gz" in mode else None
        b = gloss if "gloss" in mode else None
        gmu, glv = _backward(H, f, case, a, b, beta)
        want = [R.expected_grads(r, i["lv"], i["eps"], i["gz"] if a is not None else None, GLOSS if b is not None else None,
                                 dtype=dt) for r, dt in ((r64, torch.float64), (r32, torch.float32))]
        _check(f"{what} gmu [{mode}]", gmu, want[1][0], want[0][0])
        _check(f"{what} glv [{mode}]", glv, want[1][1], want[0][1])


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


def _kl_z(H, f):
    return H.reparam_kl_fwd(f["mu"], f["lv"], f["eps"], R.BETA)[0]


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


def test_parity_at_the_largest_shape(H):
    """(1024, 1024), the contract's upper edge: every KL slot, all 528 tiles, 16 chunks of rows, 64 blocks of rows."""
    shape, case = (1024, 1024), R.CASES[1]
    i = R.make_inputs(*shape)
    r64, r32 = _refs(shape, i, case)
    f = _forward(H, i, case)
    _check_forward(f"{shape} {case}", f, r64, r32)
    _check_backward(H, f"{shape} {case}", f, i, case, r64, r32, modes=("gz+gloss",))


# ------------------------------------------------------------------ 2. identical rows: no spread at all
def test_identical_rows(H):
    i = {k: v[:1].repeat(8, 1).contiguous() for k, v in R.make_inputs(8, 16).items()}
    case = R.CASES[0]                                             # variant I
    r64, r32 = _refs("same-rows", i, case)
    f = _forward(H, i, case)
    _check_forward("same rows", f, r64, r32)
    out4 = f["out4"].cpu()
    assert float(out4[2]) == 0.0 and float(out4[3]) == 16.0       # C = 0 exactly: od = 0, dg = D
    assert float(f["cov"].abs().max()) == 0.0
    _check_backward(H, "same rows", f, i, case, r64, r32)
    # the penalty's share of gmu is exactly zero (c = 0): with gloss alone, gmu = gloss * beta * mu
    gmu, glv = _backward(H, f, case, None, torch.full((), GLOSS, device="cuda"))
    assert torch.isfinite(gmu).all() and torch.isfinite(glv).all()
    want64, want32 = GLOSS * R.BETA * i["mu"].double(), GLOSS * R.BETA * i["mu"]
    _check("same rows gmu vs gloss*beta*mu", gmu, want32, want64)


# ------------------------------------------------------------------ 3. a common offset on the means
@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[1]], ids=str)
def test_a_common_offset_of_the_means_costs_nothing(H, case):
    """E[mu mu^T] - m m^T in fp32 loses the covariance under an offset of 30 (900 against 1: 1e-4 of it is gone); the
    centred form does not.  The restatement's own fp32 error here is <= 4.2e-7."""
    i = dict(R.make_inputs(64, 128))
    i["mu"] = i["mu"] + 30.0
    r64, r32 = _refs("offset", i, case)
    f = _forward(H, i, case)
    _check_forward(f"offset {case}", f, r64, r32)
    _check_backward(H, f"offset {case}", f, i, case, r64, r32)


# ------------------------------------------------------------------ 4. both lambdas 0: the plain KL
@pytest.mark.parametrize("variant", ["i", "ii"])
@pytest.mark.parametrize("shape", [(17, 65), (128, 128)], ids=str)
def test_zero_lambdas_give_the_plain_kl(H, shape, variant):
    i = R.make_inputs(*shape)
    case = (variant, 0.0, 0.0)
    r64, r32 = _refs(shape, i, case)
    f = _forward(H, i, case)
    z, kl, _ = H.reparam_kl_fwd(f["mu"], f["lv"], f["eps"], R.BETA)
    assert torch.equal(_bits(f["z"]), _bits(z))
    _check(f"{shape} loss", f["out4"][0].cpu(), r32["loss"], r64["loss"])
    e = R.rel_err(f["out4"][0].cpu(), kl.cpu().double().reshape(()))
    print(f"{shape} {variant} loss against reparam_kl_fwd: {e:.3e}")
    assert e <= R.bound(r32["loss"], r64["loss"])
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    gmu, glv = _backward(H, f, case, gz, gloss)
    kmu, klv = H.reparam_kl_bwd(gz, f["mu"], f["lv"], f["eps"], gloss, R.BETA)
    want = [R.expected_grads(r, i["lv"], i["eps"], i["gz"], GLOSS, dtype=dt) for r, dt in ((r64, torch.float64), (r32, torch.float32))]
    for name, got, ref, n in (("gmu", gmu, kmu, 0), ("glv", glv, klv, 1)):
        _check(f"{shape} {name}", got, want[1][n], want[0][n])
        e, b = R.rel_err(got, ref), R.bound(want[1][n], want[0][n])
        print(f"{shape} {variant} {name} against reparam_kl_bwd: {e:.3e}  bound {b:.3e}")
        assert e <= b


# ------------------------------------------------------------------ 5. beta as a float / as a device word; run to run
@pytest.mark.parametrize("shape", [(5, 7), (128, 128), (130, 200)], ids=str)
def test_beta_word_and_repeated_runs_give_the_same_bits(H, shape):
    i = R.make_inputs(*shape)
    case = R.CASES[1]
    word = torch.full((1,), R.BETA, dtype=torch.float32, device="cuda")
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    runs = []
    for beta in (R.BETA, word, R.BETA):
        f = _forward(H, i, case, beta=beta)
        gmu, glv = _backward(H, f, case, gz, gloss, beta=beta)
        runs.append([f["z"], f["out4"], f["cov"], f["mean"], gmu, glv])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(_bits(a), _bits(b))
    word.fill_(2.0)                                               # the word is read at every launch
    f = _forward(H, i, case, beta=word)
    assert not torch.equal(f["out4"][0], runs[0][1][0]) and torch.equal(_bits(f["out4"][1:]), _bits(runs[0][1][1:]))
    with pytest.raises(RuntimeError, match="one fp32 element"):
        _forward(H, i, case, beta=torch.ones(2, device="cuda"))


# ------------------------------------------------------------------ 6. autograd plumbing
def test_function_equals_the_direct_calls_and_the_parts_take_no_gradient(H):
    from disentangle_mlp_amd import functional as Fn
    i = R.make_inputs(17, 65)
    case = R.CASES[1]
    variant, lod, ld = case
    f = _forward(H, i, case)
    gz = i["gz"].cuda()
    mu, lv = f["mu"].clone().requires_grad_(True), f["lv"].clone().requires_grad_(True)
    z, loss, parts = Fn.reparam_dip(mu, lv, f["eps"], R.BETA, lod, ld, variant)
    assert loss.requires_grad and z.requires_grad and not parts.requires_grad and parts.shape == (3,)
    assert torch.equal(_bits(z), _bits(f["z"])) and torch.equal(_bits(loss), _bits(f["out4"][0]))
    assert torch.equal(_bits(parts), _bits(f["out4"][1:]))
    (GLOSS * loss + (z * gz).sum()).backward()
    gmu, glv = _backward(H, f, case, gz, torch.full((), GLOSS, device="cuda"))
    assert torch.equal(_bits(mu.grad), _bits(gmu)) and torch.equal(_bits(lv.grad), _bits(glv))
    # one output alone: the other term is absent, not zero-filled
    for use, (a, b) in (("loss", (None, torch.ones((), device="cuda"))), ("z", (gz, None))):
        mu.grad = lv.grad = None
        z, loss, _ = Fn.reparam_dip(mu, lv, f["eps"], R.BETA, lod, ld, variant)
        (loss if use == "loss" else (z * gz).sum()).backward()
        gmu, glv = _backward(H, f, case, a, b)
        assert torch.equal(_bits(mu.grad), _bits(gmu)) and torch.equal(_bits(lv.grad), _bits(glv)), use
    # beta as a tensor is the word itself
    word = torch.full((1,), R.BETA, device="cuda")
    z, loss, _ = Fn.reparam_dip(mu, lv, f["eps"], word, lod, ld, variant)
    assert torch.equal(_bits(loss), _bits(f["out4"][0]))


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
    beta, case = 6.0, ("ii", 10.0, 10.0)
    b = osteps.synthetic_batch(8)
    names = None
    ref = {}
    for dt in (torch.float64, torch.float32):
        torch.manual_seed(999)                                    # VAETrainer's recipe: the VAE alone (new_vae.py:33-37)
        net = omod.VAE(omod.OracleOpt())
        net.apply(omod.weights_init)
        net = net.to(dt)
        net.train()
        data, eps = b["data"].to(dt), b["eps2"].to(dt)
        mu, logvar = net.encode(data)
        z = net.reparameterize(mu, logvar, eps)
        mse = osteps.recon_loss(net.decode(z), data)
        o = R.objective(mu, logvar, beta, *case)
        (mse + o["loss"]).backward()
        names = [k for k, _ in net.named_parameters() if k not in BN_SHADOWED["eg"]]
        gn = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for k, p in net.named_parameters() if k in names))
        ref[dt] = dict(mse=mse.item(), kld=o["loss"].item(), kl=o["kl"].item(), dip_od=o["od"].item(),
                       dip_d=o["dg"].item(), gradnorm=gn)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    tr = T.VAETrainer(beta=beta, dip_vae=case)
    seen = {}

    def hook(phase, net):
        seen[phase] = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for k, p in net.named_parameters() if k in names))

    out = tr.step(b["data"].cuda(), b["eps2"].cuda(), grad_hook=hook)
    assert set(out) == {"mse", "kld", "kl", "dip_od", "dip_d"}
    for k in out:
        tol = max(LOSS_TOL["mse" if k == "mse" else "kld"], 5 * gap(r32[k], r64[k]))
        print(f"{k}: {float(out[k]):.8g}  oracle fp64 {r64[k]:.8g}  fp32 {r32[k]:.8g}  tol {tol:.1e}")
        assert gap(float(out[k]), r64[k]) <= tol, (k, float(out[k]), r64[k])
    # the step differentiates at the initial weights, as phase "D" does: no optimizer step in front of it
    tol = max(GRADNORM_TOL["D"], 5 * gap(r32["gradnorm"], r64["gradnorm"]))
    print(f"gradient norm: {seen['VAE']:.8g}  oracle fp64 {r64['gradnorm']:.8g}  fp32 {r32['gradnorm']:.8g}  tol {tol:.1e}")
    assert gap(seen["VAE"], r64["gradnorm"]) <= tol


def test_vae_trainer_captured_steps_equal_eager_steps():
    from disentangle_mlp_amd import trainer as T
    from test_grad_clip_trainer_gpu import _batch
    x, lat = _batch(8)
    kw = dict(beta=6.0, dip_vae=("ii", 10.0, 10.0))
    tg, te = T.VAETrainer(graph=True, capturable=True, **kw), T.VAETrainer(graph=False, **kw)
    for it in range(4):
        og = {k: v.clone() for k, v in tg.step(x, lat[0]).items()}
        oe = {k: v.clone() for k, v in te.step(x, lat[0]).items()}
        assert len(oe) == 5
        _same_outputs_and_weights(tg, te, og, oe, it)
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs


# ------------------------------------------------------------------ 8. BetaVAEGANTrainer, beta on a schedule
def test_vaegan_trainer_with_a_beta_schedule_replays_one_graph():
    from disentangle_mlp_amd import trainer as T
    from test_grad_clip_trainer_gpu import _batch
    from test_schedules_gpu import _beta_warmup
    x, lat = _batch()
    count = {"n": 0}
    real = T._CapturedIteration.replay

    def replay(self, *args, **kw):
        count["n"] += 1
        return real(self, *args, **kw)

    kw = dict(beta_schedule=_beta_warmup, dip_vae=("i", 10.0, 100.0))
    tg, te = T.BetaVAEGANTrainer(graph=True, **kw), T.BetaVAEGANTrainer(graph=False, **kw)
    T._CapturedIteration.replay = replay
    try:
        for it in range(6):
            og = {k: v.clone() for k, v in tg.step(x, *lat).items()}
            oe = {k: v.clone() for k, v in te.step(x, *lat).items()}
            assert set(oe) == {"errD_real", "errD_fake", "D_x_sum", "errG_fake", "errG_recon", "sim", "mse_dec", "kld",
                               "mse_enc", "kl", "dip_od", "dip_d"}
            _same_outputs_and_weights(tg, te, og, oe, it)
            assert tg.beta == te.beta == _beta_warmup(it)
    finally:
        T._CapturedIteration.replay = real
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs
    assert count["n"] == 4                                        # every iteration after the two warm-up ones
    # the weighted loss is what the parts say, with that iteration's beta
    # (four fp32 roundings -- of the three parts and of the loss, each formed in fp64 -- relative to the terms' magnitudes)
    B = x.shape[0]
    terms = [_beta_warmup(5) * float(og["kl"]), B * 10.0 * float(og["dip_od"]), B * 100.0 * float(og["dip_d"])]
    assert abs(float(og["kld"]) - sum(terms)) <= 4 * 2.0 ** -24 * (sum(abs(t) for t in terms) + abs(float(og["kld"])))


# ------------------------------------------------------------------ 9. the option left off
def test_without_the_option_the_trainers_are_what_they_were(monkeypatch):
    from disentangle_mlp_amd import model as M, ops, trainer as T
    from test_grad_clip_trainer_gpu import _batch

    def never(*a, **k):
        raise AssertionError("the DIP-VAE objective ran without dip_vae")

    monkeypatch.setattr(M.VAE, "forward_with_dip", never)
    monkeypatch.setattr(ops, "reparam_dip_fwd", never)
    x, lat = _batch()
    for cls, args, keys in ((T.BetaVAEGANTrainer, (x, *lat), 9), (T.VAETrainer, (x, lat[0]), 2)):
        for graph, steps in ((True, 3), (False, 1)):              # (the third step of a shape is the captured one)
            a, b = cls(graph=graph), cls(graph=graph, dip_vae=None)      # the parent's signature / the new argument at its default
            for it in range(steps):
                oa = {k: v.clone() for k, v in a.step(*args).items()}
                ob = {k: v.clone() for k, v in b.step(*args).items()}
                assert len(oa) == keys
                _same_outputs_and_weights(a, b, oa, ob, (cls.__name__, graph, it))
            assert len(a._graphs) == len(b._graphs) == (1 if graph else 0)
            assert set(a.checkpoint(0)) == set(b.checkpoint(0))
