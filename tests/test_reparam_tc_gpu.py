"""GPU: the fused beta-TCVAE kernel pair (csrc/reparam_tc.hip) against the fp64 restatement of tests/_tc_refs.py, and
through `functional.ReparamTCFn`, `VAE.forward_with_tc` and the trainers' ``tc_decomposition``.

Bound of every parity check, per tensor: max error over the reference's largest magnitude <= max(1e-6, 5 x the same
figure of the restatement evaluated in fp32) -- the project's convention (conftest.check_state, SURVEY KAT-0).  Each
check prints its figures before it asserts (``pytest -s``).

Shapes: the issue's eight -- a single pair, a partial wavefront, D not a multiple of 64, B not a multiple of the eight
wavefronts of a workgroup, D <= 128 (two elements of a row per lane) and D > 128 (the 16-element variant) -- and (3, 600):
the wide variant with idle wavefronts and D off every multiple."""
import math

import pytest
import torch

import _tc_refs as R
from conftest import BN_SHADOWED, GRADNORM_TOL, LOSS_TOL, gap

pytestmark = pytest.mark.gpu

N = R.DATASET_SIZE
SHAPES = R.SHAPES + [(3, 600)]
GLOSS = 0.75


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


_cache = {}


def _refs(key, inputs, weights, n=N):
    """(fp64, fp32) restatement of one case: computed once, shared, never modified."""
    k = (key, weights, n)
    if k not in _cache:
        _cache[k] = tuple(R.reparam_tc(inputs["mu"], inputs["lv"], inputs["eps"], *weights, dataset_size=n, dtype=dt)
                          for dt in (torch.float64, torch.float32))
    return _cache[k]


def _forward(H, i, weights, n=N, beta=None):
    alpha, b, gamma = weights
    mu, lv, eps = (i[k].cuda() for k in ("mu", "lv", "eps"))
    z, out4, lj, ld = H.reparam_tc_fwd(mu, lv, eps, b if beta is None else beta, alpha, gamma, math.log(mu.shape[0] * n))
    return dict(mu=mu, lv=lv, eps=eps, z=z, out4=out4, lse_joint=lj, lse_dim=ld)


def _backward(H, f, weights, gz, gloss, beta=None):
    alpha, b, gamma = weights
    return H.reparam_tc_bwd(gz, f["mu"], f["lv"], f["eps"], f["z"], f["lse_joint"], f["lse_dim"], gloss,
                            b if beta is None else beta, alpha, gamma)


def _check(what, got, r32, r64):
    e, b = R.rel_err(got, r64), R.bound(r32, r64)
    print(f"{what}: error {e:.3e}  bound {b:.3e}  (fp32 restatement {R.rel_err(r32, r64):.3e})")
    assert torch.isfinite(torch.as_tensor(got)).all(), what
    assert e <= b, (what, e, b)


def _check_forward(what, f, r64, r32):
    _check(f"{what} z", f["z"], r32["z"], r64["z"])
    out4 = f["out4"].cpu()
    for n, name in enumerate(("loss", "mi", "tc", "dwkl")):
        _check(f"{what} {name}", out4[n], r32[name], r64[name])


def _check_backward(H, what, f, i, weights, r64, r32, modes=("gz+gloss", "gloss", "gz")):
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    for mode in modes:
        a = gz if "gz" in mode else None
        b = gloss if "gloss" in mode else None
        gmu, glv = _backward(H, f, weights, a, b)
        want = [R.expected_grads(r, i["lv"], i["eps"], i["gz"] if a is not None else None, GLOSS if b is not None else None,
                                 dtype=dt) for r, dt in ((r64, torch.float64), (r32, torch.float32))]
        _check(f"{what} gmu [{mode}]", gmu, want[1][0], want[0][0])
        _check(f"{what} glv [{mode}]", glv, want[1][1], want[0][1])


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("weights", R.WEIGHTS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_parity_with_the_fp64_restatement(H, shape, weights):
    i = R.make_inputs(*shape)
    r64, r32 = _refs(shape, i, weights)
    f = _forward(H, i, weights)
    what = f"{shape} {weights}"
    _check_forward(what, f, r64, r32)
    _check_backward(H, what, f, i, weights, r64, r32)


# ------------------------------------------------------------------ 2. posteriors that do not overlap
def test_non_overlapping_posteriors_stay_finite():
    from disentangle_mlp_amd import ops as H
    i = R.make_inputs(16, 128)
    i["mu"] = i["mu"] * 3.0
    i["lv"] = torch.full_like(i["lv"], -8.0)
    weights = R.WEIGHTS[0]
    r64, r32 = _refs("apart", i, weights)
    f = _forward(H, i, weights)
    _check_forward("apart", f, r64, r32)
    assert torch.isfinite(f["lse_joint"]).all() and torch.isfinite(f["lse_dim"]).all()
    _check_backward(H, "apart", f, i, weights, r64, r32)
    # w is one-hot (in fp64): the joint log-sum-exp is the diagonal row sum itself
    lq = R.pair_terms(r64["z"], i["mu"].double(), i["lv"].double()).sum(2)
    w = torch.softmax(lq, dim=1)
    assert float((w - torch.eye(16, dtype=torch.float64)).abs().max()) < 1e-30
    assert R.rel_err(f["lse_joint"], lq.diagonal()) <= 1e-6


# ------------------------------------------------------------------ 3. identical rows: w uniform
def test_identical_rows():
    from disentangle_mlp_amd import ops as H
    i = {k: v[:1].repeat(8, 1).contiguous() for k, v in R.make_inputs(8, 16).items()}
    i["gz"] = R.make_inputs(8, 16)["gz"]
    weights = R.WEIGHTS[0]                                        # beta != alpha: w enters the gradients
    r64, r32 = _refs("same-rows", i, weights)
    f = _forward(H, i, weights)
    _check_forward("same rows", f, r64, r32)
    _check_backward(H, "same rows", f, i, weights, r64, r32, modes=("gloss", "gz+gloss"))


# ------------------------------------------------------------------ 4. equal weights: the plain identity, N drops out
@pytest.mark.parametrize("shape", [(17, 65), (128, 128)], ids=str)
def test_equal_weights_give_the_identity_for_every_dataset_size(H, shape):
    i = R.make_inputs(*shape)
    weights = (1.0, 1.0, 1.0)
    grads = []
    for n in (N, 1000):
        r64, r32 = _refs(shape, i, weights, n)
        f = _forward(H, i, weights, n)
        _check(f"{shape} N={n} loss vs sum_i (lqzx_i - lpz_i)", f["out4"][0].cpu(), r32["identity"], r64["identity"])
        grads.append(_backward(H, f, weights, i["gz"].cuda(), torch.full((), GLOSS, device="cuda")))
    weights = R.WEIGHTS[1]                                        # ... and with any weights N moves no gradient
    for n in (N, 1000):
        f = _forward(H, i, weights, n)
        grads.append(_backward(H, f, weights, None, torch.ones((), device="cuda")))
    for a, b in ((grads[0], grads[1]), (grads[2], grads[3])):
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


# ------------------------------------------------------------------ 5. beta as a float / as a device word; run to run
@pytest.mark.parametrize("shape", [(5, 7), (128, 128), (130, 200)], ids=str)
def test_beta_word_and_repeated_runs_give_the_same_bits(H, shape):
    i = R.make_inputs(*shape)
    weights = R.WEIGHTS[1]
    word = torch.full((1,), weights[1], dtype=torch.float32, device="cuda")
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    runs = []
    for beta in (None, word, None):
        f = _forward(H, i, weights, beta=beta)
        gmu, glv = _backward(H, f, weights, gz, gloss, beta=beta)
        runs.append([f["z"], f["out4"], f["lse_joint"], f["lse_dim"], gmu, glv])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(_bits(a), _bits(b))
    word.fill_(2.0)                                               # the word is read at every launch
    f = _forward(H, i, weights, beta=word)
    assert not torch.equal(f["out4"][0], runs[0][1][0]) and torch.equal(_bits(f["out4"][1:]), _bits(runs[0][1][1:]))
    with pytest.raises(RuntimeError, match="one fp32 element"):
        _forward(H, i, weights, beta=torch.ones(2, device="cuda"))


# ------------------------------------------------------------------ 6. autograd plumbing
def test_function_equals_the_direct_calls_and_the_parts_take_no_gradient(H):
    from disentangle_mlp_amd import functional as Fn
    i = R.make_inputs(17, 65)
    weights = R.WEIGHTS[0]
    f = _forward(H, i, weights)
    gz = i["gz"].cuda()
    mu, lv = f["mu"].clone().requires_grad_(True), f["lv"].clone().requires_grad_(True)
    z, loss, parts = Fn.reparam_tc(mu, lv, f["eps"], weights[1], weights[0], weights[2], dataset_size=N)
    assert loss.requires_grad and z.requires_grad and not parts.requires_grad and parts.shape == (3,)
    assert torch.equal(_bits(z), _bits(f["z"])) and torch.equal(_bits(loss), _bits(f["out4"][0]))
    assert torch.equal(_bits(parts), _bits(f["out4"][1:]))
    (GLOSS * loss + (z * gz).sum()).backward()
    gmu, glv = _backward(H, f, weights, gz, torch.full((), GLOSS, device="cuda"))
    assert torch.equal(_bits(mu.grad), _bits(gmu)) and torch.equal(_bits(lv.grad), _bits(glv))
    # one output alone: the other term is absent, not zero-filled
    for use, (a, b) in (("loss", (None, torch.ones((), device="cuda"))), ("z", (gz, None))):
        mu.grad = lv.grad = None
        z, loss, _ = Fn.reparam_tc(mu, lv, f["eps"], weights[1], weights[0], weights[2], dataset_size=N)
        (loss if use == "loss" else (z * gz).sum()).backward()
        gmu, glv = _backward(H, f, weights, a, b)
        assert torch.equal(_bits(mu.grad), _bits(gmu)) and torch.equal(_bits(lv.grad), _bits(glv)), use
    # beta as a tensor is the word itself
    word = torch.full((1,), weights[1], device="cuda")
    z, loss, _ = Fn.reparam_tc(mu, lv, f["eps"], word, weights[0], weights[2], dataset_size=N)
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
    alpha, beta, gamma = 1.0, 6.0, 1.0
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
        parts = R.decomposition(z, mu, logvar, N)
        kld = R.weighted(parts, alpha, beta, gamma)
        (mse + kld).backward()
        names = [k for k, _ in net.named_parameters() if k not in BN_SHADOWED["eg"]]
        gn = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for k, p in net.named_parameters() if k in names))
        ref[dt] = dict(mse=mse.item(), kld=kld.item(), mi=parts["mi"].item(), tc=parts["tc"].item(),
                       dwkl=parts["dwkl"].item(), gradnorm=gn)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    tr = T.VAETrainer(beta=beta, tc_decomposition=(alpha, gamma), dataset_size=N)
    seen = {}

    def hook(phase, net):
        seen[phase] = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for k, p in net.named_parameters() if k in names))

    out = tr.step(b["data"].cuda(), b["eps2"].cuda(), grad_hook=hook)
    assert set(out) == {"mse", "kld", "mi", "tc", "dwkl"}
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
    kw = dict(beta=6.0, tc_decomposition=(1.0, 1.0), dataset_size=N)
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

    kw = dict(beta_schedule=_beta_warmup, tc_decomposition=(1.0, 1.0), dataset_size=N)
    tg, te = T.BetaVAEGANTrainer(graph=True, **kw), T.BetaVAEGANTrainer(graph=False, **kw)
    T._CapturedIteration.replay = replay
    try:
        for it in range(6):
            og = {k: v.clone() for k, v in tg.step(x, *lat).items()}
            oe = {k: v.clone() for k, v in te.step(x, *lat).items()}
            assert set(oe) == {"errD_real", "errD_fake", "D_x_sum", "errG_fake", "errG_recon", "sim", "mse_dec", "kld",
                               "mse_enc", "mi", "tc", "dwkl"}
            _same_outputs_and_weights(tg, te, og, oe, it)
            assert tg.beta == te.beta == _beta_warmup(it)
    finally:
        T._CapturedIteration.replay = real
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs
    assert count["n"] == 4                                        # every iteration after the two warm-up ones
    # the weighted loss is what the parts say, with that iteration's beta
    # (four fp32 roundings -- of the three parts and of the loss, each formed in fp64 -- relative to the terms' magnitudes)
    terms = [float(og["mi"]), _beta_warmup(5) * float(og["tc"]), float(og["dwkl"])]
    assert abs(float(og["kld"]) - sum(terms)) <= 4 * 2.0 ** -24 * (sum(abs(t) for t in terms) + abs(float(og["kld"])))


# ------------------------------------------------------------------ 9. the option left off
def test_without_the_option_the_trainers_are_what_they_were(monkeypatch):
    from disentangle_mlp_amd import model as M, ops, trainer as T
    from test_grad_clip_trainer_gpu import _batch

    def never(*a, **k):
        raise AssertionError("the decomposed KL ran without tc_decomposition")

    monkeypatch.setattr(M.VAE, "forward_with_tc", never)
    monkeypatch.setattr(ops, "reparam_tc_fwd", never)
    x, lat = _batch()
    off = dict(tc_decomposition=None, dataset_size=None)
    for cls, args, keys in ((T.BetaVAEGANTrainer, (x, *lat), 9), (T.VAETrainer, (x, lat[0]), 2)):
        for graph, steps in ((True, 3), (False, 1)):              # (the third step of a shape is the captured one)
            a, b = cls(graph=graph), cls(graph=graph, **off)      # the parent's signature / the new arguments at their defaults
            for it in range(steps):
                oa = {k: v.clone() for k, v in a.step(*args).items()}
                ob = {k: v.clone() for k, v in b.step(*args).items()}
                assert len(oa) == keys
                _same_outputs_and_weights(a, b, oa, ob, (cls.__name__, graph, it))
            assert len(a._graphs) == len(b._graphs) == (1 if graph else 0)
            assert set(a.checkpoint(0)) == set(b.checkpoint(0))
