"""GPU: the fused KL-capacity / free-bits kernels (csrc/reparam_klc.hip) against the fp64 restatement of
tests/_klc_refs.py, and through `functional.ReparamKLCFn`, `VAE.forward_with_klc` and the trainers' ``kl_control``.

Bound of every parity check, per tensor: max error over the reference's largest magnitude <= max(1e-6, 5 x the same
figure of the restatement evaluated in fp32) -- the project's convention (conftest.check_state, SURVEY KAT-0); the gate is
compared EXACTLY, every dimension of it (tests/test_reparam_klc_cpu.py asserts the margin that allows it).  Each check
prints its figures before it asserts (``pytest -s``).

Shapes: those of the DIP-VAE tests -- a single sample, partial wavefronts, D off every multiple of the 64-column strip,
one block of 64 rows and several with a partial last one, B above and below D, (3, 600): ten strips -- and once
(1024, 1024), the largest the kernels take: sixteen row blocks, every thread of the finishing workgroup."""
import math

import pytest
import torch

import _klc_refs as R
from conftest import BN_SHADOWED, GRADNORM_TOL, LOSS_TOL, gap

pytestmark = pytest.mark.gpu

GLOSS = 0.75
MODES = ("gz+gloss", "gloss", "gz")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


_cache = {}


def _refs(key, inputs, C, lam, beta=R.BETA):
    """(fp64, fp32) restatement of one case: computed once, shared, never modified."""
    k = (key, C, lam, beta)
    if k not in _cache:
        _cache[k] = tuple(R.reparam_klc(inputs["mu"], inputs["lv"], inputs["eps"], beta, C, lam, dtype=dt)
                          for dt in (torch.float64, torch.float32))
    return _cache[k]


def _forward(H, i, C, lam, beta=R.BETA):
    mu, lv, eps = (i[k].cuda() for k in ("mu", "lv", "eps"))
    z, out4, gate, kl_dim = H.reparam_klc_fwd(mu, lv, eps, beta, C, lam)
    return dict(mu=mu, lv=lv, eps=eps, z=z, out4=out4, gate=gate, kl_dim=kl_dim)


def _backward(H, f, C, lam, gz, gloss, beta=R.BETA):
    return H.reparam_klc_bwd(gz, f["mu"], f["lv"], f["eps"], f["gate"], gloss, beta, C, lam)


def _check(what, got, r32, r64):
    e, b = R.rel_err(got, r64), R.bound(r32, r64)
    print(f"{what}: error {e:.3e}  bound {b:.3e}  (fp32 restatement {R.rel_err(r32, r64):.3e})")
    assert torch.isfinite(torch.as_tensor(got)).all(), what
    assert e <= b, (what, e, b)


def _check_forward(what, f, r64, r32):
    _check(f"{what} z", f["z"], r32["z"], r64["z"])
    out4 = f["out4"].cpu()
    for n, name in enumerate(("loss", "kl", "kl_floored")):
        _check(f"{what} {name}", out4[n], r32[name], r64[name])
    print(f"{what} dims_above: {float(out4[3]):g}  reference {int(r64['dims_above'])}")
    assert float(out4[3]) == float(r64["dims_above"])
    assert torch.equal(f["gate"].cpu().double(), r64["gate"]), what      # exact, every dimension
    _check(f"{what} kl_dim", f["kl_dim"], r32["kl_dim"], r64["kl_dim"])


def _check_backward(H, what, f, i, C, lam, r64, r32, modes=MODES, beta=R.BETA):
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    for mode in modes:
        a = gz if "gz" in mode else None
        b = gloss if "gloss" in mode else None
        gmu, glv = _backward(H, f, C, lam, a, b, beta)
        want = [R.expected_grads(r, i["lv"], i["eps"], i["gz"] if a is not None else None, GLOSS if b is not None else None,
                                 dtype=dt) for r, dt in ((r64, torch.float64), (r32, torch.float32))]
        _check(f"{what} gmu [{mode}]", gmu, want[1][0], want[0][0])
        _check(f"{what} glv [{mode}]", glv, want[1][1], want[0][1])


@pytest.fixture(scope="module")
def H():
    from disentangle_mlp_amd import ops
    return ops


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("case", R.CASES, ids=str)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_parity_with_the_fp64_restatement(H, shape, case):
    i = R.make_inputs(*shape)
    C, lam = R.capacity_of(i, case), case[1]
    r64, r32 = _refs(shape, i, C, lam)
    f = _forward(H, i, C, lam)
    what = f"{shape} {case}"
    _check_forward(what, f, r64, r32)
    z = H.reparam_kl_fwd(f["mu"], f["lv"], f["eps"], R.BETA)[0]
    assert torch.equal(_bits(f["z"]), _bits(z))                   # z: the bits of reparam_kl_fwd
    _check_backward(H, what, f, i, C, lam, r64, r32)


def test_parity_at_the_largest_shape(H):
    """(1024, 1024), the contract's upper edge: sixteen strips x sixteen row blocks, a full finishing workgroup."""
    shape, case = (1024, 1024), R.CASES[4]
    i = R.make_inputs(*shape)
    C, lam = R.capacity_of(i, case), case[1]
    r64, r32 = _refs(shape, i, C, lam)
    f = _forward(H, i, C, lam)
    _check_forward(f"{shape} {case}", f, r64, r32)
    _check_backward(H, f"{shape} {case}", f, i, C, lam, r64, r32, modes=("gz+gloss",))


# ------------------------------------------------------------------ 2. no floor, no capacity: the plain beta KL
@pytest.mark.parametrize("shape", [(17, 65), (128, 128)], ids=str)
def test_zero_capacity_and_floor_give_the_plain_kl(H, shape):
    i = R.make_inputs(*shape)
    r64, r32 = _refs(shape, i, 0.0, 0.0)
    f = _forward(H, i, 0.0, 0.0)
    z, kl, _ = H.reparam_kl_fwd(f["mu"], f["lv"], f["eps"], R.BETA)
    assert torch.equal(_bits(f["z"]), _bits(z))
    out4 = f["out4"].cpu()
    assert float(out4[3]) == shape[1]                             # every dimension counts
    for n, (name, scale) in enumerate((("loss", 1.0), ("kl", R.BETA))):
        _check(f"{shape} {name}", out4[n], r32[name], r64[name])
        e, b = R.rel_err(out4[n] * scale, kl.cpu().double().reshape(())), R.bound(r32[name], r64[name])
        print(f"{shape} {name} against reparam_kl_fwd: {e:.3e}  bound {b:.3e}")
        assert e <= b
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    gmu, glv = _backward(H, f, 0.0, 0.0, gz, gloss)
    kmu, klv = H.reparam_kl_bwd(gz, f["mu"], f["lv"], f["eps"], gloss, R.BETA)
    want = [R.expected_grads(r, i["lv"], i["eps"], i["gz"], GLOSS, dtype=dt) for r, dt in ((r64, torch.float64), (r32, torch.float32))]
    for name, got, ref, n in (("gmu", gmu, kmu, 0), ("glv", glv, klv, 1)):
        _check(f"{shape} {name}", got, want[1][n], want[0][n])
        e, b = R.rel_err(got, ref), R.bound(want[1][n], want[0][n])
        print(f"{shape} {name} against reparam_kl_bwd: {e:.3e}  bound {b:.3e}")
        assert e <= b


# ------------------------------------------------------------------ 3. every dimension under its floor
def test_every_dimension_floored(H):
    i = R.make_inputs(17, 65)
    lam = 1e3
    f = _forward(H, i, 0.0, lam)
    out4 = f["out4"].cpu()
    assert float(out4[3]) == 0.0 and float(f["gate"].abs().max()) == 0.0
    _check("floored kl_floored", out4[2], torch.tensor(17 * 65 * 1e3), torch.tensor(17 * 65 * 1e3, dtype=torch.float64))
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    gmu, glv = _backward(H, f, 0.0, lam, None, gloss)
    assert float(gmu.abs().max()) == 0.0 and float(glv.abs().max()) == 0.0      # exactly: the floor has no gradient
    gmu, glv = _backward(H, f, 0.0, lam, gz, gloss)
    omu, olv = _backward(H, f, 0.0, lam, gz, None)                # the gz-only backward
    assert torch.equal(_bits(gmu), _bits(omu)) and torch.equal(_bits(glv), _bits(olv))
    assert float(omu.abs().max()) > 0.0


# ------------------------------------------------------------------ 4. an exact tie
def test_an_exact_tie_has_no_loss_and_no_gradient(H):
    """All 16 dimensions floored at B lambda = 4: T = 64 = B C exactly.  sgn(0) = 0: no loss, no direction."""
    B, D = 8, 16
    i = R.make_inputs(B, D)
    i = dict(i, mu=i["mu"] * 0.1, lv=i["lv"] * 0.1)               # K[d] far under 4
    assert float(R.kl_per_dim(i["mu"].double(), i["lv"].double()).max()) < 1.0
    f = _forward(H, i, 0.5 * D, 0.5)
    out4 = f["out4"].cpu()
    assert float(out4[0]) == 0.0 and float(out4[2]) == 64.0 and float(out4[3]) == 0.0
    assert float(f["gate"].abs().max()) == 0.0
    gmu, glv = _backward(H, f, 0.5 * D, 0.5, None, torch.full((), GLOSS, device="cuda"))
    assert float(gmu.abs().max()) == 0.0 and float(glv.abs().max()) == 0.0


# ------------------------------------------------------------------ 5. the sign alone
def test_the_capacity_s_side_only_flips_the_sign(H):
    i = R.make_inputs(64, 128)
    gloss = torch.full((), GLOSS, device="cuda")
    lo, hi = _forward(H, i, 0.0, 0.05), _forward(H, i, 1e6, 0.05)
    assert torch.equal(lo["gate"], -hi["gate"]) and float(lo["gate"].max()) == 1.0 and float(lo["gate"].min()) == 0.0
    (amu, alv), (bmu, blv) = _backward(H, lo, 0.0, 0.05, None, gloss), _backward(H, hi, 1e6, 0.05, None, gloss)
    nz = amu != 0                                                 # (a floored dimension's zero has no sign to flip)
    assert bool(nz.any()) and torch.equal(_bits(amu[nz]), _bits(-bmu[nz])) and torch.equal(amu, -bmu)
    nz = alv != 0
    assert bool(nz.any()) and torch.equal(_bits(alv[nz]), _bits(-blv[nz])) and torch.equal(alv, -blv)


# ------------------------------------------------------------------ 6. a dimension with no KL at all
def test_a_dead_dimension_is_not_above_a_zero_floor(H):
    i = dict(R.make_inputs(17, 65))
    i["mu"], i["lv"] = i["mu"].clone(), i["lv"].clone()
    i["mu"][:, 9] = 0.0
    i["lv"][:, 9] = 0.0
    f = _forward(H, i, 0.0, 0.0)
    assert float(f["kl_dim"][9]) == 0.0 and float(f["gate"][9]) == 0.0      # K[d] == 0 is not > 0
    assert float(f["out4"][3]) == 64.0
    gmu, glv = _backward(H, f, 0.0, 0.0, None, torch.full((), GLOSS, device="cuda"))
    assert float(gmu[:, 9].abs().max()) == 0.0 and float(glv[:, 9].abs().max()) == 0.0
    assert float(gmu[:, 10].abs().max()) > 0.0


# ------------------------------------------------------------------ 7. a NaN stays a NaN
def test_a_nan_goes_through_the_floor(H):
    i = dict(R.make_inputs(17, 65))
    i["mu"] = i["mu"].clone()
    i["mu"][3, 5] = float("nan")
    f = _forward(H, i, 1.0, 0.05)
    out4 = f["out4"].cpu()
    assert all(math.isnan(float(out4[n])) for n in range(3)), out4
    assert math.isnan(float(f["kl_dim"][5])) and math.isnan(float(f["gate"][5]))
    gmu, _ = _backward(H, f, 1.0, 0.05, None, torch.full((), GLOSS, device="cuda"))
    assert bool(torch.isnan(gmu[:, 5]).all())


# ------------------------------------------------------------------ 8. floats / device words; run to run
@pytest.mark.parametrize("shape", [(5, 7), (128, 128), (130, 200)], ids=str)
def test_device_words_and_repeated_runs_give_the_same_bits(H, shape):
    i = R.make_inputs(*shape)
    lam = 0.05
    C = float(torch.tensor(R.capacity_of(i, (0.5, lam)), dtype=torch.float32))      # an fp32 value: the same in both forms
    bw = torch.full((1,), R.BETA, dtype=torch.float32, device="cuda")
    cw = torch.full((1,), C, dtype=torch.float32, device="cuda")
    gz, gloss = i["gz"].cuda(), torch.full((), GLOSS, device="cuda")
    runs = []
    for beta, cap in ((R.BETA, C), (bw, cw), (R.BETA, C)):
        f = _forward(H, i, cap, lam, beta=beta)
        gmu, glv = _backward(H, f, cap, lam, gz, gloss, beta=beta)
        runs.append([f["z"], f["out4"], f["gate"], f["kl_dim"], gmu, glv])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(_bits(a), _bits(b))
    cw.fill_(4.0 * C)                                             # the word is read at every launch: now above the total
    f = _forward(H, i, cw, lam, beta=bw)
    assert not torch.equal(f["out4"][0], runs[0][1][0]) and torch.equal(_bits(f["out4"][1:]), _bits(runs[0][1][1:]))
    assert torch.equal(f["gate"], -runs[0][2])
    with pytest.raises(TypeError, match="both"):
        _forward(H, i, C, lam, beta=bw)
    with pytest.raises(TypeError, match="both"):
        _forward(H, i, cw, lam, beta=R.BETA)
    with pytest.raises(RuntimeError, match="one fp32 element"):
        _forward(H, i, torch.ones(2, device="cuda"), lam, beta=bw)


# ------------------------------------------------------------------ 9. autograd plumbing
def test_function_equals_the_direct_calls_and_the_parts_take_no_gradient(H):
    from disentangle_mlp_amd import functional as Fn
    i = R.make_inputs(17, 65)
    lam = 0.05
    C = R.capacity_of(i, (0.5, lam))
    f = _forward(H, i, C, lam)
    gz = i["gz"].cuda()
    mu, lv = f["mu"].clone().requires_grad_(True), f["lv"].clone().requires_grad_(True)
    z, loss, parts, kl_dim = Fn.reparam_klc_dims(mu, lv, f["eps"], R.BETA, C, lam)
    assert loss.requires_grad and z.requires_grad and not parts.requires_grad and parts.shape == (3,)
    assert not kl_dim.requires_grad and torch.equal(_bits(kl_dim), _bits(f["kl_dim"]))
    assert torch.equal(_bits(z), _bits(f["z"])) and torch.equal(_bits(loss), _bits(f["out4"][0]))
    assert torch.equal(_bits(parts), _bits(f["out4"][1:]))
    (GLOSS * loss + (z * gz).sum()).backward()
    gmu, glv = _backward(H, f, C, lam, gz, torch.full((), GLOSS, device="cuda"))
    assert torch.equal(_bits(mu.grad), _bits(gmu)) and torch.equal(_bits(lv.grad), _bits(glv))
    # one output alone: the other term is absent, not zero-filled
    for use, (a, b) in (("loss", (None, torch.ones((), device="cuda"))), ("z", (gz, None))):
        mu.grad = lv.grad = None
        out = Fn.reparam_klc(mu, lv, f["eps"], R.BETA, C, lam)
        assert len(out) == 3
        z, loss, _ = out
        (loss if use == "loss" else (z * gz).sum()).backward()
        gmu, glv = _backward(H, f, C, lam, a, b)
        assert torch.equal(_bits(mu.grad), _bits(gmu)) and torch.equal(_bits(lv.grad), _bits(glv)), use
    # beta and the capacity as tensors are the words themselves
    bw = torch.full((1,), R.BETA, device="cuda")
    cw = torch.full((1,), float(torch.tensor(C, dtype=torch.float32)), device="cuda")
    z, loss, _ = Fn.reparam_klc(mu, lv, f["eps"], bw, cw, lam)
    assert torch.equal(_bits(loss), _bits(_forward(H, i, float(cw), lam)["out4"][0]))


# ------------------------------------------------------------------ 10. VAETrainer
def _same_outputs_and_weights(ta, tb, oa, ob, what):
    from test_grad_clip_trainer_gpu import _assert_same, _weights
    assert oa.keys() == ob.keys()
    for k in oa:
        assert torch.equal(_bits(oa[k].float()), _bits(ob[k].float())), (what, k)
    _assert_same(_weights(ta), _weights(tb))


def test_vae_trainer_step_against_the_fp64_oracle():
    from disentangle_mlp_amd import trainer as T
    from oracle import modules as omod, steps as osteps
    beta, lam = 6.0, 0.05
    b = osteps.synthetic_batch(8)
    names, C = None, None
    ref = {}
    for dt in (torch.float64, torch.float32):
        torch.manual_seed(999)                                    # VAETrainer's recipe: the VAE alone (new_vae.py:33-37)
        net = omod.VAE(omod.OracleOpt())
        net.apply(omod.weights_init)
        net = net.to(dt)
        net.train()
        data, eps = b["data"].to(dt), b["eps2"].to(dt)
        mu, logvar = net.encode(data)
        if C is None:                                             # half the fp64 reference's kl_floored / B: far from a tie
            C = 0.5 * float(R.objective(mu.detach(), logvar.detach(), beta, 0.0, lam)["kl_floored"]) / 8
        z = net.reparameterize(mu, logvar, eps)
        mse = osteps.recon_loss(net.decode(z), data)
        o = R.objective(mu, logvar, beta, C, lam)
        (mse + o["loss"]).backward()
        names = [k for k, _ in net.named_parameters() if k not in BN_SHADOWED["eg"]]
        gn = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for k, p in net.named_parameters() if k in names))
        ref[dt] = dict(mse=mse.item(), kld=o["loss"].item(), kl=o["kl"].item(), kl_floored=o["kl_floored"].item(),
                       dims_above=float(o["dims_above"]), gradnorm=gn)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    print(f"capacity {C:.8g}  dims above the floor {r64['dims_above']:g}")
    tr = T.VAETrainer(beta=beta, kl_control=(C, lam))
    seen = {}

    def hook(phase, net):
        seen[phase] = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for k, p in net.named_parameters() if k in names))

    out = tr.step(b["data"].cuda(), b["eps2"].cuda(), grad_hook=hook)
    assert set(out) == {"mse", "kld", "kl", "kl_floored", "dims_above"}
    for k in out:
        tol = max(LOSS_TOL["mse" if k == "mse" else "kld"], 5 * gap(r32[k], r64[k]))
        print(f"{k}: {float(out[k]):.8g}  oracle fp64 {r64[k]:.8g}  fp32 {r32[k]:.8g}  tol {tol:.1e}")
        assert gap(float(out[k]), r64[k]) <= tol, (k, float(out[k]), r64[k])
    # the step differentiates at the initial weights, as phase "D" does: no optimizer step in front of it
    tol = max(GRADNORM_TOL["D"], 5 * gap(r32["gradnorm"], r64["gradnorm"]))
    print(f"gradient norm: {seen['VAE']:.8g}  oracle fp64 {r64['gradnorm']:.8g}  fp32 {r32['gradnorm']:.8g}  tol {tol:.1e}")
    assert gap(seen["VAE"], r64["gradnorm"]) <= tol


# ------------------------------------------------------------------ 11. captured = eager
def test_vae_trainer_captured_steps_equal_eager_steps():
    from disentangle_mlp_amd import trainer as T
    from test_grad_clip_trainer_gpu import _batch
    x, lat = _batch(8)
    kw = dict(beta=6.0, kl_control=(3.0, 0.05))
    tg, te = T.VAETrainer(graph=True, capturable=True, **kw), T.VAETrainer(graph=False, **kw)
    for it in range(4):
        og = {k: v.clone() for k, v in tg.step(x, lat[0]).items()}
        oe = {k: v.clone() for k, v in te.step(x, lat[0]).items()}
        assert len(oe) == 5
        _same_outputs_and_weights(tg, te, og, oe, it)
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs


# ------------------------------------------------------------------ 12. BetaVAEGANTrainer, the capacity on a schedule
def test_vaegan_trainer_with_an_annealed_capacity_replays_one_graph():
    from disentangle_mlp_amd import trainer as T
    from test_grad_clip_trainer_gpu import _batch
    x, lat = _batch()
    count = {"n": 0}
    real = T._CapturedIteration.replay

    def replay(self, *args, **kw):
        count["n"] += 1
        return real(self, *args, **kw)

    schedule = T.linear_capacity(25.0, 4)
    kw = dict(kl_control=(schedule, 0.05))
    tg, te = T.BetaVAEGANTrainer(graph=True, **kw), T.BetaVAEGANTrainer(graph=False, **kw)
    assert tg.device_hyper and not te.device_hyper                # on by default where the optimizers can carry the word:
    #                                                               the eager trainer passes floats -- the same bits
    T._CapturedIteration.replay = replay
    try:
        for it in range(6):
            og = {k: v.clone() for k, v in tg.step(x, *lat).items()}
            oe = {k: v.clone() for k, v in te.step(x, *lat).items()}
            assert set(oe) == {"errD_real", "errD_fake", "D_x_sum", "errG_fake", "errG_recon", "sim", "mse_dec", "kld",
                               "mse_enc", "kl", "kl_floored", "dims_above"}
            _same_outputs_and_weights(tg, te, og, oe, it)
            assert tg.capacity == te.capacity == schedule(it) == min(6.25 * it, 25.0)
    finally:
        T._CapturedIteration.replay = real
    assert len(tg._graphs) == 1 and tg.graph and not te._graphs
    assert count["n"] == 4                                        # every iteration after the two warm-up ones
    assert set(tg.checkpoint(0)) == set(T.BetaVAEGANTrainer(graph=False).checkpoint(0)) | {"iteration"}
    # the weighted loss is what the parts say, with that iteration's capacity
    # (four fp32 roundings -- of the part, of the capacity's word and of the loss, formed in fp64 -- relative to the terms' magnitudes)
    B = x.shape[0]
    terms = [tg.beta * float(og["kl_floored"]), tg.beta * B * schedule(5)]
    assert abs(float(og["kld"]) - abs(terms[0] - terms[1])) <= 4 * 2.0 ** -24 * (sum(terms) + abs(float(og["kld"])))


# ------------------------------------------------------------------ 13. the option left off
def test_without_the_option_the_trainers_are_what_they_were(monkeypatch):
    from disentangle_mlp_amd import model as M, ops, trainer as T
    from test_grad_clip_trainer_gpu import _batch

    def never(*a, **k):
        raise AssertionError("the KL-capacity objective ran without kl_control")

    monkeypatch.setattr(M.VAE, "forward_with_klc", never)
    monkeypatch.setattr(ops, "reparam_klc_fwd", never)
    x, lat = _batch()
    for cls, args, keys in ((T.BetaVAEGANTrainer, (x, *lat), 9), (T.VAETrainer, (x, lat[0]), 2)):
        for graph, steps in ((True, 3), (False, 1)):              # (the third step of a shape is the captured one)
            a, b = cls(graph=graph), cls(graph=graph, kl_control=None)      # the parent's signature / the new argument at its default
            for it in range(steps):
                oa = {k: v.clone() for k, v in a.step(*args).items()}
                ob = {k: v.clone() for k, v in b.step(*args).items()}
                assert len(oa) == keys
                _same_outputs_and_weights(a, b, oa, ob, (cls.__name__, graph, it))
            assert len(a._graphs) == len(b._graphs) == (1 if graph else 0)
            assert set(a.checkpoint(0)) == set(b.checkpoint(0))
            assert b.kl_control is None and b.capacity is None and not b.device_hyper
