"""CPU: the C ABI of the KL-capacity / free-bits kernels (vg_reparam_klc_*: declared, bound, exported, arguments validated
before any launch, in the float and the ``_dev`` forms), `ops.reparam_klc_fwd` / `functional.reparam_klc` without a CPU
path, `linear_capacity`, the trainers' argument checks, keys and checkpoints, and the torch restatement the GPU tests
compare against (tests/_klc_refs.py) checked against itself: the gate formula against autograd, the margin that lets every
dimension's gate be compared, and the fp32 evaluation against the fp64 one."""
import ctypes

import pytest
import torch

import _klc_refs as R
from test_cabi_cpu import declared_symbols

NEW = ["vg_reparam_klc_bwd", "vg_reparam_klc_bwd_dev", "vg_reparam_klc_fwd", "vg_reparam_klc_fwd_dev",
       "vg_reparam_klc_workspace_bytes"]
INF, NAN = float("inf"), float("nan")


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
    assert lib.vg_reparam_klc_workspace_bytes(128, 128) > 0 and lib.vg_reparam_klc_workspace_bytes(1024, 1024) > 0
    assert lib.vg_reparam_klc_workspace_bytes(0, 128) == 0 and lib.vg_reparam_klc_workspace_bytes(128, 1025) == 0


def _fwd_args(B=4, D=8, **over):
    """Host addresses standing in for device pointers: every call below must return before a launch."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    a = dict(mu=p, lv=p, eps=p, z=p, out4=p, gate=p, kl_dim=p, B=B, D=D, beta=6.0, capacity=2.0, free_bits=0.05, ws=p,
             ws_bytes=1 << 30, stream=None)
    a.update(over)
    return buf, a


def _bwd_args(B=4, D=8, **over):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    a = dict(gz=p, mu=p, lv=p, eps=p, gate=p, gloss=p, beta=6.0, capacity=2.0, free_bits=0.05, gmu=p, glv=p, B=B, D=D, ws=p,
             ws_bytes=1 << 30, stream=None)
    a.update(over)
    return buf, a


_ids = dict(ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
_SHARED = [dict(mu=None), dict(lv=None), dict(eps=None), dict(ws=None), dict(B=0), dict(B=1025), dict(D=0), dict(D=1025),
           dict(free_bits=-1.0), dict(free_bits=INF), dict(free_bits=NAN), dict(capacity=-1.0), dict(capacity=INF),
           dict(capacity=NAN), dict(ws_bytes="short"), dict(beta=None), dict(capacity=None)]


def _refused_by_both_forms(lib, fn, fn_dev, args, over):
    """``over``: a float capacity belongs to the float entry alone, a NULL word to the ``_dev`` entry alone; everything
    else is refused by both."""
    over = dict(over)
    if over.get("ws_bytes") == "short":
        over["ws_bytes"] = lib.vg_reparam_klc_workspace_bytes(4, 8) - 1
    keep, a = args(**over)
    null = [k for k in ("beta", "capacity") if k in over and over[k] is None]
    if not null:
        assert fn(*a.values()) == -1
        if "capacity" in over:                                    # (the value IN a word is not the host's to check)
            return
    a.update({k: None if k in null else ctypes.addressof(keep) for k in ("beta", "capacity")})
    assert fn_dev(*a.values()) == -1


@pytest.mark.parametrize("over", _SHARED + [dict(z=None), dict(out4=None), dict(gate=None), dict(kl_dim=None)], **_ids)
def test_forward_rejects_bad_arguments_before_any_launch(lib, over):
    _refused_by_both_forms(lib, lib.vg_reparam_klc_fwd, lib.vg_reparam_klc_fwd_dev, _fwd_args, over)


@pytest.mark.parametrize("over", _SHARED + [dict(gate=None), dict(gmu=None), dict(glv=None)], **_ids)
def test_backward_rejects_bad_arguments_before_any_launch(lib, over):
    _refused_by_both_forms(lib, lib.vg_reparam_klc_bwd, lib.vg_reparam_klc_bwd_dev, _bwd_args, over)


def test_ops_and_functional_refuse_cpu_tensors(lib):
    from disentangle_mlp_amd import functional as F, ops
    t = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reparam_klc_fwd(t, t, t, 6.0, 2.0, 0.05)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reparam_klc_bwd(None, t, t, t, t[0], None, 6.0, 2.0, 0.05)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.reparam_klc(t, t, t, 6.0, 2.0, 0.05)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.reparam_klc_dims(t, t, t, 6.0)
    with pytest.raises(ValueError, match="free_bits"):
        F.reparam_klc(t, t, t, 6.0, 2.0, -0.05)


def test_linear_capacity():
    from disentangle_mlp_amd import trainer as T
    c = T.linear_capacity(25.0, 100000)
    assert [c(0), c(50000), c(100000), c(250000)] == [0.0, 12.5, 25.0, 25.0]
    c = T.linear_capacity(25.0, 4, c_start=5.0)
    assert [c(0), c(1), c(2), c(4), c(5)] == [5.0, 10.0, 15.0, 25.0, 25.0]
    for bad in ((-1.0, 4), (NAN, 4), (INF, 4), (25.0, 0), (25.0, 2.5)):
        with pytest.raises(ValueError, match="linear_capacity"):
            T.linear_capacity(*bad)
    with pytest.raises(ValueError, match="linear_capacity"):
        T.linear_capacity(25.0, 4, c_start=-1.0)


def test_trainer_arguments():
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(TypeError, match="GANTrainer has no KL term: kl_control does not apply"):
        T.GANTrainer(device="cpu", kl_control=(2.0, 0.05))
    for bad in (2.0, (2.0,), (2.0, 0.05, 1.0), ("c", 0.05), (2.0, "f"), (2.0, None)):
        with pytest.raises(TypeError, match="kl_control"):
            T.VAETrainer(device="cpu", kl_control=bad)
    for bad in ((-1.0, 0.05), (INF, 0.05), (NAN, 0.05), (2.0, -0.05), (2.0, INF), (2.0, NAN), (lambda it: -1.0, 0.05)):
        with pytest.raises(ValueError, match="kl_control"):
            T.VAETrainer(device="cpu", kl_control=bad)
    others = dict(tc_decomposition=(1.0, 1.0), dip_vae=("i", 10.0, 100.0), mmd_vae=("imq", 100.0))
    for cls in (T.VAETrainer, T.BetaVAEGANTrainer):
        for k, v in others.items():
            with pytest.raises(ValueError, match=f"each replace the KL term.*got kl_control and {k}"):
                cls(device="cpu", kl_control=(2.0, 0.05), dataset_size=100, **{k: v})
    plain, keyed = T.VAETrainer(device="cpu"), T.VAETrainer(device="cpu", kl_control=(2, 0.05))
    assert plain.kl_control is None and plain.capacity is None
    assert keyed.kl_control == (2.0, 0.05) and keyed.capacity == 2.0
    assert keyed.tc_decomposition is None and keyed.dip_vae is None and keyed.mmd_vae is None
    with pytest.raises(AttributeError):
        keyed.kl_control = (3.0, 0.05)                            # a view: `set_capacity` is the way
    with pytest.raises(TypeError, match="kl_control"):
        plain.set_capacity(1.0)
    keyed.set_capacity(3)
    assert keyed.capacity == 3.0 and keyed.kl_control == (3.0, 0.05)
    with pytest.raises(ValueError, match="capacity"):
        keyed.set_capacity(-1.0)
    # free_bits is a frozen kernel argument; the capacity is none of `_host_state_key`'s
    keys = {plain._host_state_key(), keyed._host_state_key(), T.VAETrainer(device="cpu", kl_control=(2, 0.1))._host_state_key()}
    assert len(keys) == 3
    assert T.VAETrainer(device="cpu", kl_control=(7, 0.05))._host_state_key() == keyed._host_state_key()
    assert T.BetaVAEGANTrainer(device="cpu", kl_control=(25, 0)).kl_control == (25.0, 0.0)
    # the latents are the trainer's own
    assert keyed._latents == plain._latents == ("eps",)
    assert T.BetaVAEGANTrainer(device="cpu", kl_control=(25, 0))._latents == ("noise", "eps2", "eps3")


def test_checkpoint_keys_and_schedule():
    from disentangle_mlp_amd import trainer as T
    plain = T.VAETrainer(device="cpu")
    const = T.VAETrainer(device="cpu", kl_control=(2.0, 0.05))
    sched = T.VAETrainer(device="cpu", kl_control=(T.linear_capacity(25.0, 4), 0.05))
    assert set(const.checkpoint(0)) == set(plain.checkpoint(0))              # a constant capacity adds no key
    assert set(sched.checkpoint(0)) == set(plain.checkpoint(0)) | {"iteration"}
    assert sched.capacity == 0.0 and not sched.device_hyper                  # (a CPU trainer's optimizers cannot carry the word)
    sched.iteration = 3                                                      # restoring: the last step's value, as beta's
    ck = sched.checkpoint(0)
    other = T.VAETrainer(device="cpu", kl_control=(T.linear_capacity(25.0, 4), 0.05))
    other._schedule_restore(ck)
    assert other.iteration == 3 and other.capacity == 12.5
    sched._begin_step()                                                      # the start of a step evaluates the schedule
    assert sched.capacity == 18.75


def test_capture_key_holds_the_capacity_only_without_device_hyper():
    from disentangle_mlp_amd import trainer as T
    data = torch.zeros(8, 3, 64, 64)
    t = T.VAETrainer(device="cpu", kl_control=(2.0, 0.05))
    t.optimizer.state_generation = 0                              # (HipAdam's: torch.optim.Adam, a CPU trainer's, has none)
    k2 = t._capture_key(data, None)
    t.set_capacity(3.0)
    assert t._capture_key(data, None) != k2                       # a frozen value, as beta
    t.set_capacity(2.0)
    assert t._capture_key(data, None) == k2
    t.device_hyper = True                                         # (the key alone: the words need a GPU)
    k2 = t._capture_key(data, None)
    t.set_capacity(3.0)
    assert t._capture_key(data, None) == k2                       # in a device word: one capture for every value
    plain = T.VAETrainer(device="cpu")                            # without the option the frozen tuple is what it was
    plain.optimizer.state_generation = 0
    assert plain._capture_key(data, None)[2] == (plain.beta, plain.optimizer.param_groups[0]["lr"])


# ---- the restatement against itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=str)
@pytest.mark.parametrize("shape", [(5, 7), (17, 65), (130, 200)], ids=str)
def test_closed_form_gradient_is_autograd_s(shape, case):
    i = R.make_inputs(*shape)
    C = R.capacity_of(i, case)
    ref = R.reparam_klc(i["mu"], i["lv"], i["eps"], R.BETA, C, case[1])
    gmu, glv = R.closed_form_grads(i["mu"], i["lv"], R.BETA, C, case[1])
    assert float(ref["gmu_loss"].abs().max()) > 0.0
    assert R.rel_err(gmu, ref["gmu_loss"]) <= 1e-12 and R.rel_err(glv, ref["glv_loss"]) <= 1e-12
    assert set(ref["gate"].tolist()) <= {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("shape", R.SHAPES + [(1024, 1024)], ids=str)
def test_no_dimension_sits_on_its_floor(shape):
    """Not a tolerance: the condition under which the GPU tests compare EVERY dimension's gate exactly.  Smallest margin
    over all shapes: 9.4e-3, at (256, 128); 44 of 128 dimensions are above the floor at (128, 128), 352 of 1024 at
    (1024, 1024)."""
    i = R.make_inputs(*shape)
    for lam in sorted({c[1] for c in R.CASES}):
        m = R.margin(i["mu"], i["lv"], lam)
        print(f"{shape} lambda {lam}: margin {m:.3e}")
        assert m > R.MARGIN, (shape, lam, m)
    above = {(128, 128): 44, (1024, 1024): 352}.get(shape)
    if above is not None:
        assert int(R.objective(i["mu"].double(), i["lv"].double(), R.BETA, 0.0, 0.05)["dims_above"]) == above


@pytest.mark.parametrize("case", R.CASES, ids=str)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_fp32_restatement_is_a_usable_yardstick(shape, case):
    """The bound of the GPU tests is 5 x the fp32 restatement's own error (floor 1e-6): on these inputs the restatement
    picks the same gate everywhere and its error stays under 1e-5 for every compared tensor (largest seen: 2.3e-7), far
    from the 1e-3 a wrong term would show."""
    i = R.make_inputs(*shape)
    C = R.capacity_of(i, case)
    r64 = R.reparam_klc(i["mu"], i["lv"], i["eps"], R.BETA, C, case[1])
    r32 = R.reparam_klc(i["mu"], i["lv"], i["eps"], R.BETA, C, case[1], dtype=torch.float32)
    assert torch.equal(r32["gate"].double(), r64["gate"]) and int(r32["dims_above"]) == int(r64["dims_above"])
    for k in R.COMPARED:
        assert R.rel_err(r32[k], r64[k]) <= 1e-5, (k, R.rel_err(r32[k], r64[k]))
