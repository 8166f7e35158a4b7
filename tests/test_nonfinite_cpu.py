"""CPU: the non-finite guard's host side -- the two checked Adam entry points of the C ABI (exported, bound, validating
before any launch), `check_finite` / `NonFiniteError` on trainers whose optimizer is torch's (the ``torch.isfinite``
path), the checkpoint a poisoned epoch must not write, the data-parallel agreement (every rank raises), and the
switches (``nonfinite_guard=``, VG_NONFINITE_GUARD, the capture key)."""
import ctypes
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from disentangle_mlp_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_checked_entry_points_are_exported_bound_and_validate_on_the_host(lib):
    from disentangle_mlp_amd import _lib
    from disentangle_mlp_amd.optim import _AdamTensor
    assert _lib.ABI_VERSION == 7 == lib.vg_version()
    for name in ("vg_adam_step_checked", "vg_adam_step_dev_checked"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the bindings are the unchecked ones plus the host array of device words, in front of the stream
    assert _lib.SIGNATURES["vg_adam_step_checked"][1] == _lib.SIGNATURES["vg_adam_step"][1][:-1] + [ctypes.c_void_p] * 2
    assert _lib.SIGNATURES["vg_adam_step_dev_checked"][1] == _lib.SIGNATURES["vg_adam_step_dev"][1][:-1] + [ctypes.c_void_p] * 2
    arr = (_AdamTensor * 1)()
    flags = (ctypes.c_void_p * 1)()
    # the same rejections as the unchecked entries, with a flag array and with NULL: VG_ERR_BAD_ARG before any launch
    for fl in (None, flags):
        assert lib.vg_adam_step(arr, -1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, None) == -1
        assert lib.vg_adam_step_checked(arr, -1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, fl, None) == -1
        assert lib.vg_adam_step(None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, None) == -1
        assert lib.vg_adam_step_checked(None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, fl, None) == -1
        assert lib.vg_adam_step(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.03, None) == -1
        assert lib.vg_adam_step_checked(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.03, fl, None) == -1        # bias_correction1
        assert lib.vg_adam_step_checked(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, float("nan"), fl, None) == -1
        assert lib.vg_adam_step_dev(arr, -1, 0.9, 0.999, 1e-8, None, None) == -1
        assert lib.vg_adam_step_dev_checked(arr, -1, 0.9, 0.999, 1e-8, None, fl, None) == -1
        assert lib.vg_adam_step_dev(arr, 1, 0.9, 0.999, 1e-8, None, None) == -1                            # no scalars
        assert lib.vg_adam_step_dev_checked(arr, 1, 0.9, 0.999, 1e-8, None, fl, None) == -1
        # a tensor with elements but a NULL pointer: rejected while the launch is being put together
        arr[0] = _AdamTensor(None, None, None, None, 16, None)
        assert lib.vg_adam_step_checked(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, fl, None) == -1
        arr[0] = _AdamTensor(None, None, None, None, 0, None)
        # nothing to do -- no tensors, or only empty ones (skipped, their flag untouched): success, no launch
        assert lib.vg_adam_step_checked(None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, fl, None) == 0
        assert lib.vg_adam_step_checked(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, fl, None) == 0


def _named(tr):
    return {f"{a}.{k}": p for a, net, _ in tr._guarded_optimizers() for k, p in net.named_parameters()}


def test_check_finite_names_exactly_the_poisoned_parameter():
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer, GANTrainer, NonFiniteError, VAETrainer
    assert issubclass(NonFiniteError, RuntimeError)
    for make, name in ((lambda: BetaVAEGANTrainer(device="cpu"), "netD.convs.3.weight"),
                       (lambda: VAETrainer(device="cpu"), "model.deconv2.weight"),
                       (lambda: GANTrainer(device="cpu"), "netG.deconv1.weight")):
        tr = make()
        assert tr.check_finite() is None                       # clean
        params = _named(tr)
        with torch.no_grad():
            params[name].view(-1)[5] = float("nan")
        with pytest.raises(NonFiniteError) as e:
            tr.check_finite()
        assert e.value.found == [(name, "param")]
        assert (e.value.first_iteration, e.value.last_iteration) == (0, 0)
        msg = str(e.value)
        assert name in msg and "input batch" in msg and "fp16x3" in msg and "checkpoint" in msg
        # a non-finite gradient next to a finite parameter / both
        other = next(k for k in params if k != name)
        params[other].grad = torch.full_like(params[other], float("inf"))
        params[name].grad = torch.zeros_like(params[name])
        params[name].grad.view(-1)[0] = float("-inf")
        with pytest.raises(NonFiniteError) as e:
            tr.check_finite()
        assert sorted(e.value.found) == sorted([(name, "grad+param"), (other, "grad")])
        with torch.no_grad():
            params[name].view(-1)[5] = 0.0
        params[name].grad = params[other].grad = None
        assert tr.check_finite() is None


class _Loader:
    def __init__(self, batches, n):
        self.batches, self.dataset = batches, list(range(n))
        self.last_global_batch = None

    def __iter__(self):
        for b in self.batches:
            self.last_global_batch = b.size(0)
            yield b, None


def _stub_step(tr):
    """The kernels need a GPU: `step` only counts (the guard's CPU path looks at parameters and gradients)."""
    def fake_step(data, real_label=None, fake_label=None, global_batch=None, **kw):
        tr.iteration += 1
        z = torch.tensor(0.0)
        return {"mse_enc": z, "D_x_sum": z, "errG": z, "errD_real": z, "errD_fake": z, "mse": z, "kld": z}
    tr.step = fake_step


def test_fit_writes_no_checkpoint_of_a_poisoned_epoch(tmp_path):
    from disentangle_mlp_amd.trainer import BetaVAEGANTrainer, NonFiniteError
    loader = _Loader([torch.zeros(2, 3, 64, 64)] * 3, n=6)
    good, bad = tmp_path / "good", tmp_path / "bad"
    good.mkdir(), bad.mkdir()
    tr = BetaVAEGANTrainer(device="cpu", nonfinite_guard=True)
    _stub_step(tr)
    tr.fit(loader, epochs=1, model_path=str(good), verbose=False)
    assert sorted(os.listdir(good)) == ["model_1.tar"]          # the clean epoch is saved as before
    with torch.no_grad():
        tr.netEG.deconv4.weight.view(-1)[-1] = float("nan")
    with pytest.raises(NonFiniteError) as e:
        tr.fit(loader, epochs=2, start_epoch=1, model_path=str(bad), verbose=False)
    assert e.value.found == [("netEG.deconv4.weight", "param")]
    assert (e.value.first_iteration, e.value.last_iteration) == (3, 6)     # clean at the end of epoch 0; three more steps
    assert os.listdir(bad) == []                                # no .tar (nor anything else) of the poisoned epoch
    # the recovery: a good checkpoint loaded -- the range starts afresh
    tr.load(torch.load(good / "model_1.tar", weights_only=False))
    assert tr.check_finite() is None
    # the other two trainers' epochs raise alike
    from disentangle_mlp_amd.trainer import GANTrainer, VAETrainer
    for tr, p in ((VAETrainer(device="cpu", nonfinite_guard=True), lambda t: t.model.deconv4.weight),
                  (GANTrainer(device="cpu", nonfinite_guard=True), lambda t: t.netD.convs[0].weight)):
        _stub_step(tr)
        tr.train_epoch(loader)
        with torch.no_grad():
            p(tr).view(-1)[0] = float("inf")
        with pytest.raises(NonFiniteError):
            tr.train_epoch(loader)


def test_guard_switches_are_honoured():
    from disentangle_mlp_amd import trainer as T
    # None: on whenever the steps run on HipAdam; an explicit value wins
    default = os.environ.get("VG_NONFINITE_GUARD", "1") != "0"      # (the suite may itself run with the switch exported)
    assert T.NONFINITE_GUARD_DEFAULT is default
    res = T._GraphedSteps._resolve_guard
    assert res(None, True) is default and res(None, False) is False
    assert res(False, True) is False and res(True, False) is True
    # off: train_epoch does not look (check_finite on demand still does)
    loader = _Loader([torch.zeros(2, 3, 64, 64)], n=2)
    for guard, raises in ((False, False), (None, False), (True, True)):
        tr = T.BetaVAEGANTrainer(device="cpu", nonfinite_guard=guard)
        assert tr.nonfinite_guard is bool(guard)                # (a CPU trainer steps torch.optim.Adam)
        _stub_step(tr)
        with torch.no_grad():
            tr.netD.convs[0].weight.view(-1)[0] = float("nan")
        if raises:
            with pytest.raises(T.NonFiniteError):
                tr.train_epoch(loader)
        else:
            tr.train_epoch(loader)
        with pytest.raises(T.NonFiniteError):
            tr.check_finite()
    # the resolved value is part of what a capture freezes (checked or unchecked Adam launches)
    a, b = T.VAETrainer(device="cpu", nonfinite_guard=True), T.VAETrainer(device="cpu", nonfinite_guard=False)
    assert a._host_state_key() != b._host_state_key()
    assert a._host_state_key() == T.VAETrainer(device="cpu", nonfinite_guard=True)._host_state_key()


def test_guarded_epoch_returns_the_unguarded_epochs_values():
    """Guarded, the epoch's sums travel in the copy that reads the flag words: the values are the unguarded epoch's."""
    from disentangle_mlp_amd import trainer as T
    loader = _Loader([torch.zeros(4, 3, 64, 64)] * 3, n=12)

    def stub(tr):
        def fake_step(data, real_label=None, fake_label=None, global_batch=None, **kw):
            tr.iteration += 1
            i = float(tr.iteration)
            return {"mse_enc": torch.tensor(100.0 * i + 1 / 3), "D_x_sum": torch.tensor(0.7 * i), "errG": torch.tensor(2.5 * i),
                    "errD_real": torch.tensor(0.25), "errD_fake": torch.tensor(0.1 * i), "mse": torch.tensor(7.0 * i),
                    "kld": torch.tensor(1 / 7)}
        tr.step = fake_step
    for make in (T.BetaVAEGANTrainer, T.VAETrainer, T.GANTrainer):
        got = []
        for guard in (True, False):
            tr = make(device="cpu", nonfinite_guard=guard)
            stub(tr)
            kw = {} if make is T.VAETrainer else {"label_rng": __import__("numpy").random.RandomState(0)}
            got.append((tr.train_epoch(loader, **kw), getattr(tr, "last_epoch_sums", None)))
        assert got[0] == got[1], make.__name__
    assert got[0][1] is not None                                  # (GANTrainer's sums went the same way)


def test_environment_turns_the_default_off():
    code = ("from disentangle_mlp_amd import trainer as T; r = T._GraphedSteps._resolve_guard; "
            "print(T.NONFINITE_GUARD_DEFAULT, r(None, True), r(True, True), r(None, False))")
    for env, want in (("0", "False False True False"), ("1", "True True True False")):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, VG_NONFINITE_GUARD=env),
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip().splitlines()[-1] == want


def test_hip_adam_guard_on_the_torch_path_is_not_silently_clean():
    """CPU tensors take torch's step, which cannot flag: `nonfinite` then forms the bits with torch.isfinite."""
    from disentangle_mlp_amd.optim import HipAdam, NONFINITE_GRAD, NONFINITE_PARAM
    ps = [torch.nn.Parameter(torch.ones(5)) for _ in range(3)]
    opt = HipAdam(ps, lr=1e-2, nonfinite_guard=True)
    words = opt.nonfinite_words()
    assert words.dtype == torch.int32 and words.shape == (3,)
    for p in ps:
        p.grad = torch.ones(5)
    opt.step()
    assert opt.nonfinite() == {}
    ps[1].grad[2] = float("nan")
    opt.step()
    got = opt.nonfinite()
    assert len(got) == 1 and next(iter(got)) is ps[1]
    assert got[ps[1]] == NONFINITE_GRAD | NONFINITE_PARAM
    assert opt.nonfinite_words() is words                      # never replaced ...
    opt.load_state_dict(opt.state_dict())
    assert opt.nonfinite_words() is words                      # ... not by load_state_dict either
    with pytest.raises(RuntimeError, match="nonfinite_guard"):
        HipAdam([torch.nn.Parameter(torch.ones(2))]).nonfinite_words()
    with pytest.raises(RuntimeError, match="constructor"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(2))]})


# ------------------------------------------------------------------ data parallel: every rank raises
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _poisoned_rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from disentangle_mlp_amd.trainer import GANTrainer, NonFiniteError
    tr = GANTrainer(device="cpu", seed=999, nonfinite_guard=True)
    _stub_step(tr)
    loader = _Loader([torch.zeros(2, 3, 64, 64)] * 2, n=4 * world)
    seen = {"clean": tr.train_epoch(loader) is not None}
    if rank == 1:                                # only this rank is poisoned
        with torch.no_grad():
            tr.netG.deconv1.weight.view(-1)[7] = float("nan")
    try:
        tr.train_epoch(loader)
        seen["raised"] = False
    except NonFiniteError as e:
        seen.update(raised=True, found=e.found, range=(e.first_iteration, e.last_iteration), msg=str(e))
    q.put((rank, seen))
    dist.barrier()                               # nobody was left waiting in a collective
    dist.destroy_process_group()


def test_every_rank_raises_when_one_is_poisoned():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_poisoned_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert got[0]["clean"] and got[1]["clean"]
    assert got[0]["raised"] and got[1]["raised"]
    assert got[1]["found"] == [("netG.deconv1.weight", "param")]
    assert got[0]["found"] == [] and "another rank" in got[0]["msg"]
    assert got[0]["range"] == got[1]["range"] == (2, 4)
