"""CPU: the host side of the trainer-driven weight EMA -- `trainer.ema_warmup` against its formula, the
``vg_adam_step_dev_ema_dev`` entry point of the C ABI (exported, bound, validating before any launch), the constructor
checks of ``HipAdam(ema_decay_on_device=True)`` and the trainers' refusal to average on torch.optim.Adam."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from disentangle_mlp_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("decay,start", [(0.999, 0), (0.999, 7), (0.5, 3), (0.05, 1)])
def test_ema_warmup_follows_its_formula(decay, start):
    from disentangle_mlp_amd.trainer import ema_warmup
    f = ema_warmup(decay, start)
    for it in sorted({0, max(start - 1, 0), start, start + 1, start + 8, 10 ** 6}):
        n = it - start
        want = 0.0 if n < 0 else min(decay, (1 + n) / (10 + n))
        assert f(it) == want, (it, f(it), want)
        assert 0.0 <= f(it) < 1.0
    if start:
        assert f(0) == 0.0 and f(start - 1) == 0.0                # the average follows the weights
    assert f(start) == min(decay, 0.1)
    assert f(10 ** 6) == decay                                    # the warm-up ends at the asked decay
    assert ema_warmup(decay)(0) == min(decay, 0.1)                # start_iteration defaults to 0


def test_ema_warmup_rejects_out_of_range_arguments():
    from disentangle_mlp_amd.trainer import ema_warmup
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            ema_warmup(bad)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="start_iteration"):
            ema_warmup(0.9, bad)


def test_entry_point_is_exported_bound_and_validates_on_the_host(lib):
    from disentangle_mlp_amd import _lib
    from disentangle_mlp_amd.optim import _AdamTensor
    name = "vg_adam_step_dev_ema_dev"
    assert _lib.ABI_VERSION == 7 == lib.vg_version()              # the entry point was only added: the version stays
    assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # vg_adam_step_dev_decay's signature with the host double replaced by a device pointer
    decay = _lib.SIGNATURES["vg_adam_step_dev_decay"][1]
    assert decay[8] is ctypes.c_double
    assert _lib.SIGNATURES[name][1] == decay[:8] + [ctypes.c_void_p] + decay[9:]
    arr = (_AdamTensor * 1)()
    arr[0] = _AdamTensor(None, None, None, None, 0, None)         # an empty tensor: skipped, nothing is launched
    ema = (ctypes.c_void_p * 1)()
    word = ctypes.c_void_p(64)                                    # never dereferenced on the host: every call returns first
    flags = (ctypes.c_void_p * 1)()

    def call(tensors, count, ema, omd, scal=word, fl=None, rec=None):
        return lib.vg_adam_step_dev_ema_dev(tensors, count, 0.9, 0.999, 1e-8, scal, fl, ema, omd, rec, None)

    for fl in (None, flags):
        for rec in (None, word):
            assert call(arr, 1, None, word, fl=fl, rec=rec) == -1     # NULL ema
            assert call(arr, 1, ema, None, fl=fl, rec=rec) == -1      # NULL ema_omd
            assert call(None, 0, None, word, fl=fl, rec=rec) == -1
            assert call(None, 0, ema, None, fl=fl, rec=rec) == -1
            assert call(None, 1, ema, word, fl=fl, rec=rec) == -1     # NULL tensors with count > 0
            assert call(arr, -1, ema, word, fl=fl, rec=rec) == -1
            assert call(arr, 1, ema, word, scal=None, fl=fl, rec=rec) == -1      # no scalars
            # nothing to do -- no tensors, or only empty ones: success, no launch
            assert call(None, 0, ema, word, fl=fl, rec=rec) == 0
            assert call(arr, 1, ema, word, fl=fl, rec=rec) == 0
    arr[0] = _AdamTensor(None, None, None, None, 16, None)        # elements but NULL pointers
    assert call(arr, 1, ema, word) == -1


def test_null_ema_is_a_bad_argument(lib):
    from disentangle_mlp_amd.optim import _AdamTensor
    arr = (_AdamTensor * 1)()
    arr[0] = _AdamTensor(None, None, None, None, 0, None)
    word = ctypes.c_void_p(64)
    assert lib.vg_adam_step_dev_ema_dev(arr, 1, 0.9, 0.999, 1e-8, word, None, None, word, None, None) == -1


def test_null_ema_omd_is_a_bad_argument(lib):
    from disentangle_mlp_amd.optim import _AdamTensor
    arr = (_AdamTensor * 1)()
    arr[0] = _AdamTensor(None, None, None, None, 0, None)
    word = ctypes.c_void_p(64)
    ema = (ctypes.c_void_p * 1)()
    assert lib.vg_adam_step_dev_ema_dev(arr, 1, 0.9, 0.999, 1e-8, word, None, ema, None, None, None) == -1


def test_hip_adam_device_decay_needs_capturable_and_a_decay():
    from disentangle_mlp_amd.optim import HipAdam

    def params():
        return [torch.nn.Parameter(torch.ones(4, 3)), torch.nn.Parameter(torch.ones(5))]
    with pytest.raises(ValueError, match="ema_decay_on_device=True.*requires capturable=True"):
        HipAdam(params(), ema_decay=0.9, ema_decay_on_device=True)
    with pytest.raises(ValueError, match="ema_decay_on_device"):
        HipAdam(params(), capturable=True, ema_decay_on_device=True)          # nothing to keep on the device
    # without the new argument nothing changes: the (0, 1) validation, and no way to move the decay
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"ema_decay must lie in \(0, 1\)"):
            HipAdam(params(), ema_decay=bad)
    opt = HipAdam(params(), ema_decay=0.9)
    with pytest.raises(RuntimeError, match="ema_decay_on_device"):
        opt.set_ema_decay(0.5)
    assert opt.ema_decay == 0.9 and opt._ema_omd is None and not opt._hyper
    with pytest.raises(RuntimeError, match="ema_decay"):
        HipAdam(params()).set_ema_decay(0.5)


@pytest.mark.parametrize("cls", ["BetaVAEGANTrainer", "VAETrainer", "GANTrainer"])
def test_cpu_trainer_refuses_to_average(cls):
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(ValueError, match=r"ema_decay.*HipAdam.*'cpu'"):
        getattr(T, cls)(device="cpu", ema_decay=0.999)
    with pytest.raises(ValueError, match=r"ema_decay.*HipAdam.*'cpu'"):
        getattr(T, cls)(device="cpu", ema_decay=T.ema_warmup(0.999, 2))


def test_cpu_trainer_without_ema_is_what_it_was():
    """The control: with ``ema_decay=None`` there is no shadow, no schedule and exactly the reference's checkpoint keys;
    asking such a trainer for its average names what is missing."""
    from disentangle_mlp_amd import trainer as T
    tr = T.BetaVAEGANTrainer(device="cpu", ema_decay=None)
    assert tr.ema_model is None and tr.ema_schedule is None
    assert set(tr.checkpoint(1)) == {"epoch", "encoder_decoder_model", "discriminator_model",
                                     "encoder_decoder_optimizer", "discriminator_optimizer"}
    for call in (tr.reset_ema, lambda: tr.recalibrate_ema_bn([]), lambda: tr.evaluate([], use_ema=True)):
        with pytest.raises(ValueError, match="ema_decay"):
            call()


def test_trainer_rejects_a_decay_out_of_range():
    from disentangle_mlp_amd import trainer as T
    with pytest.raises(ValueError, match=r"ema_decay must be a float in \(0, 1\)"):
        T.VAETrainer(device="cpu", ema_decay=1.0)
    with pytest.raises(ValueError, match=r"schedule must return a decay in \[0, 1\)"):
        T.GANTrainer(device="cpu", ema_decay=lambda it: 1.0)
