"""CPU: the two host-side decisions of a ``HipAdam`` step -- which ``vg_adam_step*`` entry point a launch takes
(`optim.step_entry`) and which prepare kernel runs in front of it (`optim.prepare_entry`) -- over their whole truth tables.

Which entry point a step takes decides which kernel runs, plain or feature, so the expected names are written here on their
own, as the two priority lists, and compared with the function's answer row by row."""
import itertools

import pytest

HOST_PREFIX = 8      # arr, n, lr, beta1, beta2, eps, bc1, bc2_sqrt
DEV_PREFIX = 6       # arr, n, beta1, beta2, eps, scalars


def _rows():
    """(dev, flags, ema, ema_dev, decay, clip): the decay on the device needs an average and device scalars."""
    for row in itertools.product((False, True), repeat=6):
        dev, flags, ema, ema_dev, decay, clip = row
        if ema_dev and not (ema and dev):
            continue
        yield row


def _expected(dev, flags, ema, ema_dev, decay, clip):
    on_device = [(ema_dev, "vg_adam_step_dev_ema_dev"), (decay, "vg_adam_step_dev_decay"), (clip, "vg_adam_step_dev_clip"),
                 (ema, "vg_adam_step_dev_ema"), (flags, "vg_adam_step_dev_checked"), (True, "vg_adam_step_dev")]
    on_host = [(decay, "vg_adam_step_decay"), (clip, "vg_adam_step_clip"), (ema, "vg_adam_step_ema"),
               (flags, "vg_adam_step_checked"), (True, "vg_adam_step")]
    return next(name for on, name in (on_device if dev else on_host) if on)


def test_truth_table_size():
    assert len(list(_rows())) == 32 + 8      # of the 32 rows with ema_dev only the 8 with ema and dev remain


@pytest.mark.parametrize("row", list(_rows()), ids=lambda r: "".join("01"[b] for b in r))
def test_step_entry_follows_the_priority_lists(row):
    from disentangle_mlp_amd.optim import step_entry
    dev, flags, ema, ema_dev, decay, clip = row
    name, tail = step_entry(dev=dev, flags=flags, ema=ema, ema_dev=ema_dev, decay=decay, clip=clip)
    assert name == _expected(*row)


def test_every_entry_is_bound_and_its_tail_fits():
    """Every name the function returns is a key of `_lib.SIGNATURES`, and common prefix + tail + stream is the argument
    list the binding declares; all eleven step entry points are reachable."""
    from disentangle_mlp_amd import _lib
    from disentangle_mlp_amd.optim import step_entry
    seen = {}
    for dev, flags, ema, ema_dev, decay, clip in _rows():
        name, tail = step_entry(dev=dev, flags=flags, ema=ema, ema_dev=ema_dev, decay=decay, clip=clip)
        assert name in _lib.SIGNATURES
        assert seen.setdefault(name, (dev, tail)) == (dev, tail), f"{name}: one entry point, two argument lists"
        assert len(_lib.SIGNATURES[name][1]) == (DEV_PREFIX if dev else HOST_PREFIX) + len(tail) + 1, name
    assert set(seen) == {k for k in _lib.SIGNATURES if k.startswith("vg_adam_step")}
    assert len(seen) == 11


@pytest.mark.parametrize("row", list(itertools.product((False, True), repeat=4)), ids=lambda r: "".join("01"[b] for b in r))
def test_prepare_entry(row):
    """``vg_adam_prepare_dev`` whenever the step reads the hyper words; else ``vg_adam_prepare`` -- unless the fused half
    of the step has run it already."""
    from disentangle_mlp_amd.optim import prepare_entry
    device_hyper, decay, ema_dev, prepared = row
    if device_hyper or decay or ema_dev:
        want = "vg_adam_prepare_dev"
    elif prepared:
        want = None
    else:
        want = "vg_adam_prepare"
    assert prepare_entry(device_hyper=device_hyper, decay=decay, ema_dev=ema_dev, prepared=prepared) == want
