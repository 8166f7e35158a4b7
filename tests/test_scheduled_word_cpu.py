"""CPU: every ``_dev`` entry whose scheduled value is a `Word` (csrc/common.hpp) refuses a NULL word
with VG_ERR_BAD_ARG before any launch -- each of its words in turn, every other argument valid.  The check is stated once
(`words_ok`) and the launchers call it (reparam_mmd.hip, still a template on the form, has its own); this is the one place
that asks all of them.

CPU only, on purpose: with the check broken such a call would launch a kernel that reads address 0.  Without a GPU the
launch merely fails; nothing here may run under the ``gpu`` mark, and no call below has all its words set."""
import ctypes

import pytest

import test_reparam_dip_cpu as dip
import test_reparam_klc_cpu as klc
import test_reparam_mmd_cpu as mmd
import test_reparam_tc_cpu as tc

A = 4096      # a made-up, aligned address: every call below is refused on the host


@pytest.fixture(scope="module")
def lib():
    from disentangle_mlp_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _kl_fwd():
    return None, dict(mu=A, lv=A, eps=A, z=A, kl=A, rows=A, B=4, D=8, beta=A, stream=None)


def _kl_bwd():
    return None, dict(gz=A, mu=A, lv=A, eps=A, gkl=A, beta=A, gmu=A, glv=A, B=4, D=8, stream=None)


def _bce():
    return None, dict(p=A, target=A, loss=A, gp=A, B=8, divisor=8.0, gscale=1.0, stream=None)


def _factor_fwd():
    return None, dict(logits=A, kl=A, out4=A, B=8, beta=A, gamma=A, ws=None, ws_bytes=0, stream=None)


def _factor_bwd():
    return None, dict(gloss=A, beta=A, gamma=A, glogits=A, gkl=A, B=8, ws=None, ws_bytes=0, stream=None)


def _augment():
    return None, dict(x=A, u=A, y=2 * A, B=1, C=3, H=64, W=64, policy=7, p=4 * A, ws=3 * A, ws_bytes=256, stream=None)


# entry -> (its valid arguments -- an objective's are the sibling test's, of the float entry: the words' places still hold floats --, its words)
ENTRIES = {
    "vg_reparam_kl_fwd_dev": (_kl_fwd, ("beta",)),
    "vg_reparam_kl_bwd_dev": (_kl_bwd, ("beta",)),
    "vg_reparam_tc_fwd_dev": (tc._fwd_args, ("beta",)),
    "vg_reparam_tc_bwd_dev": (tc._bwd_args, ("beta",)),
    "vg_reparam_dip_fwd_dev": (dip._fwd_args, ("beta",)),
    "vg_reparam_dip_bwd_dev": (dip._bwd_args, ("beta",)),
    "vg_reparam_mmd_fwd_dev": (mmd._fwd_args, ("beta",)),
    "vg_reparam_mmd_bwd_dev": (mmd._bwd_args, ("beta",)),
    "vg_reparam_klc_fwd_dev": (klc._fwd_args, ("beta", "capacity")),
    "vg_reparam_klc_bwd_dev": (klc._bwd_args, ("beta", "capacity")),
    "vg_factor_tc_fwd_dev": (_factor_fwd, ("beta", "gamma")),
    "vg_factor_tc_bwd_dev": (_factor_bwd, ("beta", "gamma")),
    "vg_diff_augment_fwd_dev": (_augment, ("p",)),
    "vg_diff_augment_bwd_dev": (_augment, ("p",)),
    "vg_bce_loss_dev": (_bce, ("target",)),
}
CASES = [(name, word) for name, (_, words) in ENTRIES.items() for word in words]


@pytest.mark.parametrize("name,null", CASES, ids=[f"{n}-{w}" for n, w in CASES])
def test_a_null_word_is_refused_before_any_launch(lib, name, null):
    args, words = ENTRIES[name]
    keep, a = args()
    word = ctypes.addressof(keep) if keep is not None else A
    a.update({w: None if w == null else word for w in words})
    assert getattr(lib, name)(*a.values()) == -1
