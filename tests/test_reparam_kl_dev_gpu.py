"""GPU: the reparameterisation / KL kernels with beta read from device memory (vg_reparam_kl_fwd_dev,
vg_reparam_kl_bwd_dev) against the kernels that take beta as a host float: the same fp32 beta gives the same bits -- z,
the KL scalar, the per-sample rows, both gradients -- with and without ``kl_rows``, with ``gz`` / ``gkl`` each NULL in turn;
the word is read at every launch (changing it between two launches changes the result); a NULL ``beta_dev`` is refused
before any launch.  Sentinels surround every written buffer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
PAD = 16
BETAS = [0.0, 1.0, 25.0, 1e-3, float(np.float32(0.1))]
SHAPES = [(1, 1), (4, 128), (17, 130), (16, 64)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lib():
    from disentangle_mlp_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _padded(n):
    buf = torch.full((n + 2 * PAD,), SENTINEL, device="cuda")
    return buf, buf[PAD:PAD + n]


def _intact(buf, n):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all())


_INPUTS = {}


def _inputs(B, D):
    """mu, logvar, eps, gz, gkl of one shape: made once, only read."""
    if (B, D) not in _INPUTS:
        gen = torch.Generator().manual_seed(100 * B + D)
        _INPUTS[(B, D)] = tuple(t.cuda() for t in (torch.randn(B, D, generator=gen), torch.randn(B, D, generator=gen) * 0.5,
                                                   torch.randn(B, D, generator=gen), torch.randn(B, D, generator=gen),
                                                   torch.randn(1, generator=gen)))
    return _INPUTS[(B, D)]


def _fwd(mu, lv, eps, beta, rows, dev):
    from disentangle_mlp_amd._lib import check
    lib = _lib()
    B, D = mu.shape
    zb, z = _padded(B * D)
    kb, kl = _padded(1)
    rb, r = _padded(B)
    args = (mu.data_ptr(), lv.data_ptr(), eps.data_ptr(), z.data_ptr(), kl.data_ptr(), r.data_ptr() if rows else None, B, D)
    if dev:
        check(lib.vg_reparam_kl_fwd_dev(*args, beta.data_ptr(), _stream()), "vg_reparam_kl_fwd_dev")
    else:
        check(lib.vg_reparam_kl_fwd(*args, float(beta), _stream()), "vg_reparam_kl_fwd")
    torch.cuda.synchronize()
    assert _intact(zb, B * D) and _intact(kb, 1) and _intact(rb, B)
    assert rows or bool((rb == SENTINEL).all())
    return zb, kb, rb


def _bwd(mu, lv, eps, gz, gkl, beta, dev):
    from disentangle_mlp_amd._lib import check
    lib = _lib()
    B, D = mu.shape
    mb, gmu = _padded(B * D)
    lb, glv = _padded(B * D)
    head = (None if gz is None else gz.data_ptr(), mu.data_ptr(), lv.data_ptr(), eps.data_ptr(),
            None if gkl is None else gkl.data_ptr())
    tail = (gmu.data_ptr(), glv.data_ptr(), B, D, _stream())
    if dev:
        check(lib.vg_reparam_kl_bwd_dev(*head, beta.data_ptr(), *tail), "vg_reparam_kl_bwd_dev")
    else:
        check(lib.vg_reparam_kl_bwd(*head, float(beta), *tail), "vg_reparam_kl_bwd")
    torch.cuda.synchronize()
    assert _intact(mb, B * D) and _intact(lb, B * D)
    return mb, lb


@pytest.mark.parametrize("B,D", SHAPES, ids=[f"{b}x{d}" for b, d in SHAPES])
def test_device_beta_gives_the_bits_of_the_host_beta(B, D):
    mu, lv, eps, gz, gkl = _inputs(B, D)
    word = torch.zeros(1, device="cuda")
    seen = set()
    for beta in BETAS:
        word.fill_(beta)
        assert float(word) == float(np.float32(beta))
        for rows in (False, True):
            for x, y in zip(_fwd(mu, lv, eps, beta, rows, False), _fwd(mu, lv, eps, word, rows, True)):
                assert torch.equal(_bits(x), _bits(y)), (beta, rows)
        for use_gz, use_gkl in ((True, True), (False, True), (True, False)):
            a = _bwd(mu, lv, eps, gz if use_gz else None, gkl if use_gkl else None, beta, False)
            b = _bwd(mu, lv, eps, gz if use_gz else None, gkl if use_gkl else None, word, True)
            for x, y in zip(a, b):
                assert torch.equal(_bits(x), _bits(y)), (beta, use_gz, use_gkl)
        seen.add(float(_fwd(mu, lv, eps, word, False, True)[1][PAD]))
    assert len(seen) == len(BETAS)                                # every beta its own KL: the word is what scales it


def test_the_word_is_read_at_every_launch():
    mu, lv, eps, gz, gkl = _inputs(4, 128)
    word = torch.full((1,), 2.0, device="cuda")
    k2 = _fwd(mu, lv, eps, word, False, True)[1][PAD].clone()
    g2 = _bwd(mu, lv, eps, None, gkl, word, True)[0][PAD:PAD + 512].clone()
    word.fill_(4.0)                                               # doubling beta is exact in fp32
    k4 = _fwd(mu, lv, eps, word, False, True)[1][PAD].clone()
    g4 = _bwd(mu, lv, eps, None, gkl, word, True)[0][PAD:PAD + 512].clone()
    assert float(k2) != 0.0 and float(k4) == 2.0 * float(k2)
    assert torch.equal(_bits(g4), _bits(2.0 * g2))
    assert torch.equal(_bits(k4), _bits(_fwd(mu, lv, eps, 4.0, False, False)[1][PAD]))


def test_a_null_word_is_refused_before_any_launch():
    lib = _lib()
    mu, lv, eps, gz, gkl = _inputs(4, 128)
    zb, z = _padded(512)
    kb, kl = _padded(1)
    mb, gmu = _padded(512)
    lb, glv = _padded(512)
    assert lib.vg_reparam_kl_fwd_dev(mu.data_ptr(), lv.data_ptr(), eps.data_ptr(), z.data_ptr(), kl.data_ptr(), None, 4, 128,
                                     None, _stream()) == -1
    assert lib.vg_reparam_kl_bwd_dev(gz.data_ptr(), mu.data_ptr(), lv.data_ptr(), eps.data_ptr(), gkl.data_ptr(), None,
                                     gmu.data_ptr(), glv.data_ptr(), 4, 128, _stream()) == -1
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in (zb, kb, mb, lb))


def test_functional_takes_the_word_and_gives_it_no_gradient():
    from disentangle_mlp_amd import functional as F
    mu, lv, eps, _, _ = _inputs(17, 130)
    word = torch.full((1,), 25.0, device="cuda")
    out = []
    for beta in (25.0, word):
        m, l = mu.clone().requires_grad_(), lv.clone().requires_grad_()
        z, kl = F.reparam_kl(m, l, eps, beta)
        (z.sum() + kl).backward()
        out.append((z.detach(), kl.detach(), m.grad, l.grad, F.kld_loss(mu, lv, beta)))
    for x, y in zip(*out):
        assert torch.equal(_bits(x), _bits(y))
    assert word.grad is None
    with pytest.raises(RuntimeError, match="one fp32 element"):
        F.reparam_kl(mu, lv, eps, torch.ones(2, device="cuda"))
