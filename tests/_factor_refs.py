"""Plain-torch CPU restatements of FactorVAE's pieces (Kim & Mnih 2018, "Disentangling by Factorising", algorithm 2 and
section 3; the batch reductions are this project's: KL and TC as sums over the batch, the critic's cross-entropy as a
mean), in fp64 or fp32, for tests/test_factor_vae_*.py.  The critic has two logits: class 0 is "drawn from q(z)", class 1
"dimensions permuted across the batch"."""
import torch
import torch.nn.functional as tF

from _tc_refs import bound, rel_err  # noqa: F401  (the project's convention, shared with the other objectives' tests)

BETA, GAMMA, GLOSS = 4.0, 6.4, 0.75
GAPS = (0.0, 1e-8, -1e-8, 30.0, -30.0, 100.0, -100.0, 1e4, -1e4)      # l0 - l1 of the first rows of `make_logits`
ROWS = (1, 63, 64, 65, 128, 1000)


def ranks(u):
    """rank[i, d]: the position of u[i, d] in the stable ascending order of column d -- by counting, as the kernel does: the
    rows that are smaller, and the equal ones in front of it."""
    u = u.double()
    B = u.shape[0]
    earlier = torch.arange(B).view(B, 1) < torch.arange(B).view(1, B)          # [j, i]: j < i
    less = u.unsqueeze(1) < u.unsqueeze(0)                                     # [j, i, d]: u[j, d] < u[i, d]
    tie = (u.unsqueeze(1) == u.unsqueeze(0)) & earlier.unsqueeze(-1)
    return (less | tie).sum(0)                                                  # [i, d]


def permute_dims(z, u):
    """z_perm[rank[i, d], d] = z[i, d]: every column permuted on its own by the stable argsort of the same column of u."""
    return torch.zeros_like(z).scatter_(0, ranks(u), z)


def make_logits(rows, seed=0):
    """[rows, 2] fp32 logits: normal draws of scale 3, the first rows with l1 = 0 and l0 = GAPS -- a tie, the smallest gaps,
    and gaps that saturate softplus and sigmoid in fp32 and in fp64."""
    g = torch.Generator().manual_seed(1000 * rows + seed)
    logits = 3.0 * torch.randn(rows, 2, generator=g)
    n = min(rows, len(GAPS))
    logits[:n, 1] = 0.0
    logits[:n, 0] = torch.tensor(GAPS[:n])
    return logits


def factor_tc(logits, kl, beta, gamma, gloss=GLOSS, dtype=torch.float64):
    """loss = beta*kl + gamma*sum_b(l0 - l1), its parts, and the gradients of gloss*loss by autograd."""
    logits = logits.detach().to(dtype, copy=True).requires_grad_(True)
    kl = torch.as_tensor(kl, dtype=dtype).clone().requires_grad_(True)
    tc = (logits[:, 0] - logits[:, 1]).sum()
    loss = beta * kl + gamma * tc
    glogits, gkl = torch.autograd.grad(gloss * loss, (logits, kl))
    return dict(loss=loss.detach(), kl=kl.detach(), tc=tc.detach(), first=int((logits[:, 0] > logits[:, 1]).sum()),
                glogits=glogits, gkl=gkl)


def critic_loss(logits, divisor=None, dtype=torch.float64):
    """The critic's loss on [z; z_perm] -- the first half of the rows is class 0, the second class 1 --: with x = the other
    class's logit minus the row's own, -log p(own) = softplus(x), summed and divided by ``divisor`` (default: the rows);
    d/dx = sigmoid(x), to the other logit with +, to the own with -; the accuracy counts x < 0 (a tie is wrong).  softplus in
    its overflow-safe form: a saturated row gives x or 0, and a gradient of exactly 1/divisor or 0."""
    rows = logits.shape[0]
    div = float(divisor if divisor is not None else rows)
    first = torch.arange(rows) < rows // 2
    l = logits.to(dtype)
    x = torch.where(first, l[:, 1] - l[:, 0], l[:, 0] - l[:, 1])
    loss = (x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))).sum() / div
    g = torch.sigmoid(x) / div
    glogits = torch.stack([torch.where(first, -g, g), torch.where(first, g, -g)], dim=1)
    return dict(loss=loss, glogits=glogits, acc=float((x < 0).double().mean()))


def cross_entropy_form(logits, divisor=None, dtype=torch.float64):
    """The same loss as torch states it -- the 2-class cross-entropy, summed, over ``divisor`` -- and its gradient by autograd."""
    rows = logits.shape[0]
    labels = (torch.arange(rows) >= rows // 2).long()
    x = logits.detach().to(dtype, copy=True).requires_grad_(True)
    loss = tF.cross_entropy(x, labels, reduction="sum") / float(divisor if divisor is not None else rows)
    glogits, = torch.autograd.grad(loss, x)
    return loss.detach(), glogits


def torch_critic(critic, dtype):
    """torch.nn modules carrying the weights of a `model.LatentCritic`: the state_dict keys are the same."""
    layers = []
    for m in critic:
        layers.append(torch.nn.Linear(m.in_features, m.out_features) if hasattr(m, "in_features") else torch.nn.LeakyReLU(0.2))
    net = torch.nn.Sequential(*layers)
    net.load_state_dict({k: v.detach().cpu() for k, v in critic.state_dict().items()})
    return net.to(dtype)
