"""Which bounds of max |tensor| (ops.amax_of) a Discriminator forward + backward finds attached by a producer ("cached") and
which it has to measure with a pass of its own.  (The conv-chain entries with a BatchNorm-on-load print MEASURED although their
bound travels in the in_affine tuple: the spy asks ops.known_amax, which looks at the tensor's own record only.)"""
import sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from disentangle_mlp_amd import ops, model
from disentangle_mlp_amd.trainer import ModelOpt
opt = ModelOpt()
enc = model.Encoder_celeba(opt).cuda() if hasattr(model, "Encoder_celeba") else None
D = model.Discriminator_celeba(opt).cuda()
x = torch.randn(32, 3, 64, 64, device="cuda")
calls = []
lib = ops._lib.load()
orig = ops.amax_of
def spy(t, in_affine=None):
    calls.append((tuple(t.shape), ops.known_amax(t, in_affine) is not None))
    return orig(t, in_affine)
ops.amax_of = spy
c = D.convs(x)
print("convs out has bound:", ops.known_amax(c) is not None, type(D.convs[-1]).__name__)
p, f = D(x)
(p.sum() + f.sum()).backward()
for s, k in calls: print(s, "cached" if k else "MEASURED")
