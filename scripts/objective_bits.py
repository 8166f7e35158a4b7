"""SHA-256 of everything the KL-phase objectives compute (beta-TCVAE, DIP-VAE I / II, InfoVAE / WAE-MMD, the KL capacity, the
plain KL term, FactorVAE's encoder loss), from seeded inputs: what a change that must not move a bit is compared by.  A few
seconds on the GPU.

  ops       `ops.reparam_<tc|dip|mmd>_fwd` / `_bwd` at (B, D) = (2, 1), (3, 5), (33, 65), (64, 128), (130, 129) -- the smallest
            legal batch, ragged strips and tiles, one full tile pair with a mirrored tile, TC's D > 128 instantiation -- with
            ``beta`` a float and the device word, DIP variants i and ii, MMD rbf with the default bandwidth and imq with 8
            bandwidths: z, out4 and the saved tensors of the forward; gmu and glv of the backward with ``gz`` and ``gloss``
            each present and absent.  `reparam_klc` at the same shapes with beta AND the capacity floats or words, free
            bits 0 and 0.05, the capacity at half and at twice the floored total (`KLC_CASES`); `reparam_kl` with its row
            sums; `factor_tc` forward and backward at `FACTOR_ROWS` rows -- 1, one below and one above the workgroup's 256.
  function  the same cases through `functional.reparam_*` and autograd: z, loss, parts and the two ``.grad``s (the loss and
            z both backpropagated).
  trainer   four iterations of `VAETrainer` at B = 8, graph on (two eager, the capture's first replay, one more replay),
            with each objective (the KL capacity constant and annealed, FactorVAE with its critic) and with none: every value of every returned loss dict and the final weights.

    objective_bits.py [--tree DIR] [--out out.json]

``--tree``: the checkout whose package is imported (default: this one), so that two commits are compared by one script.
Prints one JSON object; two runs agree when the objects are equal."""
import argparse, hashlib, json, math, os, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((2, 1), (3, 5), (33, 65), (64, 128), (130, 129))
BETA = 6.0
CASES = {      # name -> (objective, what follows ``beta`` in the forward op, what follows it in the backward op)
    "tc": ("tc", lambda B: (1.0, 0.5, math.log(B * 1000.0)), (1.0, 0.5)),
    "dip_i": ("dip", lambda B: (10.0, 100.0, "i"), (10.0, 100.0, "i")),
    "dip_ii": ("dip", lambda B: (10.0, 5.0, "ii"), (10.0, 5.0, "ii")),
    "mmd_rbf": ("mmd", lambda B: (1000.0, "rbf", None), (1000.0, "rbf", None)),
    "mmd_imq8": ("mmd", lambda B: (100.0, "imq", (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)),
                 (100.0, "imq", (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0))),
}
KLC_CASES = {f"klc_f{f}_fb{fb}": (f, fb) for f in (0.5, 2.0) for fb in (0.0, 0.05)}      # name -> (capacity / floored total, free bits)
FACTOR_ROWS = (1, 255, 257)
GAMMA = 35.0
TRAINER_CASES = {"none": {}, "tc": dict(tc_decomposition=(1.0, 0.5), dataset_size=1000), "dip_i": dict(dip_vae=("i", 10.0, 100.0)),
                 "dip_ii": dict(dip_vae=("ii", 10.0, 5.0)), "mmd_rbf": dict(mmd_vae=("rbf", 1000.0)),
                 "mmd_imq8": dict(mmd_vae=("imq", 100.0, (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0))),
                 "klc_constant": dict(kl_control=(5.0, 0.05)),
                 "klc_annealed": dict(kl_control=(lambda it: 25.0 * min(it, 3) / 3.0, 0.0)),
                 "factor": dict(factor_vae=GAMMA)}


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(str((t.dtype, tuple(t.shape))).encode() + t.numpy().tobytes()).hexdigest()


def inputs(torch, B, D):
    g = torch.Generator().manual_seed(1000 * B + D)
    i = {k: torch.randn(B, D, generator=g) for k in ("mu", "lv", "eps", "zp", "gz")}
    i["lv"] = 0.5 * i["lv"] - 1.0
    i["gloss"] = torch.tensor(0.75)
    return {k: v.cuda() for k, v in i.items()}


def word_or_float(torch, kind, v):
    return v if kind == "float" else torch.full((1,), v, device="cuda")


def klc_capacity(i, f, free_bits):
    """f times the floored total of the KL per sample, from the inputs in fp64 on the CPU, rounded to fp32"""
    import numpy as np
    mu, lv = i["mu"].double().cpu(), i["lv"].double().cpu()
    K = (-0.5 * (1.0 + lv - mu ** 2 - lv.exp())).sum(0)
    return float(np.float32(f * float(K.clamp(min=mu.shape[0] * free_bits).sum()) / mu.shape[0]))


def grads_of(bwd, i):
    """the backward with ``gz`` and ``gloss`` each present and absent: bwd(gz, gloss) -> (gmu, glv)"""
    d = {}
    for gz in (i["gz"], None):
        for gloss in (i["gloss"], None):
            gmu, glv = bwd(gz, gloss)
            tag = f"gz{int(gz is not None)}_gloss{int(gloss is not None)}"
            d[f"gmu_{tag}"], d[f"glv_{tag}"] = sha(gmu), sha(glv)
    return d


def run_ops_words(torch, ops):
    """The kernels whose scheduled words do not fit `CASES`: two words (klc, factor_tc), or no objective (reparam_kl)."""
    out = {}
    for B, D in SHAPES:
        i = inputs(torch, B, D)
        for kind in ("float", "word"):
            beta = word_or_float(torch, kind, BETA)
            z, kl, rows = ops.reparam_kl_fwd(i["mu"], i["lv"], i["eps"], beta, want_rows=True)
            out[f"{B}x{D}/kl/beta_{kind}"] = {"z": sha(z), "kl": sha(kl), "rows": sha(rows), **grads_of(
                lambda gz, gkl: ops.reparam_kl_bwd(gz, i["mu"], i["lv"], i["eps"], gkl, beta), i)}
            for name, (f, fb) in KLC_CASES.items():
                cap = word_or_float(torch, kind, klc_capacity(i, f, fb))
                z, out4, gate, kl_dim = ops.reparam_klc_fwd(i["mu"], i["lv"], i["eps"], beta, cap, fb)
                out[f"{B}x{D}/{name}/words_{kind}"] = {"z": sha(z), "out4": sha(out4), "gate": sha(gate), "kl_dim": sha(kl_dim), **grads_of(
                    lambda gz, gloss: ops.reparam_klc_bwd(gz, i["mu"], i["lv"], i["eps"], gate, gloss, beta, cap, fb), i)}
    for rows in FACTOR_ROWS:
        g = torch.Generator().manual_seed(rows)
        logits, kl, gloss = torch.randn(rows, 2, generator=g).cuda(), torch.tensor(3.25).cuda(), torch.tensor(0.75).cuda()
        for kind in ("float", "word"):
            beta, gamma = word_or_float(torch, kind, BETA), word_or_float(torch, kind, GAMMA)
            glogits, gkl = ops.factor_tc_bwd(logits, gloss, beta, gamma)
            out[f"{rows}/factor_tc/words_{kind}"] = {"out4": sha(ops.factor_tc_fwd(logits, kl, beta, gamma)), "glogits": sha(glogits),
                                                     "gkl": sha(gkl)}
    return out


def run_function_words(torch, F):
    out = {}
    for B, D in SHAPES:
        i = inputs(torch, B, D)
        i["mu"].requires_grad_(True), i["lv"].requires_grad_(True)
        for kind in ("float", "word"):
            beta = word_or_float(torch, kind, BETA)
            calls = {"kl": lambda: F.reparam_kl(i["mu"], i["lv"], i["eps"], beta)}
            for name, (f, fb) in KLC_CASES.items():
                cap = word_or_float(torch, kind, klc_capacity(i, f, fb))
                calls[name] = lambda cap=cap, fb=fb: F.reparam_klc_dims(i["mu"], i["lv"], i["eps"], beta, cap, fb)
            for name, fn in calls.items():
                i["mu"].grad = i["lv"].grad = None
                z, loss, *rest = fn()
                torch.autograd.backward([loss, z], grad_tensors=[i["gloss"], i["gz"]])
                out[f"{B}x{D}/{name}/words_{kind}"] = {"z": sha(z), "loss": sha(loss), **{f"rest{n}": sha(t) for n, t in enumerate(rest)},
                                                      "mu.grad": sha(i["mu"].grad), "lv.grad": sha(i["lv"].grad)}
    for rows in FACTOR_ROWS:
        g = torch.Generator().manual_seed(rows)
        logits, kl = torch.randn(rows, 2, generator=g).cuda().requires_grad_(True), torch.tensor(3.25).cuda().requires_grad_(True)
        for kind in ("float", "word"):
            logits.grad = kl.grad = None
            loss, parts = F.factor_tc(logits, kl, word_or_float(torch, kind, BETA), word_or_float(torch, kind, GAMMA))
            loss.backward(torch.tensor(0.75).cuda())
            out[f"{rows}/factor_tc/words_{kind}"] = {"loss": sha(loss), "parts": sha(parts), "logits.grad": sha(logits.grad),
                                                     "kl.grad": sha(kl.grad)}
    return out


def run_ops(torch, ops):
    out = run_ops_words(torch, ops)
    for B, D in SHAPES:
        i = inputs(torch, B, D)
        for name, (obj, fwd_args, bwd_args) in CASES.items():
            fwd, bwd = getattr(ops, f"reparam_{obj}_fwd"), getattr(ops, f"reparam_{obj}_bwd")
            lead = (i["mu"], i["lv"], i["eps"]) + ((i["zp"],) if obj == "mmd" else ())
            for beta_kind in ("float", "word"):
                beta = BETA if beta_kind == "float" else torch.full((1,), BETA, device="cuda")
                z, out4, *made = fwd(*lead, beta, *fwd_args(B))
                saved = (*lead[:3], *made) if obj == "dip" else (*lead[:3], z, *lead[3:], *made)
                d = {"z": sha(z), "out4": sha(out4), **{f"saved{n}": sha(t) for n, t in enumerate(made)}}
                for gz in (i["gz"], None):
                    for gloss in (i["gloss"], None):
                        gmu, glv = bwd(gz, *saved, gloss, beta, *bwd_args)
                        tag = f"gz{int(gz is not None)}_gloss{int(gloss is not None)}"
                        d[f"gmu_{tag}"], d[f"glv_{tag}"] = sha(gmu), sha(glv)
                out[f"{B}x{D}/{name}/beta_{beta_kind}"] = d
    return out


def run_function(torch, F):
    call = {"tc": lambda i, beta: F.reparam_tc(i["mu"], i["lv"], i["eps"], beta, 1.0, 0.5, dataset_size=1000),
            "dip_i": lambda i, beta: F.reparam_dip(i["mu"], i["lv"], i["eps"], beta, 10.0, 100.0, "i"),
            "dip_ii": lambda i, beta: F.reparam_dip(i["mu"], i["lv"], i["eps"], beta, 10.0, 5.0, "ii"),
            "mmd_rbf": lambda i, beta: F.reparam_mmd(i["mu"], i["lv"], i["eps"], i["zp"], beta, 1000.0, "rbf"),
            "mmd_imq8": lambda i, beta: F.reparam_mmd(i["mu"], i["lv"], i["eps"], i["zp"], beta, 100.0, "imq", CASES["mmd_imq8"][2][2])}
    out = run_function_words(torch, F)
    for B, D in SHAPES:
        i = inputs(torch, B, D)
        i["mu"].requires_grad_(True), i["lv"].requires_grad_(True)
        for name, fn in call.items():
            for beta_kind in ("float", "word"):
                i["mu"].grad = i["lv"].grad = None
                z, loss, parts = fn(i, BETA if beta_kind == "float" else torch.full((1,), BETA, device="cuda"))
                torch.autograd.backward([loss, z], grad_tensors=[i["gloss"], i["gz"]])
                out[f"{B}x{D}/{name}/beta_{beta_kind}"] = {"z": sha(z), "loss": sha(loss), "parts": sha(parts),
                                                          "mu.grad": sha(i["mu"].grad), "lv.grad": sha(i["lv"].grad)}
    return out


def run_trainer(torch, T):
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(8, 3, 64, 64, generator=g) * 2 - 1).cuda()
    eps, prior = (torch.randn(4, 8, 128, generator=g).cuda() for _ in range(2))
    out = {}
    for name, kw in TRAINER_CASES.items():
        tr = T.VAETrainer(device="cuda:0", seed=7, beta=BETA, graph=True, **kw)
        extra = (lambda n: dict(prior=prior[n])) if "mmd_vae" in kw else (lambda n: {})
        d = {}
        for n in range(4):
            for k, v in tr.step(x, eps[n], **extra(n)).items():
                d[f"iteration{n}/{k}"] = sha(v)
        d["captures"] = len(tr._graphs)
        d["weights"] = sha(torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()]))
        out[name] = d
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--out")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    import torch
    from disentangle_mlp_amd import functional as F, ops, trainer as T
    assert os.path.dirname(os.path.dirname(os.path.abspath(T.__file__))) == tree
    if not torch.cuda.is_available():
        raise SystemExit("objective_bits.py runs the kernels: it needs the GPU")
    res = {"ops": run_ops(torch, ops), "function": run_function(torch, F), "trainer": run_trainer(torch, T)}
    text = json.dumps(res, indent=1, sort_keys=True)
    res["sha256_of_all"] = hashlib.sha256(text.encode()).hexdigest()
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
