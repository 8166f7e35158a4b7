"""SHA-256 of everything the BatchNorm kernels of csrc/bn.hip compute, from seeded inputs: what a change that must not move
a bit is compared by.  A few seconds on the GPU; the largest tensor is 42 MB.

Every output of every entry point through `ops`, the amax slot or bound where one is returned, the whole set once with
``ops.CONV_ARITH`` at "fp16x3" (the slots and bounds exist) and once at "fp32":

  train       `bn_act_fwd`, `bn_stats`, `bn_act_bwd` on every shape of SHAPES_2D and SHAPES_1D (tests/_bn_refs.py): the
              three activations, momentum 0.1 and 1.0, running buffers given and None, ``need_param_grads=False``,
              ``accumulate_into``.
  misaligned  the same three on MISALIGNED_SHAPES with x, x and gy, and gy alone 1-3 floats off a 16-byte boundary, as
              tests/test_bn_gpu.py forms them.
  finalize    `bn_finalize_stats` on every (nslots, C) of SLOT_CASES, with and without ``want_bound``.
  team        the team backward on its natural cases (33, 128, 32, 32) and (65, 160, 32, 32), and on the FORCED cases of
              tests/_bn_team_refs.py through the tuning library's knob (reset afterwards).
  eval        `bn_eval_coeffs` without slots and with 7, 64, 65 and 4097 of them; `bn_eval_act_bwd` on three 2-D and two 1-D
              shapes, the three activations, with and without parameter gradients and accumulation.
  elementwise `affine_act` and `channel_sum` on a vector shape, a scalar shape and a misaligned view.

    bn_bits.py [--tree DIR] [--out out.json]

``--tree``: the checkout whose package is imported (default: this one), so that two commits are compared by one script; the
seeded case generators are always this checkout's (tests/_bn_refs.py, tests/_bn_team_refs.py): both runs see the same
inputs.  Prints one JSON object; two runs agree when the objects are equal, and the per-case keys say which kernel moved."""
import argparse, hashlib, json, os, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
import _bn_refs as R            # noqa: E402
import _bn_team_refs as T       # noqa: E402

EPS = R.EPS
EVAL_BWD_SHAPES = ((10, 5, 21, 21), (32, 128, 16, 16), (1, 3, 2, 2), (7, 33), (128, 33))
EVAL_SLOTS = (7, 64, 65, 4097)


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        if t is None:
            h.update(b"none")
            continue
        t = t.detach().contiguous().cpu()
        h.update(str((t.dtype, tuple(t.shape))).encode() + t.numpy().tobytes())
    return h.hexdigest()


def at_offset(torch, t, o):
    """A contiguous copy of t whose first element lies o floats past a 16-byte boundary."""
    t = t.contiguous()
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    v = buf[o:o + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * (o % 4)
    return v


def case(shape):
    i = R.bn_inputs(tuple(shape))
    return {k: (v.cuda() if hasattr(v, "cuda") else v) for k, v in i.items()}


def run_fwd(ops, i, x, out, tag):
    for act, code in R.ACTS.items():
        for mom in (0.1, 1.0):
            for running in (True, False):
                rm, rv = (i["rm0"].clone(), i["rv0"].clone()) if running else (None, None)
                y, mean, invstd = ops.bn_act_fwd(x, i["gamma"], i["beta"], rm, rv, EPS, mom, code)
                out[f"{tag}/fwd/{act}/mom{mom}/running{int(running)}"] = sha(y, mean, invstd, rm, rv, ops.known_amax(y))
    for mom in (0.1, 1.0):
        for running in (True, False):
            rm, rv = (i["rm0"].clone(), i["rv0"].clone()) if running else (None, None)
            res = ops.bn_stats(x, i["gamma"], i["beta"], rm, rv, EPS, mom, want_bound=True)
            out[f"{tag}/stats/mom{mom}/running{int(running)}"] = sha(*res, rm, rv)


def run_bwd(torch, ops, i, shape, gy, x, out, tag, extras=True):
    C = shape[1]
    mean, invstd = (t.cuda() for t in T.saved(tuple(shape)))
    g = torch.Generator().manual_seed(31)
    g0, b0 = torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    for act, code in R.ACTS.items():
        gx, dgamma, dbeta = ops.bn_act_bwd(gy, x, i["gamma"], i["beta"], mean, invstd, code)
        out[f"{tag}/bwd/{act}"] = sha(gx, dgamma, dbeta, ops.known_amax(gx))
        if not extras:
            continue
        gx, _, _ = ops.bn_act_bwd(gy, x, i["gamma"], i["beta"], mean, invstd, code, need_param_grads=False)
        out[f"{tag}/bwd/{act}/no_param_grads"] = sha(gx, ops.known_amax(gx))
        acc = (g0.clone(), b0.clone())
        gx, _, _ = ops.bn_act_bwd(gy, x, i["gamma"], i["beta"], mean, invstd, code, accumulate_into=acc)
        out[f"{tag}/bwd/{act}/accumulate"] = sha(gx, *acc, ops.known_amax(gx))


def run_train(torch, ops):
    out = {}
    for shape in tuple(R.SHAPES_2D) + tuple(R.SHAPES_1D):
        i = case(shape)
        run_fwd(ops, i, i["x"], out, str(shape))
        run_bwd(torch, ops, i, shape, i["gy"], i["x"], out, str(shape))
    return out


def run_misaligned(torch, ops):
    out = {}
    for shape in R.MISALIGNED_SHAPES:
        i = case(shape)
        for o in (1, 2, 3):
            xo = at_offset(torch, i["x"], o)
            run_fwd(ops, i, xo, out, f"{shape}/x+{o}")
            run_bwd(torch, ops, i, shape, i["gy"], xo, out, f"{shape}/x+{o}", extras=False)
            run_bwd(torch, ops, i, shape, at_offset(torch, i["gy"], o), xo, out, f"{shape}/x+{o},gy+{o}", extras=(o == 1))
        run_bwd(torch, ops, i, shape, at_offset(torch, i["gy"], 2), i["x"], out, f"{shape}/gy+2", extras=False)
    return out


def run_finalize(ops):
    out = {}
    for nslots, Cs in R.SLOT_CASES.items():
        for C in Cs:
            i = R.slot_inputs(nslots, C)
            stats, gamma, beta = i["stats"].cuda(), i["gamma"].cuda(), i["beta"].cuda()
            for want_bound in (False, True):
                for running in (True, False):
                    rm, rv = (i["rm0"].cuda(), i["rv0"].cuda()) if running else (None, None)
                    res = ops.bn_finalize_stats(stats, i["count"], gamma, beta, rm, rv, EPS, 0.1, want_bound=want_bound)
                    out[f"slots{nslots}/C{C}/bound{int(want_bound)}/running{int(running)}"] = sha(*res, rm, rv)
    return out


def run_team(torch, ops, _lib):
    out = {}
    for shape in ((33, 128, 32, 32), (65, 160, 32, 32)):
        i = case(shape)
        run_bwd(torch, ops, i, shape, i["gy"], i["x"], out, f"natural/{shape}")
    with _lib.use_tuning() as lib:
        try:
            for shape, (max_wgs, _) in T.FORCED.items():
                assert lib.vg_debug_set_bn_team(1, max_wgs) == 0
                i = case(shape)
                run_bwd(torch, ops, i, shape, i["gy"], i["x"], out, f"forced/{shape}/wgs{max_wgs}")
        finally:
            lib.vg_debug_set_bn_team(0, 0)
    return out


def run_eval(torch, ops):
    out = {}
    i = case((10, 5, 21, 21))
    for act, code in R.ACTS.items():
        out[f"coeffs/no_slots/{act}"] = sha(*ops.bn_eval_coeffs(i["gamma"], i["beta"], i["rm0"], i["rv0"], EPS, code, want_bound=True))
    for nslots in EVAL_SLOTS:
        for C in R.SLOT_CASES[nslots]:
            s = R.slot_inputs(nslots, C)
            res = ops.bn_eval_coeffs(s["gamma"].cuda(), s["beta"].cuda(), s["rm0"].cuda(), s["rv0"].cuda(), EPS, 1,
                                     stats=s["stats"].cuda(), count=s["count"], want_bound=True)
            out[f"coeffs/slots{nslots}/C{C}"] = sha(*res)
    g = torch.Generator().manual_seed(33)
    for shape in EVAL_BWD_SHAPES:
        i = case(shape)
        C = shape[1]
        g0, b0 = torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
        for act, code in R.ACTS.items():
            scale, shift, invstd = ops.bn_eval_coeffs(i["gamma"], i["beta"], i["rm0"], i["rv0"], EPS, code)
            args = (i["gy"], i["x"], scale, shift, i["rm0"], invstd, code)
            gx, dgamma, dbeta = ops.bn_eval_act_bwd(*args)
            out[f"bwd/{shape}/{act}"] = sha(gx, dgamma, dbeta, ops.known_amax(gx))
            gx, _, _ = ops.bn_eval_act_bwd(*args, need_param_grads=False)
            out[f"bwd/{shape}/{act}/no_param_grads"] = sha(gx, ops.known_amax(gx))
            acc = (g0.clone(), b0.clone())
            gx, _, _ = ops.bn_eval_act_bwd(*args, accumulate_into=acc)
            out[f"bwd/{shape}/{act}/accumulate"] = sha(gx, *acc, ops.known_amax(gx))
    return out


def run_elementwise(torch, ops):
    out = {}
    for name, shape, o in (("vector", (2, 5, 8, 8), 0), ("scalar", (3, 7, 5, 1), 0), ("misaligned", (2, 5, 8, 8), 1)):
        i = case(shape)
        x = at_offset(torch, i["x"], o) if o else i["x"]
        for act, code in R.ACTS.items():
            y = ops.affine_act(x, i["gamma"], i["beta"], code)
            out[f"affine_act/{name}/{act}"] = sha(y, ops.known_amax(y))
    for name, shape, o in (("vector", (17, 3, 64, 64), 0), ("scalar", (3, 7, 5, 1), 0), ("misaligned", (17, 3, 64, 64), 3)):
        i = case(shape)
        out[f"channel_sum/{name}"] = sha(ops.channel_sum(at_offset(torch, i["gy"], o) if o else i["gy"]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--out")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    import torch
    from disentangle_mlp_amd import _lib, ops
    assert os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__))) == tree
    if not torch.cuda.is_available():
        raise SystemExit("bn_bits.py runs the kernels: it needs the GPU")
    res, arith = {}, ops.CONV_ARITH
    try:
        for ops.CONV_ARITH in ("fp16x3", "fp32"):
            res[ops.CONV_ARITH] = {"train": run_train(torch, ops), "misaligned": run_misaligned(torch, ops),
                                   "finalize": run_finalize(ops), "team": run_team(torch, ops, _lib),
                                   "eval": run_eval(torch, ops), "elementwise": run_elementwise(torch, ops)}
    finally:
        ops.CONV_ARITH = arith
    text = json.dumps(res, indent=1, sort_keys=True)
    res["sha256_of_all"] = hashlib.sha256(text.encode()).hexdigest()
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
