"""Do two versions of ``disentangle_mlp_amd/optim.py`` step the same bits through the same library calls?  The fused Adam
step is bit-deterministic, so a refactor of that file is checked with ``torch.equal`` on bit patterns, not with a tolerance.

    compare_optim_modules.py OLD_OPTIM.py [--out verdicts.json] [--skip-trainers]

OLD_OPTIM.py (say ``git show <commit>:disentangle_mlp_amd/optim.py > /tmp/optim_old.py``) is loaded beside this tree's
module as a second submodule of the package, so both run on the same kernels.  Two levels:

(a) The optimizer alone.  Per case both classes take STEPS steps on parameters and gradients drawn from the same seed
    (fp32 tensors of 0, 5 and 8192 + 7 elements; the ``big`` cases add two 1024 x 1024 weights, one of them frozen, for the
    emitted Linear bounds).  Cases: plain, guard, EMA, clip, clip + skip, weight decay coupled and decoupled -- each with
    host and with device scalars -- ``device_hyper``, ``ema_decay_on_device``, decay in one of two groups, amsgrad (torch's
    step), a closure under clipping, ``load_state_dict``, ``load_state_in_place``, and ``prepare_capture`` + a step
    captured in ``torch.cuda.graph``, replayed three times and followed by an eager step.  The guard and skip cases get an
    inf planted in one gradient of step PLANT.  Compared: every ``p``, ``state_dict()`` with its key order, the EMA
    tensors, the flag words, the clip record, ``_bounds`` -- and the sequence of library calls each side made, recorded by
    a proxy in ``_lib._lib``: names, every integer and floating argument, and which pointer arguments are NULL.
(b) Through the trainers.  ``trainer.HipAdam`` is set to the old class, then to the new one, and the eight cases of
    ``compare_trainer_modules.py`` run: every loss of every iteration and every ``checkpoint(0)`` entry must be identical.

Exit status 1 when anything differs; needs a GPU."""
import argparse, copy, ctypes, importlib.util, json, os, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "scripts"))
from compare_trainer_modules import BATCH, ITERATIONS, differences, everything, run as run_trainer      # noqa: E402

SEED, STEPS, PLANT = 999, 6, 3
SIZES = [(0,), (5,), (8192 + 7,)]
BIG = [(1024, 1024), (1024, 1024)]      # the second one is frozen: its bound is measured, not emitted


def load_old(path):
    spec = importlib.util.spec_from_file_location("disentangle_mlp_amd._optim_compared", path)
    mod = importlib.util.module_from_spec(spec)      # (its name puts it in the package: relative imports resolve)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    """Stands in ``_lib._lib``: forwards every call and logs (name, arguments as far as they can be compared)."""

    def __init__(self, lib, signatures):
        self._real, self._signatures, self.calls = lib, signatures, []

    def __getattr__(self, name):
        fn, types = getattr(self._real, name), self._signatures[name][1]

        def call(*args):
            self.calls.append((name,) + tuple(self._seen(a, t) for a, t in zip(args, types)))
            return fn(*args)
        return call

    @staticmethod
    def _seen(a, t):
        if isinstance(a, ctypes.Array):
            if a._type_ in (ctypes.c_void_p, ctypes.c_size_t):
                return ("array", [bool(x) if a._type_ is ctypes.c_void_p else int(x) for x in a])
            return ("tensors", [(int(e.n), bool(e.amax)) for e in a])      # _AdamTensor: one class per module
        if t is ctypes.c_void_p:
            return "ptr" if a else "NULL"
        return a


def groups_all(ps):
    return ps


def groups_decay_in_one(ps):
    return [dict(params=ps[:2]), dict(params=ps[2:], weight_decay=0.01)]


def drive_eager(opt, ps, feed):
    for i in range(STEPS):
        feed(i)
        opt.step()


def drive_closure(opt, ps, feed):
    import torch
    losses = []
    for i in range(STEPS):
        def closure(i=i):
            feed(i)
            return torch.tensor(float(i))
        losses.append(opt.step(closure))
    opt._compared_losses = losses


def drive_load_state_dict(opt, ps, feed):
    for i in range(STEPS):
        if i == STEPS // 2:
            opt.load_state_dict(copy.deepcopy(opt.state_dict()))
        feed(i)
        opt.step()


def drive_load_in_place(opt, ps, feed):
    kept = None
    for i in range(STEPS):
        if i == 2:
            kept = copy.deepcopy(opt.state_dict())
        if i == 4:
            opt.load_state_in_place(kept)
        feed(i)
        opt.step()


def drive_graph(opt, ps, feed):
    import torch
    feed(0)
    opt.step()                                           # one eager step: the state exists
    opt.prepare_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for i in range(3):
        feed(1 + i)
        opt.sync_hyper()
        graph.replay()
        if i:                                            # (the capture's own step() has counted the first)
            opt.replayed()
    feed(4)
    opt.step()
    opt._compared_graph = graph


def cases():
    guard, ema, clip = dict(nonfinite_guard=True), dict(ema_decay=0.9), dict(max_grad_norm=1.0)
    skip = dict(max_grad_norm=1.0, skip_nonfinite=True)
    wd, wdd = dict(weight_decay=0.01), dict(weight_decay=0.01, decoupled_weight_decay=True)
    out = []
    for cap in (False, True):
        tag = "-capturable" if cap else ""
        for name, kw in (("plain", {}), ("guard", guard), ("ema", ema), ("clip", clip), ("clip-skip", skip),
                         ("decay-coupled", wd), ("decay-decoupled", wdd), ("guard-ema-clip-decay", {**guard, **ema, **skip, **wd})):
            out.append((name + tag, dict(capturable=cap, **kw), groups_all, drive_eager, SIZES))
        out.append(("decay-in-one-group" + tag, dict(capturable=cap), groups_decay_in_one, drive_eager, SIZES))
        out.append(("big-guard" + tag, dict(capturable=cap, **guard), groups_all, drive_eager, SIZES + BIG))
    out += [
        ("device-hyper", dict(capturable=True, device_hyper=True), groups_all, drive_eager, SIZES),
        ("ema-decay-on-device", dict(capturable=True, ema_decay=0.9, ema_decay_on_device=True), groups_all, drive_eager, SIZES),
        ("amsgrad", dict(amsgrad=True, **guard, **ema), groups_all, drive_eager, SIZES),
        ("closure-clip", dict(**skip, **ema), groups_all, drive_closure, SIZES),
        ("load-state-dict", dict(capturable=True, **ema), groups_all, drive_load_state_dict, SIZES),
        ("load-state-in-place", dict(capturable=True, **guard), groups_all, drive_load_in_place, SIZES),
        ("graph", dict(capturable=True), groups_all, drive_graph, SIZES),
        ("graph-everything", dict(capturable=True, device_hyper=True, ema_decay_on_device=True, **guard, **ema, **skip, **wdd),
         groups_decay_in_one, drive_graph, SIZES),
    ]
    return out


def run_case(mod, rec, kw, groups, drive, sizes):
    """One class through one case; returns (what it left, the calls it made)."""
    import torch
    gen = torch.Generator().manual_seed(SEED)
    ps = [(torch.randn(*s, generator=gen) * 0.05).cuda().requires_grad_() for s in sizes]
    plan = [[torch.randn(*s, generator=gen).cuda() for s in sizes] for _ in range(STEPS)]
    if kw.get("nonfinite_guard") or kw.get("skip_nonfinite"):
        plan[PLANT][2][3] = float("inf")
    frozen = ps[-1] if len(sizes) > len(SIZES) else None
    for p in ps:
        if p is not frozen:
            p.grad = torch.zeros_like(p)

    def feed(i):
        for p, g in zip(ps, plan[i]):
            if p is not frozen:
                p.grad.copy_(g)

    opt = mod.HipAdam(groups(ps), lr=1e-3, **kw)
    rec.calls.clear()
    drive(opt, ps, feed)
    torch.cuda.synchronize()
    left = {"p": [p.detach().clone() for p in ps], "state_dict": opt.state_dict(),
            "ema": None if opt._ema is None else [e.clone() for e in opt._ema],
            "words": None if opt._words is None else opt._words.clone(),
            "clip_record": None if opt._clip_rec is None else opt.clip_record().clone(),
            "bounds": None if opt._bounds is None else opt._bounds.clone(),
            "bound_of": [i for i, p in enumerate(ps) if p in opt._bound_of],
            "losses": getattr(opt, "_compared_losses", None), "torch_stepped": opt._torch_stepped}
    return left, list(rec.calls)


def as_bits(x):
    """``x`` with every floating tensor viewed as integers of its width: a NaN the planted inf left compares too, and -0
    is not +0."""
    import torch
    if isinstance(x, torch.Tensor):
        ints = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16}
        return x.contiguous().view(ints[x.dtype]) if x.dtype in ints else x
    if isinstance(x, dict):
        return {k: as_bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [as_bits(v) for v in x]
    return x


def first_call_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return [f"call {i}: {x!r} != {y!r}"]
    return [] if len(a) == len(b) else [f"{len(a)} calls against {len(b)}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old_optim")
    ap.add_argument("--out")
    ap.add_argument("--skip-trainers", action="store_true", help="level (a) only")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("compare_optim_modules.py compares on the GPU; none found")
    from disentangle_mlp_amd import _lib, optim as new, trainer
    old = load_old(os.path.abspath(a.old_optim))
    rec = Recorder(_lib.load(), _lib.SIGNATURES)
    _lib._lib = rec
    alone = []
    for name, kw, groups, drive, sizes in cases():
        (l0, c0), (l1, c1) = (run_case(mod, rec, kw, groups, drive, sizes) for mod in (old, new))
        diff = differences(as_bits(l0), as_bits(l1), "left") + first_call_difference(c0, c1)
        alone.append({"case": name, "identical": not diff, "library_calls": len(c1),
                      "entry_points": sorted({c[0] for c in c1 if c[0].startswith("vg_adam_")}), "differences": diff[:8]})
        print(json.dumps(alone[-1]), flush=True)
    _lib._lib = rec._real
    through = []
    if not a.skip_trainers:
        g = torch.Generator().manual_seed(SEED)
        data = [(torch.rand(BATCH, 3, 64, 64, generator=g) * 2 - 1).cuda() for _ in range(ITERATIONS)]
        for name, extra in (("BetaVAEGANTrainer", False), ("VAETrainer", False), ("GANTrainer", False),
                            ("BetaVAEGANTrainer", True)):
            for graph in (True, False):
                res = []
                for cls in (old.HipAdam, new.HipAdam):
                    trainer.HipAdam = cls
                    res.append(run_trainer(trainer, name, dict(graph=graph, **(everything(torch) if extra else {})), data))
                trainer.HipAdam = new.HipAdam
                (l0, c0, *rest0), (l1, c1, *rest1) = res
                diff = differences(l0, l1, "losses") + differences(c0, c1)
                if rest0 != rest1:
                    diff.append(f"captures / graph / iteration: {rest0} != {rest1}")
                through.append({"trainer": name, "graph": graph, "all_options": extra, "identical": not diff,
                                "losses_compared": sum(len(l) for l in l0), "captures": rest1[0], "differences": diff[:8]})
                print(json.dumps(through[-1]), flush=True)
    out = {"what": "old against new optim.py: torch.equal on parameters, state_dict, EMA, flag words, clip record and "
                   "bounds, equality of the recorded library calls; then both classes under the trainers",
           "seed": SEED, "steps": STEPS, "planted_inf_at_step": PLANT, "optimizer_alone": alone,
           "through_trainers": {"batch": BATCH, "iterations": ITERATIONS, "cases": through},
           "all_identical": all(v["identical"] for v in alone + through)}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    sys.exit(0 if out["all_identical"] else 1)


if __name__ == "__main__":
    main()
