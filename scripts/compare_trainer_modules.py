"""Do two versions of ``disentangle_mlp_amd/trainer.py`` train the same bits?  The trainers are bit-deterministic, so a
refactor of that file is checked with ``torch.equal``, not with a tolerance.

    compare_trainer_modules.py OLD_TRAINER.py [--out verdicts.json]

OLD_TRAINER.py (say ``git show <commit>:disentangle_mlp_amd/trainer.py > /tmp/trainer_old.py``) is loaded beside this
tree's module as a second submodule of the package, so both run on the same kernels, model and optimizer code.  Cases:
each of the three trainers with ``graph`` on and off, and BetaVAEGANTrainer once more (on and off) with ``lr_scheduler``,
``beta_schedule``, ``ema_decay``, ``max_grad_norm`` and ``tc_decomposition`` all set.  Per case both versions run
ITERATIONS iterations at batch BATCH from seed SEED on the same data, latents left to the trainer, labels alternating
(0.9, 0.1) / (0.1, 0.9); every loss of every iteration and every entry of ``checkpoint(0)`` afterwards (weights,
BatchNorm buffers, Adam state, and the EMA / scheduler / iteration keys where there are some) must be identical.  Exit
status 1 when a case differs; needs a GPU."""
import argparse, importlib.util, json, os, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SEED, BATCH, ITERATIONS = 999, 8, 6
LABELS = [(0.9, 0.1), (0.1, 0.9)]


def load_old(path):
    spec = importlib.util.spec_from_file_location("disentangle_mlp_amd._trainer_compared", path)
    mod = importlib.util.module_from_spec(spec)      # (its name puts it in the package: relative imports resolve)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def everything(torch):
    return dict(lr_scheduler=lambda opt: torch.optim.lr_scheduler.LambdaLR(opt, lambda i: 0.97 ** i),
                beta_schedule=lambda it: 1.0 + 4.0 * it, ema_decay=0.9, max_grad_norm=50.0,
                tc_decomposition=(1.0, 1.0), dataset_size=1000)


def differences(a, b, where="checkpoint"):
    """Paths at which two nested dict / list / tensor / scalar structures differ."""
    import torch
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        same = (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape
                and torch.equal(a, b))
        return [] if same else [where]
    if isinstance(a, dict) and isinstance(b, dict):
        if list(a) != list(b):
            return [f"{where}: keys {list(a)} != {list(b)}"]
        return [d for k in a for d in differences(a[k], b[k], f"{where}[{k!r}]")]
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return [f"{where}: lengths {len(a)} != {len(b)}"]
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, f"{where}[{i}]")]
    return [] if type(a) is type(b) and a == b else [where]


def run(module, name, kwargs, data):
    import torch
    tr = getattr(module, name)(seed=SEED, **kwargs)
    losses = []
    for i, x in enumerate(data):
        labels = {} if name == "VAETrainer" else dict(real_label=LABELS[i % 2][0], fake_label=LABELS[i % 2][1])
        losses.append({k: v.clone() for k, v in tr.step(x, **labels).items()})
    torch.cuda.synchronize()
    return losses, tr.checkpoint(0), len(tr._graphs), tr.graph, tr.iteration


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old_trainer")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("compare_trainer_modules.py compares on the GPU; none found")
    from disentangle_mlp_amd import trainer as new
    old = load_old(os.path.abspath(a.old_trainer))
    g = torch.Generator().manual_seed(SEED)
    data = [(torch.rand(BATCH, 3, 64, 64, generator=g) * 2 - 1).cuda() for _ in range(ITERATIONS)]
    cases = [(n, graph, extra) for n, extra in (("BetaVAEGANTrainer", False), ("VAETrainer", False), ("GANTrainer", False),
                                                ("BetaVAEGANTrainer", True)) for graph in (True, False)]
    verdicts = []
    for name, graph, extra in cases:
        res = []
        for module in (old, new):
            kwargs = dict(graph=graph, **(everything(torch) if extra else {}))
            res.append(run(module, name, kwargs, data))
        (l0, c0, caps0, g0, it0), (l1, c1, caps1, g1, it1) = res
        diff = differences(l0, l1, "losses") + differences(c0, c1)
        if (caps0, g0, it0) != (caps1, g1, it1):
            diff.append(f"captures / graph / iteration: {(caps0, g0, it0)} != {(caps1, g1, it1)}")
        verdicts.append({"trainer": name, "graph": graph, "all_options": extra, "identical": not diff,
                         "losses_compared": sum(len(l) for l in l0), "checkpoint_keys": list(c1),
                         "captures": caps1, "iterations": it1, "differences": diff[:8]})
        print(json.dumps(verdicts[-1]), flush=True)
    out = {"what": "old against new trainer.py, torch.equal on every loss of every iteration and every checkpoint entry",
           "seed": SEED, "batch": BATCH, "iterations": ITERATIONS, "cases": verdicts,
           "all_identical": all(v["identical"] for v in verdicts)}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    sys.exit(0 if out["all_identical"] else 1)


if __name__ == "__main__":
    main()
