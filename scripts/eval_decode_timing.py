"""Time VAE.decode under no_grad in eval mode (running statistics) against train mode (batch statistics), at B = 128
and B = 1, interleaved in one process; medians and spread go to profiles/r07_eval_decode.json.  Also counts, per eval
decode, how many BatchNorm bounds came from the producer's statistics slots and how many from an exact
vg_absmax_affine pass.

``--parent DIR``: a directory holding the PARENT commit's ``disentangle_mlp_amd`` package with a built library
(``git archive <parent> disentangle_mlp_amd | tar -x -C DIR`` + the two .so files); its train-mode decode is then timed
as well ("parent_train"), loaded under another module name beside this tree's.  Without it only this tree's train mode
is timed, and the JSON says so.

    python scripts/eval_decode_timing.py [--parent DIR] [--rounds 15] [--inner 20] [--out profiles/r07_eval_decode.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from disentangle_mlp_amd import model as M, ops  # noqa: E402
from disentangle_mlp_amd.trainer import ModelOpt  # noqa: E402


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner * 1e3          # microseconds per decode


def count_bounds(vae, z):
    """(bounds from slots, exact affine passes) of one eval decode."""
    n = {"slots": 0, "exact": 0}
    coeffs, lib = ops.bn_eval_coeffs, ops._lib.load()

    def counted(*a, **k):
        out = coeffs(*a, **k)
        if k.get("want_bound") and out[3] is not None:
            n["slots"] += 1
        return out
    exact = lib.vg_absmax_affine

    def counted_exact(*a):
        n["exact"] += 1
        return exact(*a)
    ops.bn_eval_coeffs, lib.vg_absmax_affine = counted, counted_exact
    try:
        with torch.no_grad(), M.eval_mode(vae):
            vae.decode(z)
    finally:
        ops.bn_eval_coeffs, lib.vg_absmax_affine = coeffs, exact
    return n


def load_parent(root):
    """The package under ``root`` as module ``vg_parent`` (its relative imports stay inside it)."""
    path = os.path.join(root, "disentangle_mlp_amd")
    spec = importlib.util.spec_from_file_location("vg_parent", os.path.join(path, "__init__.py"),
                                                  submodule_search_locations=[path])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["vg_parent"] = pkg
    spec.loader.exec_module(pkg)
    import vg_parent.model as PM
    import vg_parent.ops as Pops
    return PM, Pops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "r07_eval_decode.json"))
    args = ap.parse_args()
    torch.manual_seed(0)
    vae = M.VAE(ModelOpt()).cuda()
    vae.apply(M.weights_init)
    res = {"device": torch.cuda.get_device_name(0), "arith": ops.CONV_ARITH, "rounds": args.rounds, "inner": args.inner,
           "unit": "microseconds per VAE.decode under no_grad, eager",
           "parent_train": "the parent commit's package, same weights" if args.parent else "not timed (no --parent)"}
    pvae, pscope = None, None
    if args.parent:
        PM, Pops = load_parent(args.parent)
        pvae = PM.VAE(ModelOpt()).cuda()
        pvae.load_state_dict(vae.state_dict())
        pscope = Pops.packed_filter_scope()
        pscope.__enter__()
    with torch.no_grad(), ops.packed_filter_scope():
        for B in (128, 1):
            z = torch.randn(B, 128, device="cuda")
            runs = {"parent_train": [], "train": [], "eval": []}

            def train():
                vae.decode(z)

            def parent_train():
                pvae.decode(z)

            def evald():
                vae.decode(z)
            if B > 1:
                for _ in range(3):
                    train()
                    if pvae is not None:
                        parent_train()
            with M.eval_mode(vae):
                for _ in range(3):
                    evald()
            def eval_round():
                with M.eval_mode(vae):
                    return timed(evald, args.inner)
            legs = [("eval", eval_round)]
            if B > 1:                                 # batch statistics of one sample are meaningless: eval only
                legs.append(("train", lambda: timed(train, args.inner)))
                if pvae is not None:
                    legs.append(("parent_train", lambda: timed(parent_train, args.inner)))
            for r in range(args.rounds):              # interleaved, the order rotated round by round
                for name, leg in legs[r % len(legs):] + legs[:r % len(legs)]:
                    runs[name].append(leg())
            entry = {}
            for k, v in runs.items():
                if v:
                    entry[k] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v),
                                "spread_pct": 100 * (max(v) - min(v)) / statistics.median(v)}
            entry["bounds_per_eval_decode"] = count_bounds(vae, z)
            res[f"B{B}"] = entry
    if pscope is not None:
        pscope.__exit__(None, None, None)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
