"""SHA-256 of everything the three MFMA forward kernels of the 5x5 convolutions compute (csrc/conv_igemm.hip,
conv_bf16split.hip, conv_ring.hip behind csrc/conv_tile.hpp) and of the packed filters they read, from seeded inputs: what
a change that must not move a bit is compared by.  A few seconds on the GPU; the largest tensor is about 34 MB.

  igemm      ``ops.CONV_ARITH`` = "fp32", tuning library: the 8 tile variants, forward and transposed, stride 1 and 2,
             packed and plain filters on IGEMM_SHAPES; the statistics entry point on IGEMM_STATS_SHAPES; the transposed
             stride-1 convolution to 3 channels (the thin hand-off without a forced tile, the MFMA tiles with one).
  bf16split  fp16x3, bf16x6 and bf16x3: forward stride 1 under variants -1, 0, 1, 2, 3, 5; transposed stride 1, and stride 2
             with <= 64 output channels, under -1 and 0-6 (6 = quad) on SPLIT_SHAPES; the split-K cases of
             tests/test_kernels_gpu.py::test_conv_fwd_bf16x3_split_k; the ragged quad cases of tests/test_convT_quad_gpu.py
             under variants 6 and 4.
  ring       fp16x3, and bf16x6 / bf16x3 as well: forward and transposed stride 2 under ring variants -1, 0, 1, 2, 3 on
             RING_SHAPES ((1, 256, 256, 8, 8) runs K-split); the affine-input + output-statistics cases of
             test_conv_input_affine_and_output_stats (y and the statistics buffer); the paired transposed path (no knob:
             it engages under variant 2 at PAIRED_SHAPES: 128 workgroups per class, no K split).
  pack       the packed buffers of `vg_conv5x5_pack`, `vg_conv5x5_pack_bf16split` and its multi form: transposed and not,
             stride 1 and 2, 2 / 3 bf16 planes and 2 fp16 planes, filters PACK_FILTERS; spare steps and trailer included
             (the buffers are pre-filled, so a byte the pack leaves alone is part of the digest too).

    conv_bits.py [--tree DIR] [--out out.json]

``--tree``: the checkout whose package is imported (default: this one), so that two commits are compared by one script; the
seeded case generators are this file's: both runs see the same inputs.  Prints one JSON object (with the number of
digests); two runs agree when the objects are equal, and the per-case keys say which kernel moved."""
import argparse, ctypes, hashlib, json, os, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, Cin, Cout, H, W)
IGEMM_SHAPES = ((2, 5, 130, 9, 13), (3, 3, 32, 16, 16), (1, 256, 256, 8, 8))
IGEMM_STATS_SHAPES = ((4, 32, 128, 16, 16), (3, 48, 70, 14, 10))
SPLIT_SHAPES = ((3, 16, 130, 16, 24), (4, 64, 40, 8, 8), (2, 128, 32, 32, 32), (5, 48, 70, 7, 5), (2, 32, 3, 16, 16))
SPLIT_K_SHAPES = ((16, 256, 256, 16, 2), (8, 144, 200, 8, 1), (32, 128, 130, 16, 2))      # (B, Cin, Cout, H = W, stride)
QUAD_EDGES = tuple((B, 16, Cout, Hs, Ws) for B in (1, 3) for (Hs, Ws) in ((8, 32), (9, 33), (5, 7)) for Cout in (32, 20, 1))
RING_SHAPES = ((3, 16, 32, 16, 16), (2, 128, 256, 32, 32), (5, 48, 70, 13, 9), (1, 256, 256, 8, 8), (2, 256, 128, 16, 16))
# (transposed, B, Cin, Cout, H, W, act) of test_conv_input_affine_and_output_stats
FUSED_CASES = ((False, 4, 32, 128, 16, 16, 2), (False, 3, 48, 70, 14, 10, 1), (False, 64, 128, 256, 16, 16, 2),
               (True, 4, 256, 128, 8, 8, 1), (True, 3, 64, 256, 16, 16, 1), (True, 2, 128, 32, 8, 8, 1),
               (False, 2, 3, 8, 16, 16, 0))
PAIRED_SHAPES = ((64, 16, 128, 16, 16), (32, 16, 128, 12, 20))
PACK_FILTERS = ((130, 48), (256, 256))      # (Cout, Cin)
SPLIT_ARITHS = ("fp16x3", "bf16x6", "bf16x3")
PACK_FILL = -12345.5


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        if t is None:
            h.update(b"none")
            continue
        t = t.detach().contiguous().cpu()
        h.update(str((t.dtype, tuple(t.shape))).encode() + t.numpy().tobytes())
    return h.hexdigest()


def operands(torch, B, Cin, Cout, Hs, Ws, transposed, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * Cin + Cout + Hs + Ws + int(transposed))
    x = torch.randn(B, Cin, Hs, Ws, generator=g)
    w = torch.randn(*((Cin, Cout, 5, 5) if transposed else (Cout, Cin, 5, 5)), generator=g) * 0.05
    return x.cuda(), w.cuda(), torch.randn(Cout, generator=g).cuda()


def conv(ops, transposed):
    return ops.convT5x5_fwd if transposed else ops.conv5x5_fwd


def run_igemm(torch, ops, lib):
    out = {}
    ops.CONV_ARITH = "fp32"
    try:
        for variant in range(8):
            lib.vg_debug_set_conv_tile(0, variant)
            lib.vg_debug_set_conv_tile(1, variant)
            for shape in IGEMM_SHAPES:
                for tr in (False, True):
                    x, w, bias = operands(torch, *shape, tr)
                    for stride in (1, 2):
                        for ops.USE_PACKED_FILTERS in (True, False):
                            key = f"v{variant}/{shape}/tr{int(tr)}/s{stride}/packed{int(ops.USE_PACKED_FILTERS)}"
                            out[key] = sha(conv(ops, tr)(x, w, bias, stride))
            ops.USE_PACKED_FILTERS, ops.FP32_CONV_STATS = True, True
            for shape in IGEMM_STATS_SHAPES:
                x, w, bias = operands(torch, *shape, False)
                for stride in (1, 2):
                    y, stats = ops.conv5x5_fwd(x, w, bias, stride, want_stats=True)
                    assert stats is not None
                    out[f"v{variant}/stats/{shape}/s{stride}"] = sha(y, stats)
            ops.FP32_CONV_STATS = False
        for variant in (-1, 0, 3, 6, 7):     # 32 -> 3 channels, transposed stride 1: thin hand-off / MFMA tiles
            lib.vg_debug_set_conv_tile(1, variant)
            x, w, bias = operands(torch, 2, 32, 3, 16, 16, True)
            out[f"v{variant}/thin_handoff"] = sha(ops.convT5x5_fwd(x, w, bias, 1))
    finally:
        ops.USE_PACKED_FILTERS, ops.FP32_CONV_STATS = True, False
        lib.vg_debug_set_conv_tile(0, -1)
        lib.vg_debug_set_conv_tile(1, -1)
    return out


def run_bf16split(torch, ops, lib):
    out = {}
    try:
        for ops.CONV_ARITH in SPLIT_ARITHS:
            a = ops.CONV_ARITH
            for shape in SPLIT_SHAPES:
                Cout = shape[2]
                x, w, bias = operands(torch, *shape, False)
                xt, wt, biast = operands(torch, *shape, True)
                for variant in (-1, 0, 1, 2, 3, 4, 5, 6):
                    lib.vg_debug_set_conv_bf16split_tile(variant)
                    if variant not in (4, 6):
                        out[f"{a}/fwd/s1/{shape}/v{variant}"] = sha(ops.conv5x5_fwd(x, w, bias, 1))
                    if Cout > 4:        # (<= 4 channels at stride 1: the thin kernels, not these files)
                        out[f"{a}/tr/s1/{shape}/v{variant}"] = sha(ops.convT5x5_fwd(xt, wt, biast, 1))
                    if Cout <= 64:
                        out[f"{a}/tr/s2/{shape}/v{variant}"] = sha(ops.convT5x5_fwd(xt, wt, biast, 2))
            lib.vg_debug_set_conv_bf16split_tile(-1)
            for (B, Cin, Cout, Hs, s) in SPLIT_K_SHAPES:
                x, w, bias = operands(torch, B, Cin, Cout, Hs, Hs, False)
                out[f"{a}/split_k/{(B, Cin, Cout, Hs, s)}"] = sha(ops.conv5x5_fwd(x, w, bias, s))
            if a == "bf16x6":
                continue                # the quad form has two planes
            for shape in QUAD_EDGES:
                xt, wt, biast = operands(torch, *shape, True)
                for variant in (6, 4):
                    lib.vg_debug_set_conv_bf16split_tile(variant)
                    out[f"{a}/quad/{shape}/v{variant}"] = sha(ops.convT5x5_fwd(xt, wt, biast, 2))
    finally:
        lib.vg_debug_set_conv_bf16split_tile(-1)
    return out


def run_ring(torch, ops, lib):
    out = {}
    try:
        for ops.CONV_ARITH in SPLIT_ARITHS:
            a = ops.CONV_ARITH
            for variant in (-1, 0, 1, 2, 3):
                lib.vg_debug_set_conv_ring_tile(variant)
                for shape in RING_SHAPES:
                    for tr in (False, True):
                        x, w, bias = operands(torch, *shape, tr)
                        out[f"{a}/v{variant}/{shape}/tr{int(tr)}"] = sha(conv(ops, tr)(x, w, bias, 2))
                for (tr, B, Cin, Cout, Hs, Ws, act) in FUSED_CASES:
                    x, w, bias = operands(torch, B, Cin, Cout, Hs, Ws, tr, seed=1)
                    g = torch.Generator().manual_seed(70 + Cin)
                    scale, shift = (0.5 + torch.rand(Cin, generator=g)).cuda(), torch.randn(Cin, generator=g).cuda()
                    y, stats = conv(ops, tr)(x, w, bias, 2, in_affine=(scale, shift, act), want_stats=True)
                    out[f"{a}/v{variant}/fused/{(tr, B, Cin, Cout, Hs, Ws, act)}"] = sha(y, stats)
            lib.vg_debug_set_conv_ring_tile(2)
            for shape in PAIRED_SHAPES:
                x, w, bias = operands(torch, *shape, True)
                out[f"{a}/paired/{shape}"] = sha(ops.convT5x5_fwd(x, w, bias, 2))
    finally:
        lib.vg_debug_set_conv_ring_tile(-1)
    return out


def run_pack(torch, ops, _lib, lib):
    out = {}
    stream = ops._stream()
    filters = []
    for (Cout, Cin) in PACK_FILTERS:
        for tr in (0, 1):
            g = torch.Generator().manual_seed(5 + Cout + Cin + tr)
            filters.append((Cout, Cin, tr, (torch.randn(*((Cin, Cout) if tr else (Cout, Cin)), 5, 5, generator=g) * 0.05).cuda()))
    for (Cout, Cin, tr, w) in filters:
        for stride in (1, 2):
            p = torch.full((lib.vg_conv5x5_packed_floats(Cout, Cin),), PACK_FILL, dtype=torch.float32, device="cuda")
            _lib.check(lib.vg_conv5x5_pack(w.data_ptr(), p.data_ptr(), Cout, Cin, tr, stride, stream), "vg_conv5x5_pack")
            out[f"fp32/{(Cout, Cin)}/tr{tr}/s{stride}"] = sha(p)
    for planes, name in ((2, "bf16x2"), (3, "bf16x3planes"), (2 | ops.PLANES_F16, "fp16x2")):
        f16 = bool(planes & ops.PLANES_F16)
        cases = [(Cout, Cin, tr, w, stride) for (Cout, Cin, tr, w) in filters for stride in (1, 2)]
        slots, single, multi = [], [], []
        arr = (_lib.PackEntry * len(cases))()
        for i, (Cout, Cin, tr, w, stride) in enumerate(cases):
            slot = None
            if f16:
                slot = torch.zeros(1, device="cuda")
                _lib.check(lib.vg_absmax(w.data_ptr(), w.numel(), slot.data_ptr(), stream), "vg_absmax")
            slots.append(slot)
            n = lib.vg_conv5x5_packed_bf16split_bytes(Cout, Cin, planes) // 4
            single.append(torch.full((n,), PACK_FILL, dtype=torch.float32, device="cuda"))
            multi.append(torch.full((n,), PACK_FILL, dtype=torch.float32, device="cuda"))
            _lib.check(lib.vg_conv5x5_pack_bf16split(w.data_ptr(), single[i].data_ptr(), Cout, Cin, tr, stride, planes,
                                                     ops._ptr(slot), stream), "vg_conv5x5_pack_bf16split")
            arr[i] = _lib.PackEntry(w.data_ptr(), multi[i].data_ptr(), Cout, Cin, tr, stride, ops._ptr(slot))
        _lib.check(lib.vg_conv5x5_pack_bf16split_multi(arr, len(cases), planes, stream), "vg_conv5x5_pack_bf16split_multi")
        for i, (Cout, Cin, tr, _w, stride) in enumerate(cases):
            out[f"{name}/{(Cout, Cin)}/tr{tr}/s{stride}"] = sha(single[i])
            out[f"{name}/{(Cout, Cin)}/tr{tr}/s{stride}/multi"] = sha(multi[i])
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
        raise SystemExit("conv_bits.py runs the kernels: it needs the GPU")
    arith = ops.CONV_ARITH
    try:
        with _lib.use_tuning() as lib:
            res = {"igemm": run_igemm(torch, ops, lib), "bf16split": run_bf16split(torch, ops, lib),
                   "ring": run_ring(torch, ops, lib), "pack": run_pack(torch, ops, _lib, lib)}
    finally:
        ops.CONV_ARITH = arith
    res["digests"] = sum(len(v) for v in res.values())
    text = json.dumps(res, indent=1, sort_keys=True)
    res["sha256_of_all"] = hashlib.sha256(text.encode()).hexdigest()
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
