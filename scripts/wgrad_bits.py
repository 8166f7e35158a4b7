"""SHA-256 of everything the weight-gradient kernels and the <= 3-channel convolution kernels compute (csrc/conv_wgrad.hip,
wgrad_bf16split.hip, conv_thin_wgrad.hip, conv_thin_fwd.hip, conv_thin_mfma.hip), from seeded inputs: what a change that
must not move a bit is compared by.  The companion of conv_bits.py (the MFMA forward kernels); a few seconds on the GPU.

  fp32     ``ops.CONV_ARITH`` = "fp32", tuning library: FP32_SHAPES under every row-tile form the shape can take (128 rows
           with the 8-wave K split, 4-wave, 10-channel column tile; 64; 32) x both gy load paths at a split whose last slab
           is short, then the one-slab, slab-per-chunk and planned splits -- the enumeration of
           tests/test_wgrad_gpu.py::test_fp32_every_plan; the key carries the plan the library reports.
  split    fp16x3 (operands far from 1), bf16x6, bf16x3: SPLIT_SHAPES x forced chunk heights; the affine-on-load case on x
           and on gy with the three activations, both chunk heights.
  thin     thin weight gradient: THIN_SHAPES, three planes (fp16x3) and two (bf16x3), plain and with the affine on gy.
  acc      ACC_CASES: the plain call, ``out=`` prefilled with NaN and ``accumulate=True``, aligned and 4 (mod 16) bytes
           off -- each of the four slab reducers and wx_reduce_kernel.
  thin_fwd / thin_tr   the shapes of tests/test_kernels_gpu.py::test_conv_thin_split (y and the statistics slots, with
           and without bias) and ::test_convT_thin_split (plain and affine with each activation), two and three planes.

    wgrad_bits.py [--tree DIR] [--out out.json] [--time ROUNDS]

``--tree``: the checkout whose package is imported (default: this one), so that two commits are compared by one script;
the seeded case generators are this file's: both runs see the same inputs.  Prints one JSON object (with the number of
digests); two runs agree when the objects are equal, and the per-case keys say which kernel moved.
``--time ROUNDS``: no digests; the median over ROUNDS rounds of the mean time of 40 launches, in microseconds, of the
weight gradient at each benchmarked layer (B = 128, default arithmetic, the trainer's operand transform) and of the thin
forward / transposed kernels at the benchmark's shapes."""
import argparse, ctypes, hashlib, json, os, statistics, sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOB_DEFAULTS = {"tm": -1, "target": -1, "ks": 2, "cit": 5, "vec4": 1, "th": 0}
KNOB_IDS = {"tm": 0, "target": 1, "ks": 2, "cit": 3, "vec4": 4, "th": 5}
PLANES = {"bf16x3": 2, "bf16x6": 3, "fp16x3": 2 | 0x100}
FP32_FORMS = ((128, 2, 5), (128, 1, 5), (128, 1, 10), (64, 1, 5), (32, 1, 5))      # (tm, ks, cit) of the dispatch switch
# (B, Cin, Cout, H, W, stride): the tables of tests/test_wgrad_gpu.py
FP32_SHAPES = ((5, 21, 130, 11, 8, 1), (7, 21, 130, 13, 15, 2), (5, 21, 130, 6, 16, 1), (5, 21, 130, 10, 24, 2),
               (3, 21, 130, 5, 32, 1), (5, 21, 130, 6, 56, 2), (3, 21, 130, 3, 72, 1), (3, 21, 130, 5, 136, 2),
               (1, 3, 33, 9, 7, 1), (5, 7, 65, 7, 13, 1), (3, 12, 65, 9, 21, 2), (2, 9, 33, 5, 54, 2),
               (1, 5, 33, 2, 256, 1), (1, 6, 40, 3, 256, 2), (2, 4, 70, 3, 130, 1))
SPLIT_SHAPES = (((1, 32, 40, 7, 8, 1), (1,)), ((15, 33, 130, 8, 16, 2), (1, 2)), ((17, 37, 128, 6, 16, 1), (1, 2)),
                ((16, 32, 33, 4, 16, 2), (1, 2)), ((33, 65, 260, 13, 8, 1), (1,)), ((33, 48, 130, 12, 16, 1), (1, 2)),
                ((17, 64, 200, 20, 16, 2), (1, 2)))
SPLIT_AFFINE_SHAPE = (17, 35, 70, 8, 16, 2)
THIN_SHAPES = ((130, 1, 33, 40, 16, 1), (3, 2, 50, 80, 32, 2), (5, 3, 20, 37, 32, 1), (2, 3, 32, 70, 64, 2), (2, 3, 63, 20, 16, 1))
# (family / arithmetic, shape, out 4 (mod 16) bytes off)
ACC_CASES = (("fp32", (2, 8, 16, 8, 8, 1), False), ("fp32", (70, 4, 8, 8, 8, 1), False), ("fp32", (70, 4, 8, 8, 8, 1), True),
             ("fp32", (3, 3, 3, 8, 8, 2), False), ("fp32", (66, 41, 64, 8, 8, 1), False), ("fp32", (17, 8, 16, 8, 8, 1), False),
             ("fp32", (2, 8, 16, 8, 8, 1), True), ("fp32", (17, 8, 16, 8, 8, 1), True), ("fp32", (5, 21, 130, 13, 15, 2), True),
             ("fp16x3", (17, 37, 128, 6, 16, 1), False), ("fp16x3", (17, 37, 128, 6, 16, 1), True),
             ("fp16x3", (33, 65, 260, 13, 8, 1), True), ("bf16x6", (17, 37, 128, 6, 16, 1), True),
             ("bf16x6", (15, 33, 130, 8, 16, 2), False), ("bf16x3", (15, 33, 130, 8, 16, 2), True),
             ("thin", (5, 3, 20, 37, 32, 1), False), ("thin", (130, 1, 33, 40, 16, 1), False), ("thin", (3, 1, 33, 40, 16, 1), False),
             ("thin", (5, 3, 20, 37, 32, 1), True), ("thin", (3, 1, 33, 40, 16, 1), True), ("thin", (130, 1, 33, 40, 16, 1), True))
# (B, Cin, Cout, H, W, stride) of test_conv_thin_split; (B, Cout, H, W) of test_convT_thin_split
THIN_FWD_SHAPES = ((3, 3, 32, 64, 64, 1), (2, 3, 64, 64, 64, 2), (2, 1, 32, 9, 32, 1), (1, 2, 20, 5, 64, 1), (2, 3, 70, 14, 128, 2),
                   (1, 3, 32, 30, 256, 1), (2, 3, 64, 128, 128, 2))
THIN_TR_SHAPES = ((3, 3, 64, 64), (2, 3, 21, 16), (2, 1, 5, 48), (1, 2, 40, 128), (5, 3, 1, 32))
# (transposed, Cin, Cout, H, stride, activation of the producer's BatchNorm or None): BENCH_LAYERS of tests/test_wgrad_gpu.py
BENCH_LAYERS = ((False, 3, 64, 64, 2, None), (False, 64, 128, 32, 2, 1), (False, 128, 256, 16, 2, 1), (False, 3, 32, 64, 1, None),
                (False, 32, 128, 64, 2, 2), (False, 128, 256, 32, 2, 2), (False, 256, 256, 16, 2, 2), (True, 256, 256, 8, 2, None),
                (True, 256, 128, 16, 2, 1), (True, 128, 32, 32, 2, 1), (True, 32, 3, 64, 1, 1))


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        if t is None:
            h.update(b"none")
            continue
        t = t.detach().contiguous().cpu()
        h.update(str((t.dtype, tuple(t.shape))).encode() + t.numpy().tobytes())
    return h.hexdigest()


def out_hw(Hs, Ws, S):
    return (Hs - 1) // S + 1, (Ws - 1) // S + 1


def operands(torch, shape, seed, x_mag=1.0, gy_mag=1.0):
    B, Cin, Cout, Hs, Ws, S = shape
    g = torch.Generator().manual_seed(seed)
    OH, OW = out_hw(Hs, Ws, S)
    x = torch.randn(B, Cin, Hs, Ws, generator=g) * x_mag
    return x.cuda(), (torch.randn(B, Cout, OH, OW, generator=g) * gy_mag).cuda()


def affine(torch, C, seed, mag=1.0):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + torch.rand(C, generator=g)).cuda(), (torch.randn(C, generator=g) * mag).cuda()


def mags(arith):
    return (3e3, 1e-5) if arith == "fp16x3" else (1.0, 1.0)


def set_knobs(lib, **kw):
    for name, default in KNOB_DEFAULTS.items():
        assert lib.vg_debug_set_wgrad(KNOB_IDS[name], kw.get(name, default)) == 0


def plan_fp32(lib, shape):
    B, Cin, Cout, Hs, Ws, S = shape
    o = (ctypes.c_int * 9)()
    assert lib.vg_debug_wgrad_plan(B, Cin, Hs, Ws, Cout, S, 0, 0, 0, o) == 0
    return dict(zip(("tw", "tm", "cit", "ks", "splits", "vec4", "reducer", "chunks", "cps"), o))


def plan_split(lib, shape, arith):
    B, Cin, Cout, Hs, Ws, S = shape
    o = (ctypes.c_int * 9)()
    assert lib.vg_debug_wgrad_split_plan(B, Cin, Hs, Ws, Cout, S, PLANES[arith], o) == 0, (shape, "not taken")
    return dict(zip(("th", "wco", "mtiles", "ntiles", "units", "upw", "wgs", "pieces", "chunks"), o))


def fp32_runs(lib, shape):
    """The knob settings of test_fp32_every_plan, each with the plan the library reports for it."""
    runs, seen = [], set()

    def add(**kn):
        set_knobs(lib, **kn)
        p = plan_fp32(lib, shape)
        key = tuple(sorted(p.items()))
        if key not in seen:
            seen.add(key)
            runs.append((kn, p))

    OW = out_hw(shape[3], shape[4], shape[5])[1]
    for tm, ks, cit in sorted(FP32_FORMS):
        form = dict(tm=tm, ks=ks, cit=cit)
        set_knobs(lib, **form)
        p = plan_fp32(lib, shape)
        if (p["tm"], p["ks"], p["cit"]) != (tm, ks, cit):
            continue
        target = None
        for t in range(2, 2048):
            lib.vg_debug_set_wgrad(KNOB_IDS["target"], t)
            q = plan_fp32(lib, shape)
            if q["splits"] > 1 and q["chunks"] % q["cps"]:
                target = t
                break
        for vec4 in ((1, 0) if OW % 4 == 0 else (1,)):
            add(vec4=vec4, **({"target": target} if target else {}), **form)
    add(target=1)
    add(target=1 << 20)
    add()
    set_knobs(lib)
    return runs


def tag(d):
    return ",".join(f"{k}={v}" for k, v in sorted(d.items()))


def run_fp32(torch, ops, lib):
    out = {}
    ops.CONV_ARITH = "fp32"
    for shape in FP32_SHAPES:
        x, gy = operands(torch, shape, 100)
        for kn, p in fp32_runs(lib, shape):
            set_knobs(lib, **kn)
            out[f"{shape}/{tag(p)}"] = sha(ops.conv5x5_wgrad(x, gy, shape[5]))
    set_knobs(lib)
    return out


def run_split(torch, ops, lib):
    out = {}
    for arith in ("fp16x3", "bf16x6", "bf16x3"):
        ops.CONV_ARITH = arith
        xm, gm = mags(arith)
        for shape, ths in SPLIT_SHAPES:
            x, gy = operands(torch, shape, 200, xm, gm)
            for th in ths:
                set_knobs(lib, th=th)
                p = plan_split(lib, shape, arith)
                assert p["th"] == th, (shape, th, p)
                out[f"{arith}/{shape}/{tag(p)}"] = sha(ops.conv5x5_wgrad(x, gy, shape[5]))
        shape = SPLIT_AFFINE_SHAPE
        x, gy = operands(torch, shape, 210, xm, gm)
        for th in (1, 2):
            set_knobs(lib, th=th)
            assert plan_split(lib, shape, arith)["th"] == th
            for on_gy in (False, True):
                scale, shift = affine(torch, shape[2] if on_gy else shape[1], 211 + int(on_gy), gm if on_gy else xm)
                for act in (0, 1, 2):
                    got = ops.conv5x5_wgrad(x, gy, shape[5], in_affine=(scale, shift, act), affine_on_gy=on_gy)
                    out[f"{arith}/affine/th{th}/{'gy' if on_gy else 'x'}/act{act}"] = sha(got)
    set_knobs(lib)
    return out


def run_thin(torch, ops, lib):
    out = {}
    for arith in ("fp16x3", "bf16x3"):      # three planes, two planes
        ops.CONV_ARITH = arith
        for shape in THIN_SHAPES:
            B, Cin, Cout, Hs, Ws, S = shape
            assert lib.vg_conv5x5_thin_wgrad_bf16split_workspace_bytes(B, Cin, Hs, Ws, Cout, S, ops._thin_planes()) > 0
            x, gy = operands(torch, shape, 300)
            out[f"{arith}/{shape}/plain"] = sha(ops.conv5x5_wgrad(x, gy, S))
            scale, shift = affine(torch, Cout, 301)
            for act in (0, 1, 2):
                got = ops.conv5x5_wgrad(x, gy, S, in_affine=(scale, shift, act), affine_on_gy=True)
                out[f"{arith}/{shape}/affine/act{act}"] = sha(got)
    return out


def run_acc(torch, ops, lib):
    out = {}
    for family, shape, misaligned in ACC_CASES:
        ops.CONV_ARITH = "fp16x3" if family == "thin" else family
        B, Cin, Cout, Hs, Ws, S = shape
        n = Cout * Cin * 25
        x, gy = operands(torch, shape, 400)
        flat_init = torch.randn(n + 8, generator=torch.Generator().manual_seed(401)).cuda()
        off = 1 if misaligned else 4

        def view(flat):
            v = flat[off:off + n].view(Cout, Cin, 5, 5)
            assert v.data_ptr() % 16 == (4 if misaligned else 0)
            return v

        key = f"{family}/{shape}/{'off4' if misaligned else 'aligned'}"
        out[key + "/plain"] = sha(ops.conv5x5_wgrad(x, gy, S))
        flat = flat_init.clone()
        view(flat).fill_(float("nan"))
        ops.conv5x5_wgrad(x, gy, S, out=view(flat))
        out[key + "/out"] = sha(flat)
        flat = flat_init.clone()
        ops.conv5x5_wgrad(x, gy, S, out=view(flat), accumulate=True)
        out[key + "/accumulate"] = sha(flat)
    return out


def run_thin_fwd(torch, ops, lib):
    out = {}
    for arith in ("fp16x3", "bf16x3"):
        ops.CONV_ARITH = arith
        for shape in THIN_FWD_SHAPES:
            B, Cin, Cout, Hs, Ws, S = shape
            assert lib.vg_conv5x5_thin_bf16split_ok(Cin, Hs, Ws, Cout, S) == 1
            g = torch.Generator().manual_seed(91)
            x = torch.randn(B, Cin, Hs, Ws, generator=g).cuda()
            w = (torch.randn(Cout, Cin, 5, 5, generator=g) * 0.1).cuda()
            bias = torch.randn(Cout, generator=g).cuda()
            y, stats = ops.conv5x5_fwd(x, w, bias, S, want_stats=True)
            assert stats is not None
            out[f"{arith}/{shape}"] = sha(y, stats)
            out[f"{arith}/{shape}/no_bias"] = sha(ops.conv5x5_fwd(x, w, None, S))
    return out


def run_thin_tr(torch, ops, lib):
    out = {}
    for arith in ("fp16x3", "bf16x3"):
        ops.CONV_ARITH = arith
        for shape in THIN_TR_SHAPES:
            B, Cout, Hs, Ws = shape
            assert lib.vg_convT5x5_s1_thin_bf16split_ok(32, Hs, Ws, Cout) == 1
            g = torch.Generator().manual_seed(90)
            x = torch.randn(B, 32, Hs, Ws, generator=g).cuda()
            w = (torch.randn(32, Cout, 5, 5, generator=g) * 0.05).cuda()
            bias = torch.randn(Cout, generator=g).cuda()
            out[f"{arith}/{shape}/plain"] = sha(ops.convT5x5_fwd(x, w, bias, 1))
            scale, shift = affine(torch, 32, 92)
            for act in (0, 1, 2):
                out[f"{arith}/{shape}/affine/act{act}"] = sha(ops.convT5x5_fwd(x, w, bias, 1, in_affine=(scale, shift, act)))
    return out


def run_times(torch, ops, rounds):
    """Median over `rounds` rounds of the mean time of 40 launches, microseconds."""
    def timeit(fn):
        for _ in range(60):
            fn()                               # the clock takes tens of launches to settle after idle
        torch.cuda.synchronize()
        ts = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(40):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / 40 * 1e3)
        return round(statistics.median(ts), 2)

    out, B = {}, 128
    gen = torch.Generator(device="cuda").manual_seed(600)
    for (tr, Cin, Cout, Hs, s, act) in BENCH_LAYERS:
        if tr:      # the layer's input is the wide "gy" operand; the gradient of its output plays x
            a = torch.randn(B, Cout, s * Hs, s * Hs, device="cuda", generator=gen)
            b = torch.randn(B, Cin, Hs, Hs, device="cuda", generator=gen)
        else:
            a = torch.randn(B, Cin, Hs, Hs, device="cuda", generator=gen)
            b = torch.randn(B, Cout, (Hs - 1) // s + 1, (Hs - 1) // s + 1, device="cuda", generator=gen)
        kw = {}
        if act is not None:
            scale, shift = 0.5 + torch.rand(Cin, device="cuda", generator=gen), torch.randn(Cin, device="cuda", generator=gen)
            kw = dict(in_affine=(scale, shift, act), affine_on_gy=tr)
        out[f"wgrad {'convT' if tr else 'conv'} {Cin}->{Cout} @{Hs} s{s}"] = timeit(lambda: ops.conv5x5_wgrad(a, b, s, **kw))
    for (Cout, s) in ((32, 1), (64, 2)):
        x = torch.randn(B, 3, 64, 64, device="cuda", generator=gen)
        w = torch.randn(Cout, 3, 5, 5, device="cuda", generator=gen) * 0.1
        bias = torch.randn(Cout, device="cuda", generator=gen)
        out[f"thin fwd 3->{Cout} @64 s{s}"] = timeit(lambda: ops.conv5x5_fwd(x, w, bias, s, want_stats=True))
    x = torch.randn(B, 32, 64, 64, device="cuda", generator=gen)
    w = torch.randn(32, 3, 5, 5, device="cuda", generator=gen) * 0.05
    bias = torch.randn(3, device="cuda", generator=gen)
    scale, shift = 0.5 + torch.rand(32, device="cuda", generator=gen), torch.randn(32, device="cuda", generator=gen)
    out["thin convT 32->3 @64 s1"] = timeit(lambda: ops.convT5x5_fwd(x, w, bias, 1, in_affine=(scale, shift, 1)))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--out")
    ap.add_argument("--time", type=int, default=0, metavar="ROUNDS")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    import torch
    from disentangle_mlp_amd import _lib, ops
    assert os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__))) == tree
    if not torch.cuda.is_available():
        raise SystemExit("wgrad_bits.py runs the kernels: it needs the GPU")
    arith = ops.CONV_ARITH
    if a.time:
        res = {"tree": tree, "arith": arith, "us": run_times(torch, ops, a.time)}
    else:
        try:
            with _lib.use_tuning() as lib:
                try:
                    res = {"fp32": run_fp32(torch, ops, lib), "split": run_split(torch, ops, lib), "thin": run_thin(torch, ops, lib),
                           "acc": run_acc(torch, ops, lib), "thin_fwd": run_thin_fwd(torch, ops, lib),
                           "thin_tr": run_thin_tr(torch, ops, lib)}
                finally:
                    set_knobs(lib)
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
