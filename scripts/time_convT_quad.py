"""Stride-2 transposed convolution with <= 32 output channels (conv_bf16split.hip): tile variant 4 (one workgroup per parity
class) against 6 (quad: all four classes per workgroup) over shapes on both sides of the dispatch rule, forced through the
tuning build; 15 interleaved rounds of 4 launches each, medians and min / max in us per launch.  Prints one
JSON line per shape; with a file name as its argument, writes the list there too."""
import json, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from disentangle_mlp_amd import ops as H, _lib

shapes = [  # B, Cin, H, W, Cout
    (128, 128, 32, 32, 32), (8, 16, 64, 64, 32), (8, 128, 64, 64, 32), (32, 128, 32, 32, 32), (16, 32, 64, 64, 20),
    (64, 128, 32, 32, 32), (128, 32, 32, 32, 32), (128, 128, 32, 32, 3), (32, 64, 64, 64, 32), (4, 64, 128, 128, 16)]
out = []
with _lib.use_tuning() as lib:
    for B, Cin, Hs, Ws, Cout in shapes:
        x = torch.randn(B, Cin, Hs, Ws, device="cuda")
        w = torch.randn(Cin, Cout, 5, 5, device="cuda") * 0.05
        b = torch.randn(Cout, device="cuda")
        H.amax_of(x)
        t = {4: [], 6: []}
        with H.packed_filter_scope():
            for v in (4, 6):
                lib.vg_debug_set_conv_bf16split_tile(v)
                for _ in range(3):
                    H.convT5x5_fwd(x, w, b, 2)
            for rep in range(15):
                for v in (4, 6):
                    lib.vg_debug_set_conv_bf16split_tile(v)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(4):
                        H.convT5x5_fwd(x, w, b, 2)
                    e1.record()
                    torch.cuda.synchronize()
                    t[v].append(e0.elapsed_time(e1) * 1e3 / 4)
        lib.vg_debug_set_conv_bf16split_tile(-1)
        px = B * Hs * Ws
        r = {"B": B, "Cin": Cin, "H": Hs, "W": Ws, "Cout": Cout, "input_pixels": px, "quad_workgroups": -(-Hs // 8) * -(-Ws // 32) * B,
             "per_class_us": round(statistics.median(t[4]), 1), "quad_us": round(statistics.median(t[6]), 1),
             "per_class_min_max": [round(min(t[4]), 1), round(max(t[4]), 1)], "quad_min_max": [round(min(t[6]), 1), round(max(t[6]), 1)]}
        print(json.dumps(r), flush=True)
        out.append(r)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
