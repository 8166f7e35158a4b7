#!/usr/bin/env python
"""One SHA-256 over every host-side answer of the 5x5 convolution launchers (conv_ring.hip, conv_bf16split.hip,
conv_igemm.hip) on a fixed sweep of shapes and tuning knobs: workspace bytes, statistics floats, fusability and the
ring's route.  Host queries only -- nothing is launched, no GPU is needed.  Two builds whose digests agree size every
buffer, pick every tile and split every K alike on the sweep:

    python scripts/conv_plan_digest.py [path/to/libvaegan_hip_tuning.so] [--jobs N]
"""
import argparse
import ctypes
import hashlib
import itertools
import multiprocessing
import os
import struct

BS = (1, 2, 3, 8, 128)
CINS = (16, 32, 256)
HWS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64)
COUTS = (1, 32, 33, 64, 65, 128, 129, 256, 257)
STRIDES = (1, 2)
MODES = (0, 1)
PLANES = (2, 3, 2 | 0x100)          # VG_PLANES_F16
RING_VARIANTS = (-1, 0, 1, 2, 3)
X_TILES = (-1, 0, 1, 2, 3, 4, 5, 6)

_I, _Z = ctypes.c_int, ctypes.c_size_t


def _load(path):
    lib = ctypes.CDLL(path)
    for name in ("vg_conv5x5_fwd_bf16split_workspace_bytes", "vg_convT5x5_fwd_bf16split_workspace_bytes",
                 "vg_conv5x5_fwd_bf16split_stats_floats", "vg_convT5x5_fwd_bf16split_stats_floats"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _Z, [_I] * 7
    lib.vg_conv5x5_bf16split_fusable.restype, lib.vg_conv5x5_bf16split_fusable.argtypes = _I, [_I] * 4
    lib.vg_conv5x5_fwd_packed_stats_floats.restype, lib.vg_conv5x5_fwd_packed_stats_floats.argtypes = _Z, [_I] * 6
    lib.vg_debug_ring_route.restype, lib.vg_debug_ring_route.argtypes = _I, [_I] * 7 + [ctypes.POINTER(_I)]
    for name in ("vg_debug_set_conv_ring_tile", "vg_debug_set_conv_bf16split_tile"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _I, [_I]
    return lib


def _walk(job):
    """Digest of the whole shape sweep under one (forced ring variant, forced bf16split tile)."""
    path, ring_variant, x_tile = job
    lib = _load(path)
    lib.vg_debug_set_conv_ring_tile(ring_variant)
    lib.vg_debug_set_conv_bf16split_tile(x_tile)
    ws = (lib.vg_conv5x5_fwd_bf16split_workspace_bytes, lib.vg_convT5x5_fwd_bf16split_workspace_bytes)
    st = (lib.vg_conv5x5_fwd_bf16split_stats_floats, lib.vg_convT5x5_fwd_bf16split_stats_floats)
    fusable, packed, route = lib.vg_conv5x5_bf16split_fusable, lib.vg_conv5x5_fwd_packed_stats_floats, lib.vg_debug_ring_route
    out = (_I * 6)()
    pack = struct.Struct("<QQQQiQi6i").pack
    h = hashlib.sha256()
    for B, Cin, H, W, Cout, S, mode, planes in itertools.product(BS, CINS, HWS, HWS, COUTS, STRIDES, MODES, PLANES):
        for i in range(6):
            out[i] = -7           # (a refused route leaves its words alone)
        shape = (B, Cin, H, W, Cout, S, planes)
        h.update(pack(ws[0](*shape), ws[1](*shape), st[0](*shape), st[1](*shape), fusable(mode, Cin, Cout, S),
                      packed(B, Cin, H, W, Cout, S), route(mode, B, Cin, H, W, Cout, planes, out), *out))
    lib.vg_debug_set_conv_ring_tile(-1)
    lib.vg_debug_set_conv_bf16split_tile(-1)
    return h.digest()


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib", nargs="?", default=os.path.join(here, "..", "disentangle_mlp_amd", "libvaegan_hip_tuning.so"))
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    jobs = [(os.path.abspath(a.lib), r, x) for r in RING_VARIANTS for x in X_TILES]
    with multiprocessing.Pool(a.jobs) as pool:
        parts = pool.map(_walk, jobs)         # in the order of `jobs`, whatever the process count
    shapes = len(BS) * len(CINS) * len(HWS) ** 2 * len(COUTS) * len(STRIDES) * len(MODES) * len(PLANES)
    print(f"{hashlib.sha256(b''.join(parts)).hexdigest()}  {len(jobs)} knob settings x {shapes} shapes, 13 words each")


if __name__ == "__main__":
    main()
