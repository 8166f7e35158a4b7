"""Tensor-level wrappers over the C-ABI HIP library (include/vaegan_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every
arithmetic op below runs in libvaegan_hip.so.  Inputs must be CUDA (ROCm) fp32
tensors -- there is deliberately no CPU path.
"""
import ctypes
import math
import os
import weakref
from typing import NamedTuple

import torch

from . import _lib
from ._lib import check

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
EW_LRELU, EW_TANH, EW_SIGMOID = 0, 1, 2

_workspaces = {}

# Optional launch timing (bench.py): when set to a dict, every convolution launch whose
# key passes `_timing_filter` is bracketed by HIP events on the launch stream.
_timing = None
_timing_filter = None


def start_timing(only=None):
    """Collect (start, end) HIP-event pairs per convolution launch key; ``only`` restricts
    collection to one key (dominant-kernel timing inside the timed region)."""
    global _timing, _timing_filter
    _timing, _timing_filter = {}, only


def stop_timing():
    """Returns {key: [ms, ...]} (synchronises)."""
    global _timing, _timing_filter
    t, _timing, _timing_filter = _timing, None, None
    if not t:
        return {}
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in t.items()}


class _timed:
    __slots__ = ("key", "a")

    def __init__(self, key):
        self.key = key if (_timing is not None and (_timing_filter is None or _timing_filter == key)) else None

    def __enter__(self):
        if self.key is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if self.key is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _timing.setdefault(self.key, []).append((self.a, b))
        return False


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _req(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: disentangle_mlp_amd ops need CUDA/ROCm tensors (no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: tensor must be contiguous")
    return t


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def workspace(nbytes, device):
    """Scratch per (device, stream), grown on demand: kernels launched on one stream are ordered, so
    one buffer serves every two-stage reduction / split-K slab of that stream in turn; work on
    another stream (a side stream, a second trainer thread) gets its own."""
    key = (device.type, device.index, _stream())
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        nbytes = max(int(nbytes), 1 << 20)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def reserve_workspace(nbytes, device):
    """Pre-size the scratch buffer (call before HIP-graph capture)."""
    return workspace(nbytes, device)


# ---------------------------------------------------------------- convolutions
# Packed filters (vg_conv5x5_pack): the implicit-GEMM kernels read the filter as
# [class][ci][tap][cout].  Outside a `packed_filter_scope` every launch re-packs its weight
# (a few microseconds); inside one -- the trainer opens it around an iteration, where it
# alone decides when weights change -- a pack is reused until `invalidate_packed_filters()`.  It belongs
# to the weight tensor OBJECT (`_WeightRecord`), not to its address, and lives as long as that.
USE_PACKED_FILTERS = True
FP32_CONV_STATS = False     # see route_conv
# Arithmetic of the three convolution kernels (forward, transposed = data gradient, weight gradient):
#   "fp16x3"  the product DEFAULT: every fp32 operand, times an exact power of two taken from a bound of the tensor's
#             largest magnitude, split into fp16 hi + lo (11 + 11 significand bits, residual <= 2^-24), the 3 plane
#             products hi*hi, hi*lo, lo*hi on the f16 MFMA, fp32 accumulation, scales undone on the accumulators:
#             fp32-equivalent (4e-7..6e-7 vs fp64 per convolution) at half the matrix work of bf16x6.  The bounds live in
#             device memory (`amax_of`, producers emit them: bn_act_bwd, bn_finalize_stats, affine_act);
#   "bf16x6"  OPT-IN: 3 bf16 planes (8 + 8 + 8 mantissa bits: exact, full fp32 range), 6 plane products:
#             fp32-equivalent at any dynamic range (4e-7..9e-7 vs fp64), the default of rounds 2-3;
#   "fp32"    OPT-IN: exact fp32-input MFMA (v_mfma_f32_32x32x2_f32), bit-for-bit a k-ordered fmaf chain;
#   "bf16x3"  OPT-IN: 2 bf16 planes (hi/lo), 3 MFMAs per multiply, ~4.5e-6 relative error per convolution.
# The 3-channel edge layers (conv_thin_*.hip) run bf16x6 under fp16x3 too: they are bound by HBM and issue slots.
# Set here, or with VG_CONV_ARITH in the environment.  DESIGN.md section 2.
CONV_ARITH = os.environ.get("VG_CONV_ARITH", "fp16x3")
WGRAD_SPLIT = True      # within the split modes: False keeps the weight gradient on the exact-fp32 kernel
if CONV_ARITH not in ("fp32", "bf16x3", "bf16x6", "fp16x3"):
    raise ImportError(f"VG_CONV_ARITH={CONV_ARITH!r}: expected 'fp16x3', 'bf16x6', 'bf16x3' or 'fp32'")


THIN_SPLIT = os.environ.get("VG_THIN_SPLIT", "1") != "0"   # 0: the 3-channel edge layers stay on the fp32 VALU / fp32-MFMA kernels in every arithmetic
PLANES_F16 = 0x100      # VG_PLANES_F16 of include/vaegan_hip.h


def _planes():
    """`planes` argument of the split kernels for the active arithmetic: 0 (exact fp32 MFMA), 2 (bf16x3), 3 (bf16x6) or
    2 | VG_PLANES_F16 (fp16x3)."""
    return {"fp32": 0, "bf16x3": 2, "bf16x6": 3, "fp16x3": 2 | PLANES_F16}[CONV_ARITH]


def _f16():
    return CONV_ARITH == "fp16x3"


def _thin_planes():
    """The 3-channel edge kernels take bf16 planes only: bf16x6 under fp16x3."""
    return 3 if _f16() else _planes()


# ---- bounds of max |tensor| for the fp16 planes (csrc/absmax.hip) ---------------------------------------------------
# A bound is a one-element fp32 device tensor.  Slots come zeroed from an arena (one fill launch per 512 of them); the
# producing kernel adds its maximum with an atomic.  A tensor object remembers its bound (an `_Amax` record, written by
# `set_amax` and read by `known_amax` alone), so that a gradient used by the data gradient AND the weight gradient, or
# an input used forward and again by the weight gradient, is measured once.  Nothing here or in the weights' records
# (`_WeightRecord`) is matched by an address or by an id alone: a Function whose output needs a bound outside returns it.
_AMAX_CHUNK = 512
_amax_arenas = {}        # (device index, capturing) -> [chunk, next free]


def new_amax_slot(device):
    """A zeroed bound slot: one launch, or several (the branches of an Inception block), add their maxima into it."""
    key = (device.index, torch.cuda.is_current_stream_capturing())
    a = _amax_arenas.get(key)
    if a is None or a[1] >= _AMAX_CHUNK:
        a = _amax_arenas[key] = [torch.zeros(_AMAX_CHUNK, dtype=torch.float32, device=device), 0]
    a[1] += 1
    return a[0][a[1] - 1:a[1]]


class amax_capture_scope:
    """Around a HIP-graph capture: the slots handed out inside come from chunks allocated -- and zero-filled -- INSIDE
    the capture (a replay zeroes them again before its kernels add their maxima), and no slot of those chunks is handed
    out once the capture has ended (a replay would zero it under an eager consumer)."""

    def __enter__(self):
        for k in [k for k in _amax_arenas if k[1]]:
            del _amax_arenas[k]
        return self

    def __exit__(self, *exc):
        for k in [k for k in _amax_arenas if k[1]]:
            del _amax_arenas[k]
        return False


class _Amax(NamedTuple):
    version: int            # the tensor's version counter when the bound was taken
    through: object         # the scale tensor of the affine the tensor was read through (compared with `is`), or None
    slot: torch.Tensor


def set_amax(t, slot, in_affine=None):
    """Remember ``slot`` as the bound of ``t`` (as read through ``in_affine``); returns ``slot``."""
    t._vg_amax = _Amax(t._version, None if in_affine is None else in_affine[0], slot)
    return slot


def known_amax(t, in_affine=None):
    """The bound slot remembered for ``t`` as it is now, read through ``in_affine`` (None: as it is) -- or None."""
    known = getattr(t, "_vg_amax", None)
    through = None if in_affine is None else in_affine[0]
    if known is not None and known.version == t._version and known.through is through:
        return known.slot
    return None


def keep_amax(src, view):
    """``view`` is a reshape of ``src`` (same elements): it inherits the bound a producer attached to ``src``."""
    slot = known_amax(src)
    if slot is not None:
        set_amax(view, slot)
    return view


def amax_of(t, in_affine=None):
    """Bound of max |t| -- of max |act(t * scale[c] + shift[c])| with ``in_affine`` = (scale, shift, act[, bound]) -- as a
    one-element device tensor: the one a producer attached, the 4th element of ``in_affine``, or one pass over t."""
    if in_affine is not None and len(in_affine) > 3 and in_affine[3] is not None:
        return in_affine[3]
    slot = known_amax(t, in_affine)
    if slot is not None:
        return slot
    lib = _lib.load()
    slot = new_amax_slot(t.device)
    if in_affine is None:
        check(lib.vg_absmax(t.data_ptr(), t.numel(), slot.data_ptr(), _stream()), "vg_absmax")
    else:
        B, C = t.shape[0], t.shape[1]
        check(lib.vg_absmax_affine(t.data_ptr(), in_affine[0].data_ptr(), in_affine[1].data_ptr(), int(in_affine[2]), B, C,
                                   t.numel() // (B * C), slot.data_ptr(), _stream()), "vg_absmax_affine")
    return set_amax(t, slot, in_affine)


# ---- which kernel family takes a convolution launch ------------------------------------------------------------------
# Every kernel is correct for every shape it accepts, so a slip here costs speed and no numeric test notices:
# tests/test_host_logic_cpu.py pins the routes of the benchmarked layers.  The switches and the channel thresholds are
# written here and nowhere else; what depends on the full shape is asked of the library (host-only queries).
SPLIT, THIN, FP32_PACKED, FP32_PACKED_STATS, FP32_PLAIN = "split", "thin", "fp32_packed", "fp32_packed_stats", "fp32_plain"


class ConvRoute(NamedTuple):
    """SPLIT: conv_ring.hip / conv_bf16split.hip / wgrad_bf16split.hip; THIN: conv_thin_*.hip; FP32_PACKED[_STATS]:
    conv_igemm.hip; FP32_PLAIN: the direct kernels on the plain filter layout, the exact-fp32 weight gradient."""
    family: str
    affine_on_load: bool    # the kernel applies the operand's affine while it loads; False with an affine: materialise it first
    stats_floats: int       # statistics slots the launch fills, in floats (0: it leaves none)
    workspace_bytes: int


def _thin_transposed(op, cout, stride):
    """A stride-1 transposed convolution with <= 4 output channels (the decoder's last layer, the data gradient of the
    discriminator's first) reads the plain filter layout: the direct VALU kernel, or conv_thin_mfma.hip."""
    return op == "convT_fwd" and stride == 1 and cout is not None and cout <= 4


def _split_asked(op, cin, cout, stride):
    """Whether the launch goes to the split kernels of the active arithmetic (the weight gradient: if they take the shape)."""
    planes = _planes()
    if not planes:
        return False
    if op == "conv_wgrad":
        # thin inputs stay on the exact-fp32 kernel: the re-layout of gy costs more than the split arithmetic saves
        # (measured: 2 planes pay off from 16 input channels, 3 planes from 32)
        return WGRAD_SPLIT and cin >= (16 if (planes & 0xff) == 2 else 32)
    return cin % 16 == 0 and not _thin_transposed(op, cout, stride)


def _thin_asked(op, cin, cout, stride):
    """Whether the launch is offered to the 3-channel edge kernels (they say which shapes they take)."""
    if not (_planes() and THIN_SPLIT):
        return False
    return _thin_transposed(op, cout, stride) if op == "convT_fwd" else cin <= 3


def conv_runs_split(op, cin, cout=None, stride=None):
    """Whether a convolution launch of kind ``op`` ("conv_fwd" | "convT_fwd" | "conv_wgrad") with
    ``cin`` input channels runs on the split-bf16 kernels under the active arithmetic (bench.py:
    which roofline a launch is priced against).  `route_conv` without the spatial shape: the edge kernels' limits
    on the image size are not asked (the 32 -> 3 transposed one is asked at a 16 x 16 image)."""
    if _split_asked(op, cin, cout, stride):
        return True
    if not _thin_asked(op, cin, cout, stride):
        return False
    return op != "convT_fwd" or bool(_lib.load().vg_convT5x5_s1_thin_bf16split_ok(cin, 16, 16, cout))


def conv_fusable(transposed, cin, cout, stride):
    """Whether the kernel of this layer (under the active arithmetic) applies a producer's BatchNorm + activation
    while it loads its input and can leave output statistics (include/vaegan_hip.h, vg_conv_fusion)."""
    return bool(_planes()) and bool(_lib.load().vg_conv5x5_bf16split_fusable(1 if transposed else 0, cin, cout, stride))


def route_conv(op, B, Cin, H, W, Cout, stride, affine=None, want_stats=False):
    """The one decision "which kernel runs this convolution launch": ``op`` "conv_fwd" | "convT_fwd" | "conv_wgrad" on
    the full shape (of x and, for the weight gradient, gy's channels), ``affine`` None | "x" | "gy": the operand read as
    act(v * scale[c] + shift[c]), ``want_stats``: the caller wants the output's statistics slots (their size is asked
    only then).  Host only: no tensor, no launch; reads the arithmetic and the switches as they are now."""
    lib = _lib.load()
    shape = (B, Cin, H, W, Cout, stride)
    split, thin = _split_asked(op, Cin, Cout, stride), _thin_asked(op, Cin, Cout, stride)
    if op == "conv_wgrad":
        need = lib.vg_conv5x5_wgrad_bf16split_workspace_bytes(*shape, _planes()) if split else 0     # 0: shape not taken
        if need:
            return ConvRoute(SPLIT, affine is not None, 0, need)
        # <= 3 input channels: one read pass over gy (a producer's BatchNorm + activation applied to it on load: the weight
        # gradient of the decoder's last layer), x split once per workgroup into shifted plane copies in LDS
        need = lib.vg_conv5x5_thin_wgrad_bf16split_workspace_bytes(*shape, _thin_planes()) if thin else 0   # 0: shape not taken
        if need:
            return ConvRoute(THIN, affine == "gy", 0, need)
        return ConvRoute(FP32_PLAIN, False, 0, lib.vg_conv5x5_wgrad_workspace_bytes(*shape))
    tr = op == "convT_fwd"
    if split:
        fus = conv_fusable(tr, Cin, Cout, stride)
        q = "vg_convT5x5_fwd_bf16split" if tr else "vg_conv5x5_fwd_bf16split"
        n = getattr(lib, q + "_stats_floats")(*shape, _planes()) if (want_stats and fus) else 0
        # workspace: split-K slabs (forward: deep-K layers only, transposed: small grids only)
        return ConvRoute(SPLIT, fus and affine is not None, n, getattr(lib, q + "_workspace_bytes")(*shape, _planes()))
    if thin and tr and lib.vg_convT5x5_s1_thin_bf16split_ok(Cin, H, W, Cout):
        # 32 -> (<= 3) channels: filter resident in registers, one pass over x (BatchNorm + activation applied on load)
        return ConvRoute(THIN, affine is not None, 0, 0)
    if thin and not tr and lib.vg_conv5x5_thin_bf16split_ok(Cin, H, W, Cout, stride):
        # <= 3 input channels: filter resident in registers, one write pass over y, statistics on the way out
        return ConvRoute(THIN, False, lib.vg_conv5x5_thin_bf16split_stats_floats(*shape) if want_stats else 0, 0)
    if USE_PACKED_FILTERS and not _thin_transposed(op, Cout, stride):
        # The exact-fp32 kernel can leave the next BatchNorm's statistics too (vg_conv5x5_fwd_packed_stats), but on the
        # 3-channel first layers -- 16 384 slots for 32 channels at B = 128 -- writing and reducing the slots costs more
        # than the one pass over the output it saves (measured: +0.26 ms per iteration): opt-in only.
        n = lib.vg_conv5x5_fwd_packed_stats_floats(*shape) if (want_stats and FP32_CONV_STATS and not tr) else 0
        return ConvRoute(FP32_PACKED_STATS if n else FP32_PACKED, False, n, 0)
    return ConvRoute(FP32_PLAIN, False, 0, 0)


def _launch(key, symbol, *args):
    """One convolution launch on the current stream, timed under ``key`` while `start_timing` is active."""
    with _timed(key):
        check(getattr(_lib.load(), symbol)(*args, _stream()), symbol)


# ---- packed filters --------------------------------------------------------------------------------------------------
_pack_scope_depth = 0
_records = {}         # id(w) -> _WeightRecord of a live weight: its weak reference takes it out before the id can be re-used
_pack_scratch = {}    # (device, stream, numel) -> tensor, for un-cached packs
PACK_FP32, PACK_SPLIT = "fp32", "split"      # layouts: vg_conv5x5_pack (conv_igemm.hip) / vg_conv5x5_pack_bf16split


class _Bound(NamedTuple):
    version: int            # the weight's version counter when the bound was taken
    slot: torch.Tensor
    emitted: bool           # by the optimizer step that wrote the weight; False: measured inside a packed_filter_scope


class _WeightRecord:
    """What is derived from ONE weight tensor object and lives as long as it: ``bound``, the `_Bound` of a Linear weight
    (or None), and ``packs``, (layout, transposed, stride, planes) -> [valid, version, packed tensor] of a convolution
    filter.  A pack's tensor is allocated when its key is first asked for and never replaced."""
    __slots__ = ("ref", "bound", "packs")

    def __init__(self, ref):
        self.ref, self.bound, self.packs = ref, None, {}


def _record(w, create=False):
    """The record of THIS tensor object, or None: never that of another tensor at its address or with its id."""
    rec = _records.get(id(w))
    if (rec is None or rec.ref() is not w) and create:
        rec = _records[id(w)] = _WeightRecord(weakref.ref(w, lambda _ref, key=id(w): _records.pop(key, None)))
    return rec if rec is not None and rec.ref() is w else None


class packed_filter_scope:
    """Within the scope packed filters are cached per weight tensor object; the owner of the scope promises to call
    `invalidate_packed_filters()` after every in-place weight update.  Outside one every pack is stale (`__exit__`)."""

    def __enter__(self):
        global _pack_scope_depth
        _pack_scope_depth += 1
        return self

    def __exit__(self, *exc):
        global _pack_scope_depth
        _pack_scope_depth -= 1
        if _pack_scope_depth == 0:
            invalidate_packed_filters()
        return False


def buffers_in_use():
    """Every pack buffer of a live weight, every workspace and scratch buffer that exists now, as a list of tensors.  A
    HIP graph captured over launches that read or write them holds raw device pointers: its owner keeps this list for as
    long as the graph may be replayed, so that the memory outlives a weight dropped or a workspace regrown meanwhile."""
    packs = [ent[2] for rec in list(_records.values()) for ent in rec.packs.values()]
    return packs + list(_workspaces.values()) + list(_pack_scratch.values())


def invalidate_packed_filters(params=None):
    """Mark the packs stale and drop the measured bounds -- of every live weight, or of the given tensor objects.  The
    fused Adam step writes weights without moving their version counter: that is why measured entries need this call.
    A bound the step emitted itself (`set_weight_bound`) is as new as the weights and is never dropped here."""
    for rec in list(_records.values()) if params is None else filter(None, map(_record, params)):
        for ent in rec.packs.values():
            ent[0] = False
        if rec.bound is not None and not rec.bound.emitted:
            rec.bound = None


def _pack_floats(lib, cout, cin, layout):
    if layout == PACK_SPLIT:
        return lib.vg_conv5x5_packed_bf16split_bytes(cout, cin, _planes()) // 4
    return lib.vg_conv5x5_packed_floats(cout, cin)


def _pack_entry(lib, w, cout, cin, layout, transposed, stride):
    """(the entry [valid, version, packed tensor] of this weight object in this layout -- created, stale, when it is asked
    for the first time --, whether its pack is that of the weight as it is now)."""
    packs = _record(w, create=True).packs
    key = (layout, transposed, stride, _planes() if layout == PACK_SPLIT else 0)
    ent = packs.get(key)
    if ent is None:
        ent = packs[key] = [False, -1, torch.empty(_pack_floats(lib, cout, cin, layout), dtype=torch.float32, device=w.device)]
    return ent, ent[0] and ent[1] == w._version


def _packed_filter(lib, w, cout, cin, layout, transposed, stride):
    split_layout = layout == PACK_SPLIT
    if split_layout and _pack_log is not None:
        _pack_log.append(PackRequest(w, cout, cin, transposed, stride))
    if _pack_scope_depth > 0:
        ent, fresh = _pack_entry(lib, w, cout, cin, layout, transposed, stride)
        if fresh:
            return ent[2]
    else:
        skey = (w.device.index, _stream(), _pack_floats(lib, cout, cin, layout))
        if skey not in _pack_scratch:
            _pack_scratch[skey] = torch.empty(skey[2], dtype=torch.float32, device=w.device)
        ent = [False, -1, _pack_scratch[skey]]          # un-cached: an entry nobody reads again
    if split_layout:
        wmax = None
        if _f16():          # a fresh (zeroed) slot per pack: the bound follows the weights down as well as up
            wmax = new_amax_slot(w.device)
            check(lib.vg_absmax(w.data_ptr(), w.numel(), wmax.data_ptr(), _stream()), "vg_absmax")
        check(lib.vg_conv5x5_pack_bf16split(w.data_ptr(), ent[2].data_ptr(), cout, cin, int(transposed), stride, _planes(),
                                         _ptr(wmax), _stream()), "vg_conv5x5_pack_bf16split")
    else:
        check(lib.vg_conv5x5_pack(w.data_ptr(), ent[2].data_ptr(), cout, cin, int(transposed), stride, _stream()),
              "vg_conv5x5_pack")
    ent[0], ent[1] = True, w._version
    return ent[2]


PackRequest = NamedTuple("PackRequest", [("w", torch.Tensor), ("cout", int), ("cin", int), ("transposed", bool), ("stride", int)])
_pack_log = None      # while a list: every split-layout pack request appends its PackRequest (which keeps the weight alive)


class record_pack_requests:
    """Context: collects which (weight, layout) pairs the convolutions inside it asked for -- a trainer records its
    first iteration and afterwards re-packs all filters an optimizer step has changed in ONE launch
    (`prepack_filters`) instead of one launch per filter on first use."""

    def __enter__(self):
        global _pack_log
        self._prev, _pack_log = _pack_log, []
        self.requests = _pack_log
        return self

    def __exit__(self, *exc):
        global _pack_log
        _pack_log = self._prev
        return False


def prepack_filters(requests):
    """Pack (split layout) every listed filter whose pack is stale, all in one launch, each into the one buffer its weight
    object ever has.  ``requests``: `PackRequest`s as `record_pack_requests` collects them.  Only inside a
    `packed_filter_scope` (outside it nothing is cached)."""
    if _pack_scope_depth <= 0 or not requests or not _planes():
        return
    lib = _lib.load()
    entries = [(r, *_pack_entry(lib, r.w, r.cout, r.cin, PACK_SPLIT, r.transposed, r.stride)) for r in requests]
    todo = [(r, _record(r.w), ent) for r, ent, fresh in entries if not fresh]
    if not todo:
        return
    arr = (_lib.PackEntry * len(todo))()
    wmax = {}                            # weight record -> bound slot
    if _f16():                           # the filters' bounds first, all in one launch (one per weight, not per layout)
        for r, rec, _ent in todo:
            if rec not in wmax:
                wmax[rec] = new_amax_slot(r.w.device)
        am = (_lib.AbsmaxEntry * len(wmax))()
        for i, (rec, slot) in enumerate(wmax.items()):
            am[i] = _lib.AbsmaxEntry(rec.ref().data_ptr(), rec.ref().numel(), slot.data_ptr())
        check(lib.vg_absmax_multi(am, len(wmax), _stream()), "vg_absmax_multi")
    for i, (r, rec, ent) in enumerate(todo):
        slot = wmax[rec].data_ptr() if wmax else None
        arr[i] = _lib.PackEntry(r.w.data_ptr(), ent[2].data_ptr(), r.cout, r.cin, int(r.transposed), r.stride, slot)
    check(lib.vg_conv5x5_pack_bf16split_multi(arr, len(todo), _planes(), _stream()), "vg_conv5x5_pack_bf16split_multi")
    for r, _rec, ent in todo:
        ent[0], ent[1] = True, r.w._version


# ---- the three entry points: validate, route, allocate, launch --------------------------------------------------------
def _fusion_struct(x, in_affine, stats):
    """ctypes vg_conv_fusion (or None) + the tensors it points at (kept alive by the caller).  fp16 planes: always, with
    the bound of the input as the kernel reads it."""
    if in_affine is None and stats is None and not _f16():
        return None
    f = _lib.ConvFusion()
    if _f16():
        f._amax = amax_of(x, in_affine)          # kept alive with the struct
        f.in_amax = f._amax.data_ptr()
    if in_affine is not None:
        f.in_scale, f.in_shift, f.in_act = _affine_args(in_affine, x.shape[1])
    if stats is not None:
        f.stats, f.stats_floats = stats.data_ptr(), stats.numel()
    return f


def _affine_args(in_affine, channels=None):
    """(scale pointer, shift pointer, activation) of ``in_affine`` = (scale, shift, act[, bound]) for a kernel that applies it
    on load; (0, 0, 0) without one."""
    if in_affine is None:
        return 0, 0, ACT_NONE
    scale, shift, act = in_affine[:3]
    _req(scale, "in_scale"), _req(shift, "in_shift")
    if channels is not None and (scale.numel() != channels or shift.numel() != channels):
        raise RuntimeError("in_affine: one coefficient per input channel")
    return scale.data_ptr(), shift.data_ptr(), int(act)


def _materialize(x, in_affine):
    """act(x * scale[c] + shift[c]) as a tensor: the fallback for kernels that cannot apply it on load."""
    return x if in_affine is None else affine_act(x, *in_affine[:3])


def _conv_forward(op, x, w, bias, stride, in_affine, want_stats):
    lib = _lib.load()
    tr = op == "convT_fwd"
    name = "convT5x5_fwd" if tr else "conv5x5_fwd"
    _req(x, "x"), _req(w, "w")
    B, Cin, H, W = x.shape
    Cout = w.shape[1 if tr else 0]
    if w.shape != ((Cin, Cout, 5, 5) if tr else (Cout, Cin, 5, 5)):
        raise RuntimeError(f"{name}: weight {tuple(w.shape)} does not match input channels {Cin}")
    if bias is not None:
        _req(bias, "bias")
    shape = (B, Cin, H, W, Cout, stride)
    out_hw = (H * stride, W * stride) if tr else ((H - 1) // stride + 1, (W - 1) // stride + 1)
    y = torch.empty((B, Cout) + out_hw, dtype=torch.float32, device=x.device)
    r = route_conv(op, *shape, affine=None if in_affine is None else "x", want_stats=want_stats)
    if in_affine is not None and not r.affine_on_load:
        x, in_affine = _materialize(x, in_affine), None
    stats = torch.empty(r.stats_floats, dtype=torch.float32, device=x.device) if r.stats_floats else None
    io = (_ptr(bias), y.data_ptr()) + shape
    if r.family == SPLIT:
        f = _fusion_struct(x, in_affine, stats)
        pk = _packed_filter(lib, w, Cout, Cin, PACK_SPLIT, tr, stride)    # the stride-2 kernel has its own step order
        ws = workspace(r.workspace_bytes, x.device) if r.workspace_bytes else None
        sym, args = f"vg_{name}_bf16split", (x.data_ptr(), pk.data_ptr()) + io + (
            _planes(), _ptr(ws), ws.numel() if ws is not None else 0, ctypes.byref(f) if f is not None else None)
    elif r.family == THIN and tr:
        sym, args = "vg_convT5x5_s1_thin_bf16split", (x.data_ptr(), w.data_ptr()) + io[:-1] + (      # (stride 1 only)
            _thin_planes(),) + _affine_args(in_affine)
    elif r.family == THIN:
        sym, args = "vg_conv5x5_thin_bf16split", (x.data_ptr(), w.data_ptr()) + io + (_thin_planes(), _ptr(stats), r.stats_floats)
    elif r.family == FP32_PLAIN:
        sym, args = f"vg_{name}", (x.data_ptr(), w.data_ptr()) + io
    else:
        pk = _packed_filter(lib, w, Cout, Cin, PACK_FP32, tr, stride)
        sym, args = f"vg_{name}_packed", (x.data_ptr(), pk.data_ptr()) + io
        if r.family == FP32_PACKED_STATS:
            sym, args = sym + "_stats", args + (stats.data_ptr(), r.stats_floats)
    _launch((op,) + shape, sym, *args)
    return (y, stats) if want_stats else y


def conv5x5_fwd(x, w, bias, stride, in_affine=None, want_stats=False):
    """``in_affine`` = (scale, shift, act): the input is act(x * scale[c] + shift[c]) -- the producing layer's
    train-mode BatchNorm + activation -- applied on load where the kernel can, materialised first where it cannot.
    ``want_stats``: returns (y, stats) with per-channel partial sums of y for `bn_finalize_stats`, or (y, None)
    when this layer's kernel cannot emit them."""
    return _conv_forward("conv_fwd", x, w, bias, stride, in_affine, want_stats)


def convT5x5_fwd(x, w, bias, stride, in_affine=None, want_stats=False):
    """w is (Cin, Cout, 5, 5); output is (B, Cout, stride*H, stride*W).  ``in_affine`` / ``want_stats``: see
    `conv5x5_fwd`."""
    return _conv_forward("convT_fwd", x, w, bias, stride, in_affine, want_stats)


def conv5x5_wgrad(x, gy, stride, out=None, in_affine=None, affine_on_gy=False, accumulate=False):
    """dw[Cout,Cin,5,5] for y = conv(x, w, stride); x (B,Cin,H,W), gy (B,Cout,OH,OW).  ``in_affine`` = (scale, shift,
    act): the operand x -- or gy when ``affine_on_gy`` (the weight gradient of a transposed convolution passes the
    layer's input there) -- is read as act(v * scale[c] + shift[c]), on load where the kernel can.  ``accumulate``: the
    result is added to what ``out`` holds (inside the kernel's final slab sum)."""
    if accumulate and out is None:
        raise RuntimeError("conv5x5_wgrad: accumulate needs the tensor to accumulate into (out=)")
    acc = 1 if accumulate else 0
    _req(x, "x"), _req(gy, "gy")
    B, Cin, H, W = x.shape
    Cout = gy.shape[1]
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if gy.shape != (B, Cout, OH, OW):
        raise RuntimeError(f"conv5x5_wgrad: gy {tuple(gy.shape)} does not match x {tuple(x.shape)} stride {stride}")
    shape = (B, Cin, H, W, Cout, stride)
    dw = out if out is not None else torch.empty((Cout, Cin, 5, 5), dtype=torch.float32, device=x.device)
    r = route_conv("conv_wgrad", *shape, affine=None if in_affine is None else ("gy" if affine_on_gy else "x"))
    if in_affine is not None and not r.affine_on_load:      # this kernel takes the operand as a tensor
        if affine_on_gy:
            gy = _materialize(gy, in_affine)
        else:
            x = _materialize(x, in_affine)
        in_affine = None
    ws = workspace(r.workspace_bytes, x.device)
    args = (x.data_ptr(), gy.data_ptr(), dw.data_ptr()) + shape
    if r.family == SPLIT:
        xmax = gmax = None
        if _f16():       # bounds of the two operands as the kernel reads them
            xmax = amax_of(x, None if affine_on_gy else in_affine)
            gmax = amax_of(gy, in_affine if affine_on_gy else None)
        sym, args = "vg_conv5x5_wgrad_bf16split", args + (_planes(), ws.data_ptr(), ws.numel()) + _affine_args(in_affine) + (
            1 if affine_on_gy else 0, _ptr(xmax), _ptr(gmax), acc)
    elif r.family == THIN:
        sym, args = "vg_conv5x5_thin_wgrad_bf16split", args + (_thin_planes(), ws.data_ptr(), ws.numel()) + _affine_args(
            in_affine) + (acc,)
    else:
        sym, args = "vg_conv5x5_wgrad", args + (ws.data_ptr(), ws.numel(), acc)
    _launch(("conv_wgrad",) + shape, sym, *args)
    return dw


# ---------------------------------------------------- general forward convolution (csrc/conv_general.hip)
class ConvGeneralMeta(NamedTuple):
    """Shape of a filter packed by `conv_general_pack` and how it is applied."""
    cout: int
    cin: int
    kh: int
    kw: int
    sh: int
    sw: int
    ph: int
    pw: int


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def conv_general_pack(w, stride=1, padding=0):
    """Pack the fp32 filter ``w`` (Cout, Cin, KH, KW) once for `conv2d_bias_act` (scaled by its bound from one
    vg_absmax pass, split into fp16 planes); returns (packed, meta)."""
    _req(w, "w")
    if w.dim() != 4:
        raise RuntimeError(f"conv_general_pack: expected a (Cout, Cin, KH, KW) filter, got {tuple(w.shape)}")
    lib = _lib.load()
    meta = ConvGeneralMeta(*(int(s) for s in w.shape), *_pair(stride), *_pair(padding))
    nbytes = lib.vg_conv_general_packed_bytes(meta.cout, meta.cin, meta.kh, meta.kw)
    if not nbytes:
        raise RuntimeError(f"conv_general_pack: filter {tuple(w.shape)} is not taken")
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    check(lib.vg_conv_general_pack(w.data_ptr(), packed.data_ptr(), meta.cout, meta.cin, meta.kh, meta.kw,
                                   amax_of(w).data_ptr(), _stream()), "vg_conv_general_pack")
    return packed, meta


def conv2d_bias_act(x, packed, meta, bias=None, out=None, out_channel_offset=0, relu=True, amax=None):
    """act(conv2d(x, w, stride, padding) + bias) in the fp16x3 arithmetic, w packed by `conv_general_pack`.  ``out``: a
    (B, C, OH, OW) tensor whose images are contiguous (a whole NCHW tensor or a channel slice of one); channels
    [out_channel_offset, out_channel_offset + Cout) are written, the others are not touched.  ``amax``: the bound slot
    max |y| is added to (a new one by default); the returned view of the written channels carries it."""
    _req(x, "x")
    if bias is not None:
        _req(bias, "bias")
    if x.dim() != 4 or x.shape[1] != meta.cin:
        raise RuntimeError(f"conv2d_bias_act: input {tuple(x.shape)} does not match {meta.cin} input channels")
    B, _, H, W = x.shape
    OH, OW = (H + 2 * meta.ph - meta.kh) // meta.sh + 1, (W + 2 * meta.pw - meta.kw) // meta.sw + 1
    if out is None:
        out = torch.empty((B, meta.cout, OH, OW), dtype=torch.float32, device=x.device)
    else:
        if not out.is_cuda or out.dtype != torch.float32 or out.dim() != 4:
            raise RuntimeError("conv2d_bias_act: out must be a 4-D float32 CUDA/ROCm tensor")
        if (out.shape[0], out.shape[2], out.shape[3]) != (B, OH, OW) or out.stride()[1:] != (OH * OW, OW, 1) or \
                not 0 <= out_channel_offset <= out.shape[1] - meta.cout or (B > 1 and out.stride(0) < out.shape[1] * OH * OW):
            raise RuntimeError(f"conv2d_bias_act: out {tuple(out.shape)} (strides {out.stride()}) cannot take channels "
                               f"[{out_channel_offset}, {out_channel_offset + meta.cout}) of a (B={B}, {OH}x{OW}) output")
    view = out[:, out_channel_offset:out_channel_offset + meta.cout]
    slot = amax if amax is not None else new_amax_slot(x.device)
    _launch(("conv_general", B, H, W) + tuple(meta), "vg_conv_general_fwd", x.data_ptr(), packed.data_ptr(), _ptr(bias),
            view.data_ptr(), B, meta.cin, H, W, meta.cout, meta.kh, meta.kw, meta.sh, meta.sw, meta.ph, meta.pw,
            max(out.stride(0), meta.cout * OH * OW), 1 if relu else 0, amax_of(x).data_ptr(), slot.data_ptr())
    set_amax(view, slot)
    return view


# ------------------------------------------------------------------- Linear layers
# The Linear GEMMs of the big layers (16384 <-> 2048 / 512, 128 -> 16384: model.py:460-471, 402-408, 490-492) on this
# package's fp16x3 GEMM (csrc/gemm_split.hip) under the default arithmetic; under the opt-in arithmetics, for small
# layers and for reductions that are not a multiple of 32 (the weight gradient at such batches) they stay on the vendor
# fp32 GEMM.  VG_LINEAR_SPLIT=0 (or ops.LINEAR_SPLIT = False): vendor GEMMs everywhere.
LINEAR_SPLIT = os.environ.get("VG_LINEAR_SPLIT", "1") != "0"
LINEAR_SPLIT_MIN_WEIGHTS = 1 << 20


def linear_split_ok(reduction, nweights):
    return LINEAR_SPLIT and _f16() and reduction % 32 == 0 and nweights >= LINEAR_SPLIT_MIN_WEIGHTS


def _weight_bound_entry(w):
    """The `_Bound` recorded for THIS tensor object as it is now (same object, same version counter), or None."""
    rec = _record(w)
    return rec.bound if rec is not None and rec.bound is not None and rec.bound.version == w._version else None


def set_weight_bound(w, bound):
    """``bound`` (one-element device tensor) holds max |w| as of now -- HipAdam's step emits it (VgAdamTensor.amax).
    Valid for THIS tensor object until the next torch-side in-place write (the version counter) or the next call for
    this weight."""
    _record(w, create=True).bound = _Bound(w._version, bound, True)


def weight_bound(w):
    """Bound of max |w| of a Linear weight: the one the optimizer step emitted when it wrote the weight; failing that,
    inside a `packed_filter_scope`, measured once per weight version (the scope's owner invalidates after optimizer
    steps, as for the packed filters), otherwise per call."""
    ent = _weight_bound_entry(w)
    if ent is not None and (ent.emitted or _pack_scope_depth > 0):
        return ent.slot
    slot = new_amax_slot(w.device)       # a fresh (zeroed) slot: the bound follows the weights down as well as up
    check(_lib.load().vg_absmax(w.data_ptr(), w.numel(), slot.data_ptr(), _stream()), "vg_absmax")
    if _pack_scope_depth > 0:
        _record(w, create=True).bound = _Bound(w._version, slot, False)
    return slot


def _gemm_nt(A, B, bias, C, M, N, K, ars, aks, brs, bks, a_amax, b_amax):
    lib = _lib.load()
    need = lib.vg_gemm_nt_f16x3_workspace_bytes(M, N, K)
    ws = workspace(need, A.device) if need else None
    check(lib.vg_gemm_nt_f16x3(A.data_ptr(), B.data_ptr(), _ptr(bias), C.data_ptr(), M, N, K, ars, aks, brs, bks,
                               a_amax.data_ptr(), b_amax.data_ptr(), _ptr(ws), ws.numel() if need else 0, _stream()),
          "vg_gemm_nt_f16x3")
    return C


def linear_fwd(x, w, bias):
    """y = x W^T + bias (nn.Linear forward, model.py:460-471): x (M, K), w (N, K)."""
    _req(x, "x"), _req(w, "w")
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    return _gemm_nt(x, w, bias, y, M, N, K, K, 1, K, 1, amax_of(x), weight_bound(w))


def linear_dgrad(gy, w):
    """gx = gy W: gy (M, N), w (N, K) -> (M, K); the reduction runs over N, W is read with its row index contiguous."""
    _req(gy, "gy"), _req(w, "w")
    M, N = gy.shape
    K = w.shape[1]
    gx = torch.empty((M, K), dtype=torch.float32, device=gy.device)
    return _gemm_nt(gy, w, None, gx, M, K, N, N, 1, 1, K, amax_of(gy), weight_bound(w))


GEMM_MAX_GROUPS = 3      # VG_GEMM_MAX_GROUPS of include/vaegan_hip.h


def _gemm_nt_grouped(As, B, bias, Cs, M, N, K, ars, aks, brs, bks, a_amaxes, b_amax):
    """vg_gemm_nt_f16x3_grouped: every Cs[g] = As[g] B^T (+ bias), bit for bit `_gemm_nt` on As[g], with B read once."""
    lib = _lib.load()
    G = len(As)
    if not 1 <= G <= GEMM_MAX_GROUPS:
        raise RuntimeError(f"grouped Linear GEMM: 1..{GEMM_MAX_GROUPS} groups, got {G}")
    need = lib.vg_gemm_nt_f16x3_grouped_workspace_bytes(G, M, N, K)
    ws = workspace(need, B.device) if need else None
    ptrs = ctypes.c_void_p * G
    check(lib.vg_gemm_nt_f16x3_grouped(G, ptrs(*(a.data_ptr() for a in As)), B.data_ptr(), _ptr(bias),
                                       ptrs(*(c.data_ptr() for c in Cs)), M, N, K, ars, aks, brs, bks,
                                       ptrs(*(a.data_ptr() for a in a_amaxes)), b_amax.data_ptr(), _ptr(ws),
                                       ws.numel() if need else 0, _stream()), "vg_gemm_nt_f16x3_grouped")
    return Cs


def _req_group(ts, name):
    for t in ts:
        _req(t, name)
        if t.shape != ts[0].shape:
            raise RuntimeError(f"grouped Linear GEMM: every {name} of a group call has the same shape")


def linear_fwd_grouped(xs, w, bias):
    """`linear_fwd` for 1..3 inputs of one shape against the same weight, the weight streamed and split once: the passes
    of the discriminator over unchanged weights.  Returns the list of outputs, each bit for bit `linear_fwd(x, w, bias)`."""
    _req_group(xs, "x"), _req(w, "w")
    M, K = xs[0].shape
    N = w.shape[0]
    ys = [torch.empty((M, N), dtype=torch.float32, device=w.device) for _ in xs]
    return _gemm_nt_grouped(xs, w, bias, ys, M, N, K, K, 1, K, 1, [amax_of(x) for x in xs], weight_bound(w))


def linear_dgrad_grouped(gys, w):
    """`linear_dgrad` for 1..3 output gradients of one shape against the same weight (read once)."""
    _req_group(gys, "gy"), _req(w, "w")
    M, N = gys[0].shape
    K = w.shape[1]
    gxs = [torch.empty((M, K), dtype=torch.float32, device=w.device) for _ in gys]
    return _gemm_nt_grouped(gys, w, None, gxs, M, K, N, N, 1, 1, K, [amax_of(g) for g in gys], weight_bound(w))


def linear_wgrad(gy, x):
    """gW = gy^T x: gy (M, N), x (M, K) -> (N, K); the reduction runs over the batch M (both operands strided)."""
    _req(gy, "gy"), _req(x, "x")
    M, N = gy.shape
    K = x.shape[1]
    gw = torch.empty((N, K), dtype=torch.float32, device=gy.device)
    return _gemm_nt(gy, x, None, gw, N, K, M, 1, N, 1, K, amax_of(gy), amax_of(x))


def linear_wgrad_adam(gy, x, reg):
    """`linear_wgrad` and the plain Adam step of the weight in ONE launch (``vg_linear_wgrad_adam`` / ``_dev``): the
    gradient gy^T x is consumed in registers and never written.  ``reg``: the weight's registration for this step
    (optim.FusedLinearStep: p, m, v, its bound word -- zeroed by the entry, in stream order behind the layer's data
    gradient -- its flag word, the step's scalars).  p, m, v, the bound and the flag bits are what `linear_wgrad` followed
    by the optimizer's own launch leave.  Returns False -- nothing was launched -- when the entry point refuses the
    shape (a reduction that is split over workgroups): the caller takes the two launches."""
    _req(gy, "gy"), _req(x, "x")
    lib = _lib.load()
    M, N = gy.shape
    K = x.shape[1]
    if tuple(reg.p.shape) != (N, K):
        raise RuntimeError(f"linear_wgrad_adam: weight {tuple(reg.p.shape)} against a ({N}, {K}) gradient")
    head = (gy.data_ptr(), x.data_ptr(), M, N, K, amax_of(gy).data_ptr(), amax_of(x).data_ptr(), reg.p.data_ptr(),
            reg.m.data_ptr(), reg.v.data_ptr(), reg.amax.data_ptr(), _ptr(reg.flag))
    if reg.scalars is not None:
        rc = lib.vg_linear_wgrad_adam_dev(*head, reg.beta1, reg.beta2, reg.eps, reg.scalars.data_ptr(), None, _stream())
    else:
        rc = lib.vg_linear_wgrad_adam(*head, reg.lr, reg.beta1, reg.beta2, reg.eps, reg.bc1, reg.bc2_sqrt, None,
                                      _stream())
    if rc == -1:                                         # VG_ERR_BAD_ARG: refused before any launch
        return False
    check(rc, "vg_linear_wgrad_adam")
    return True


def channel_sum(g):
    lib = _lib.load()
    _req(g, "g")
    B, C = g.shape[0], g.shape[1]
    HW = g.numel() // (B * C)
    out = torch.empty(C, dtype=torch.float32, device=g.device)
    ws = workspace(lib.vg_bn_workspace_bytes(C), g.device)
    check(lib.vg_channel_sum(g.data_ptr(), out.data_ptr(), B, C, HW, ws.data_ptr(), ws.numel(), _stream()),
          "vg_channel_sum")
    return out


# ------------------------------------------------------------------- BatchNorm
def bn_act_fwd(x, gamma, beta, running_mean, running_var, eps, momentum, act):
    lib = _lib.load()
    _req(x, "x"), _req(gamma, "gamma"), _req(beta, "beta")
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = workspace(lib.vg_bn_workspace_bytes(C), x.device)
    slot = new_amax_slot(x.device) if (_f16() and HW > 1) else None      # max |y| on the way out (as affine_act)
    check(lib.vg_bn_act_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _ptr(running_mean),
                            _ptr(running_var), mean.data_ptr(), invstd.data_ptr(), B, C, HW, eps, momentum, act, _ptr(slot),
                            ws.data_ptr(), ws.numel(), _stream()), "vg_bn_act_fwd")
    if slot is not None:
        set_amax(y, slot)
    return y, mean, invstd


def bn_finalize_stats(stats, count, gamma, beta, running_mean, running_var, eps, momentum, want_bound=False):
    """Coefficients of a train-mode BatchNorm from a convolution's statistics slots (``stats`` from
    conv5x5_fwd / convT5x5_fwd with want_stats): (mean, invstd, scale, shift); running statistics updated in place.
    ``want_bound``: a 5th result, the bound of max |act(BN(x))| an fp16-plane consumer needs (None in other arithmetics) --
    from the coefficients alone, no pass over x."""
    lib = _lib.load()
    _req(stats, "stats"), _req(gamma, "gamma"), _req(beta, "beta")
    C = gamma.numel()
    nslots = stats.numel() // (2 * C)
    out = torch.empty((4, C), dtype=torch.float32, device=gamma.device)
    mean, invstd, scale, shift = out[0], out[1], out[2], out[3]
    bound = new_amax_slot(gamma.device) if (want_bound and _f16()) else None
    ws = workspace(lib.vg_bn_workspace_bytes(C), gamma.device)
    check(lib.vg_bn_finalize_stats(stats.data_ptr(), nslots, C, float(count), gamma.data_ptr(), beta.data_ptr(),
                                   _ptr(running_mean), _ptr(running_var), mean.data_ptr(), invstd.data_ptr(),
                                   scale.data_ptr(), shift.data_ptr(), eps, momentum, _ptr(bound), ws.data_ptr(), ws.numel(),
                                   _stream()), "vg_bn_finalize_stats")
    return (mean, invstd, scale, shift, bound) if want_bound else (mean, invstd, scale, shift)


def bn_stats(x, gamma, beta, running_mean, running_var, eps, momentum, want_bound=False):
    """The same coefficients from a pass over x (layers whose producer leaves no statistics)."""
    lib = _lib.load()
    _req(x, "x"), _req(gamma, "gamma"), _req(beta, "beta")
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    out = torch.empty((4, C), dtype=torch.float32, device=x.device)
    mean, invstd, scale, shift = out[0], out[1], out[2], out[3]
    bound = new_amax_slot(x.device) if (want_bound and _f16()) else None
    ws = workspace(lib.vg_bn_workspace_bytes(C), x.device)
    check(lib.vg_bn_stats(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(running_mean), _ptr(running_var),
                          mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), B, C, HW, eps, momentum,
                          _ptr(bound), ws.data_ptr(), ws.numel(), _stream()), "vg_bn_stats")
    return (mean, invstd, scale, shift, bound) if want_bound else (mean, invstd, scale, shift)


def affine_act(x, scale, shift, act):
    """act(x * scale[c] + shift[c]) (the normalise pass of a BatchNorm whose coefficients are known)."""
    lib = _lib.load()
    _req(x, "x"), _req(scale, "scale"), _req(shift, "shift")
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = torch.empty_like(x)
    slot = new_amax_slot(x.device) if _f16() else None          # max |y| on the way out: y feeds a convolution
    check(lib.vg_affine_act(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), B, C, HW, int(act), _ptr(slot),
                            _stream()), "vg_affine_act")
    if slot is not None:
        set_amax(y, slot)
    return y


def bn_act_bwd(gy, x, gamma, beta, mean, invstd, act, need_param_grads=True, accumulate_into=None):
    """``accumulate_into`` = (dgamma, dbeta) tensors the parameter gradients are ADDED to (the layer's second use before
    one backward); they are then returned as they are."""
    lib = _lib.load()
    _req(gy, "gy"), _req(x, "x")
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    gx = torch.empty_like(x)
    if accumulate_into is not None:
        dgamma, dbeta = accumulate_into
    else:
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device) if need_param_grads else None
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device) if need_param_grads else None
    ws = workspace(lib.vg_bn_workspace_bytes(C), x.device)
    slot = new_amax_slot(x.device) if (_f16() and HW > 1) else None   # max |gx| on the way out: gx feeds a data / weight gradient
    check(lib.vg_bn_act_bwd(gy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                            invstd.data_ptr(), gx.data_ptr(), _ptr(dgamma), _ptr(dbeta), B, C, HW, act,
                            1 if accumulate_into is not None else 0, _ptr(slot), ws.data_ptr(), ws.numel(), _stream()),
          "vg_bn_act_bwd")
    if slot is not None:
        set_amax(gx, slot)
    return gx, dgamma, dbeta


# ---------------------------------------------------- BatchNorm on running statistics (eval mode)
def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps, act, stats=None, count=None, want_bound=False):
    """Coefficients of an eval-mode BatchNorm: (scale, shift, invstd) with scale = gamma / sqrt(running_var + eps),
    shift = beta - running_mean * scale; the running buffers are only read.  ``want_bound``: a 4th result, an upper bound
    of max |act(x * scale + shift)| for the x whose statistics slots ``stats`` (with ``count`` values per channel) the
    producing convolution left -- from the sums alone, no pass over x; None in other arithmetics and without slots
    (`amax_of` then measures the tensor through the affine)."""
    lib = _lib.load()
    _req(gamma, "gamma"), _req(beta, "beta"), _req(running_mean, "running_mean"), _req(running_var, "running_var")
    C = gamma.numel()
    if beta.numel() != C or running_mean.numel() != C or running_var.numel() != C:
        raise RuntimeError("bn_eval_coeffs: one gamma, beta, running mean and running variance per channel")
    have = stats is not None and stats.numel() > 0
    nslots = 0
    if have:
        _req(stats, "stats")
        if count is None or count <= 0 or stats.numel() % (2 * C):
            raise RuntimeError("bn_eval_coeffs: stats holds [nslots][C][2] floats and comes with the count per channel")
        nslots = stats.numel() // (2 * C)
    out = torch.empty((3, C), dtype=torch.float32, device=gamma.device)
    scale, shift, invstd = out[0], out[1], out[2]
    bound = new_amax_slot(gamma.device) if (want_bound and have and _f16()) else None
    check(lib.vg_bn_eval_coeffs(gamma.data_ptr(), beta.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(),
                                scale.data_ptr(), shift.data_ptr(), invstd.data_ptr(), C, eps, int(act),
                                stats.data_ptr() if bound is not None else 0, nslots if bound is not None else 0,
                                float(count) if bound is not None else 0.0, _ptr(bound), _stream()), "vg_bn_eval_coeffs")
    return (scale, shift, invstd, bound) if want_bound else (scale, shift, invstd)


def bn_eval_act_bwd(gy, x, scale, shift, mean, invstd, act, need_param_grads=True, accumulate_into=None):
    """Backward of y = act(x * scale[c] + shift[c]) with frozen coefficients (``mean``: the running mean they were made
    of): (gx, dgamma, dbeta).  ``need_param_grads`` / ``accumulate_into``: as `bn_act_bwd`."""
    lib = _lib.load()
    _req(gy, "gy"), _req(x, "x"), _req(scale, "scale"), _req(shift, "shift"), _req(mean, "mean"), _req(invstd, "invstd")
    if gy.shape != x.shape:
        raise RuntimeError(f"bn_eval_act_bwd: gy {tuple(gy.shape)} does not match x {tuple(x.shape)}")
    B, C = x.shape[0], x.shape[1]
    if any(t.numel() != C for t in (scale, shift, mean, invstd)):
        raise RuntimeError("bn_eval_act_bwd: one coefficient per channel")
    HW = x.numel() // (B * C)
    gx = torch.empty_like(x)
    if accumulate_into is not None:
        dgamma, dbeta = accumulate_into
    else:
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device) if need_param_grads else None
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device) if need_param_grads else None
    ws = workspace(lib.vg_bn_workspace_bytes(C), x.device)
    slot = new_amax_slot(x.device) if (_f16() and HW > 1) else None   # max |gx| on the way out (as bn_act_bwd)
    check(lib.vg_bn_eval_act_bwd(gy.data_ptr(), x.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                                 invstd.data_ptr(), gx.data_ptr(), _ptr(dgamma), _ptr(dbeta), B, C, HW, int(act),
                                 1 if accumulate_into is not None else 0, _ptr(slot), ws.data_ptr(), ws.numel(), _stream()),
          "vg_bn_eval_act_bwd")
    if slot is not None:
        set_amax(gx, slot)
    return gx, dgamma, dbeta


# ----------------------------------------------------------------- elementwise
def bias_act_fwd(x, bias, kind):
    lib = _lib.load()
    _req(x, "x")
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = torch.empty_like(x)
    check(lib.vg_bias_act_fwd(x.data_ptr(), _ptr(bias), y.data_ptr(), B, C, HW, kind, _stream()),
          "vg_bias_act_fwd")
    return y


def act_bwd(gy, y, kind):
    lib = _lib.load()
    _req(gy, "gy"), _req(y, "y")
    gx = torch.empty_like(y)
    slot = new_amax_slot(y.device) if (_f16() and LINEAR_SPLIT and y.dim() == 2) else None      # feeds a Linear layer's backward GEMMs
    check(lib.vg_act_bwd(gy.data_ptr(), y.data_ptr(), gx.data_ptr(), y.numel(), kind, _ptr(slot), _stream()), "vg_act_bwd")
    if slot is not None:
        set_amax(gx, slot)
    return gx


def scale_by_scalar(g, s):
    """g * s[0] with s a 0-dim device tensor (no host read)."""
    lib = _lib.load()
    _req(g, "g"), _req(s, "s")
    out = torch.empty_like(g)
    check(lib.vg_scale_by_scalar(g.data_ptr(), s.data_ptr(), out.data_ptr(), g.numel(), _stream()),
          "vg_scale_by_scalar")
    return out


# ---------------------------------------------------------------------- losses
def _beta_word(beta):
    """``beta`` given as a tensor: the one-element fp32 device word the ``_dev`` KL kernels read."""
    if beta.numel() != 1 or beta.dtype != torch.float32 or not beta.is_cuda:
        raise RuntimeError("reparam_kl: beta as a tensor must be one fp32 element on the GPU")
    return beta


def reparam_kl_fwd(mu, logvar, eps, beta, want_rows=False):
    """``beta``: a float, or a one-element fp32 device tensor read by the kernel (a value that changes between the replays
    of a captured iteration); the same fp32 value gives the same bits either way."""
    lib = _lib.load()
    _req(mu, "mu"), _req(logvar, "logvar"), _req(eps, "eps")
    B, D = mu.shape
    z = torch.empty_like(mu)
    kl = torch.empty((), dtype=torch.float32, device=mu.device)
    rows = torch.empty(B, dtype=torch.float32, device=mu.device) if want_rows else None
    if isinstance(beta, torch.Tensor):
        check(lib.vg_reparam_kl_fwd_dev(mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), z.data_ptr(), kl.data_ptr(),
                                        _ptr(rows), B, D, _beta_word(beta).data_ptr(), _stream()), "vg_reparam_kl_fwd_dev")
        return z, kl, rows
    check(lib.vg_reparam_kl_fwd(mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), z.data_ptr(), kl.data_ptr(),
                                _ptr(rows), B, D, float(beta), _stream()), "vg_reparam_kl_fwd")
    return z, kl, rows


def reparam_kl_bwd(gz, mu, logvar, eps, gkl, beta):
    """gz: tensor or None; gkl: 0-dim device tensor (upstream grad of the KL scalar) or None."""
    lib = _lib.load()
    B, D = mu.shape
    gmu, glv = torch.empty_like(mu), torch.empty_like(mu)
    if gz is not None:
        _req(gz, "gz")
    if gkl is not None:
        _req(gkl, "gkl")
    if isinstance(beta, torch.Tensor):
        check(lib.vg_reparam_kl_bwd_dev(_ptr(gz), mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), _ptr(gkl),
                                        _beta_word(beta).data_ptr(), gmu.data_ptr(), glv.data_ptr(), B, D, _stream()),
              "vg_reparam_kl_bwd_dev")
        return gmu, glv
    check(lib.vg_reparam_kl_bwd(_ptr(gz), mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), _ptr(gkl), float(beta),
                                gmu.data_ptr(), glv.data_ptr(), B, D, _stream()), "vg_reparam_kl_bwd")
    return gmu, glv


def _objective_launch(workspace_bytes, fn, fn_dev, mu, head, beta, tail, second=None):
    """The one call site of the KL-phase objectives' entry points (beta-TCVAE, DIP-VAE, InfoVAE / WAE-MMD, KL capacity;
    DESIGN.md section 4.24): ``fn(*head, beta, *tail, workspace, bytes, stream)`` -- or, ``beta`` given as a tensor,
    ``fn_dev`` with the word's address in that place.  ``workspace_bytes``, ``fn``, ``fn_dev``: the objective's three entries
    of the library; ``mu`` gives B, D and the device.  ``second``: ``(name, value)`` of an objective's OWN scheduled word,
    the argument right behind beta -- a float with a float beta, a one-element fp32 device tensor with beta's word (the
    ``_dev`` entry reads both); a mix is a TypeError.  An objective without one passes nothing and pays nothing."""
    B, D = mu.shape
    ws = workspace(workspace_bytes(B, D), mu.device)
    if isinstance(beta, torch.Tensor):
        fn, beta = fn_dev, _beta_word(beta).data_ptr()
    else:
        beta = float(beta)
    if second is not None:
        tail = (_second_word(*second, fn is fn_dev), *tail)
    check(fn(*head, beta, *tail, ws.data_ptr(), ws.numel(), _stream()), fn.__name__)


def _second_word(name, value, dev):
    """`_objective_launch`'s ``second`` as the C argument: the word's address (``dev``) or the float."""
    if isinstance(value, torch.Tensor) != dev:
        raise TypeError(f"beta and {name} must both be floats or both be one-element fp32 device tensors "
                        f"(beta is a {'tensor' if dev else 'float'}, {name} is not)")
    if not dev:
        return float(value)
    if value.numel() != 1 or value.dtype != torch.float32 or not value.is_cuda:
        raise RuntimeError(f"{name} as a tensor must be one fp32 element on the GPU")
    return value.data_ptr()


def reparam_tc_fwd(mu, logvar, eps, beta, alpha, gamma, log_bn):
    """Reparameterisation + the beta-TCVAE decomposition of the KL term (vg_reparam_tc_fwd).
    ``beta`` (the total-correlation weight): a float or the device word, as `reparam_kl_fwd`; ``alpha`` / ``gamma``: the
    weights of the mutual-information and dimension-wise-KL parts; ``log_bn``: log(B * dataset size).  Returns ``z``,
    ``out4`` = [loss, mi, tc, dwkl] and the two log-sum-exps the backward reads (``lse_joint`` [B] fp64, ``lse_dim`` [B, D])."""
    lib = _lib.load()
    _req(mu, "mu"), _req(logvar, "logvar"), _req(eps, "eps")
    if mu.dim() != 2 or logvar.shape != mu.shape or eps.shape != mu.shape:
        raise RuntimeError("reparam_tc: mu, logvar and eps must be [B, D] tensors of one shape")
    B, D = mu.shape
    z, lse_dim = torch.empty_like(mu), torch.empty_like(mu)
    out4 = torch.empty(4, dtype=torch.float32, device=mu.device)
    lse_joint = torch.empty(B, dtype=torch.float64, device=mu.device)
    head = (mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), z.data_ptr(), out4.data_ptr(), lse_joint.data_ptr(),
            lse_dim.data_ptr(), B, D, float(alpha))
    _objective_launch(lib.vg_reparam_tc_workspace_bytes, lib.vg_reparam_tc_fwd, lib.vg_reparam_tc_fwd_dev, mu, head, beta,
                      (float(gamma), float(log_bn)))
    return z, out4, lse_joint, lse_dim


AGG_POINT_TILE = 64      # VG_AGG_POINT_TILE: evaluation points per wavefront of vg_agg_posterior_lse
AGG_WORKGROUP_WAVES = 4  # wavefronts (point tiles) per workgroup of its two main kernels
AGG_ROW_TILE = 8         # VG_AGG_ROW_TILE: rows per row tile, the unit of its splits


def agg_posterior_splits(M, N, D, splits=None):
    """The number of row ranges `agg_posterior_lse` runs for these sizes: the launcher's choice for ``None``, else the
    request clamped to the number of row tiles (ceil(N / AGG_ROW_TILE)) with ranges left empty by the rounding dropped."""
    return int(_lib.load().vg_agg_posterior_splits(int(M), int(N), int(D), 0 if splits is None else int(splits)))


def agg_posterior_lse(z, mu, logvar, splits=None):
    """log sum_j N(z_m; mu_j, exp(logvar_j)), unnormalised (the caller subtracts log N), for M evaluation points under N
    diagonal Gaussians (vg_agg_posterior_lse): ``lse_joint`` [M] fp64 over whole vectors and
    ``lse_dim`` [M, D] fp32 per dimension.  ``z``: [M, D]; ``mu``, ``logvar``: [N, D].  ``splits``: the number of row
    ranges (tests), ``None`` = chosen from the sizes alone.  Forward only."""
    lib = _lib.load()
    _req(z, "z"), _req(mu, "mu"), _req(logvar, "logvar")
    if z.dim() != 2 or mu.dim() != 2 or logvar.shape != mu.shape or z.shape[1] != mu.shape[1]:
        raise RuntimeError("agg_posterior_lse: z must be [M, D], mu and logvar [N, D]")
    (M, D), N = z.shape, mu.shape[0]
    splits = 0 if splits is None else int(splits)      # (0, as in the C ABI, is None)
    if splits < 0:
        raise RuntimeError("agg_posterior_lse: splits must not be negative")
    lse_joint = torch.empty(M, dtype=torch.float64, device=z.device)
    lse_dim = torch.empty(M, D, dtype=torch.float32, device=z.device)
    ws = workspace(lib.vg_agg_posterior_workspace_bytes(M, N, D, splits), z.device)
    check(lib.vg_agg_posterior_lse(z.data_ptr(), mu.data_ptr(), logvar.data_ptr(), lse_joint.data_ptr(), lse_dim.data_ptr(),
                                   M, N, D, splits, ws.data_ptr(), ws.numel(), _stream()), "vg_agg_posterior_lse")
    return lse_joint, lse_dim


PAIR_TILE = 64           # VG_PAIR_TILE: rows of a per workgroup and rows of b per column tile, the unit of vg_pair_* splits
PAIR_MAX_K = 8           # VG_PAIR_MAX_K


def _pair_splits_arg(splits, name):
    splits = 0 if splits is None else int(splits)      # (0, as in the C ABI, is None)
    if splits < 0:
        raise RuntimeError(f"{name}: splits must not be negative")
    return splits


def _pair_operands(a, b, name):
    _req(a, "a"), _req(b, "b")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.device != b.device:
        raise RuntimeError(f"{name}: a must be [M, D] and b [N, D] on one device")
    return a.shape[0], b.shape[0], a.shape[1]


def pair_splits(M, N, D, splits=None):
    """The number of column ranges `pair_knn` / `pair_hits` run for these sizes: the launcher's choice for ``None``, else
    the request clamped to the number of column tiles (ceil(N / PAIR_TILE)) with ranges left empty by the rounding
    dropped; 0 for sizes the kernels reject."""
    return int(_lib.load().vg_pair_splits(int(M), int(N), int(D), _pair_splits_arg(splits, "pair_splits")))


def pair_knn(a, b=None, k=1, splits=None):
    """[M, k] fp32: per row of ``a`` [M, D] the ``k`` smallest SQUARED Euclidean distances to the rows of ``b`` [N, D],
    ascending (vg_pair_knn); ``+inf`` where fewer than ``k`` candidates exist.  ``b=None``: ``a``
    against itself with each row's own index excluded (a duplicate row elsewhere still counts, with distance 0).
    ``splits``: the number of column ranges (tests), ``None`` = chosen from the sizes; the bits do not depend on it."""
    k = int(k)
    if not 1 <= k <= PAIR_MAX_K:
        raise ValueError(f"pair_knn: k must be in 1..{PAIR_MAX_K}, got {k}")
    splits = _pair_splits_arg(splits, "pair_knn")
    exclude_self = b is None
    b = a if exclude_self else b
    M, N, D = _pair_operands(a, b, "pair_knn")
    lib = _lib.load()
    out = torch.empty(M, k, dtype=torch.float32, device=a.device)
    ws = workspace(lib.vg_pair_workspace_bytes(M, N, D, k, splits), a.device)
    check(lib.vg_pair_knn(a.data_ptr(), b.data_ptr(), int(exclude_self), out.data_ptr(), M, N, D, k, splits, ws.data_ptr(),
                          ws.numel(), _stream()), "vg_pair_knn")
    return out


def pair_hits(a, b, thr, splits=None):
    """[M] int32: per row i of ``a`` [M, D] the number of rows j of ``b`` [N, D] with squared distance ``<= thr[j]``
    (``thr`` [N] fp32, one threshold per row of ``b``; vg_pair_hits).  ``splits`` as in `pair_knn`."""
    splits = _pair_splits_arg(splits, "pair_hits")
    M, N, D = _pair_operands(a, b, "pair_hits")
    _req(thr, "thr")
    if thr.shape != (N,) or thr.device != a.device:
        raise RuntimeError("pair_hits: thr must be [N], one threshold per row of b, on the operands' device")
    lib = _lib.load()
    count = torch.empty(M, dtype=torch.int32, device=a.device)
    ws = workspace(lib.vg_pair_workspace_bytes(M, N, D, 1, splits), a.device)
    check(lib.vg_pair_hits(a.data_ptr(), b.data_ptr(), thr.data_ptr(), count.data_ptr(), M, N, D, splits, ws.data_ptr(),
                           ws.numel(), _stream()), "vg_pair_hits")
    return count


RECON_BAND_ROWS = 16     # VG_RECON_BAND_ROWS: output rows of the SSIM map per workgroup of vg_recon_quality
RECON_TILE_COLS = 32     # VG_RECON_TILE_COLS: output columns per workgroup
RECON_WINDOWS = (3, 5, 7, 9, 11)


def recon_quality(x, y, data_range=2.0, window=11, sigma=1.5, k1=0.01, k2=0.03):
    """[B, 3] fp64 on the device: per image of ``x`` against ``y`` (contiguous fp32 [B, C, H, W]) the sum of squared
    errors, the mean SSIM and the mean contrast-structure term over the valid positions of a ``window`` x ``window``
    Gaussian window (vg_recon_quality): fp64 window moments, no intermediate of their size, two
    launches, the same bits every run.  ``data_range``: the span L of the pixel values (2 for the tanh decoder's
    [-1, 1]); C1 = (k1 L)^2, C2 = (k2 L)^2.  A batch of any size goes in one call: the images share grid.x."""
    _req(x, "x"), _req(y, "y")
    if x.dim() != 4 or y.shape != x.shape or y.device != x.device:
        raise RuntimeError(f"recon_quality: x and y must be [B, C, H, W] tensors of one shape on one device, got "
                           f"{tuple(x.shape)} and {tuple(y.shape)}")
    window = int(window)
    if window not in RECON_WINDOWS:
        raise ValueError(f"recon_quality: window must be odd and in 3..11, got {window}")
    B, C, H, W = x.shape
    if min(B, C) < 1 or H < window or W < window:
        raise RuntimeError(f"recon_quality: a {window} x {window} window needs B, C >= 1 and H, W >= {window}, got "
                           f"{tuple(x.shape)}")
    for name, v, low in (("sigma", sigma, 0.0), ("data_range", data_range, 0.0), ("k1", k1, None), ("k2", k2, None)):
        v = float(v)
        if not math.isfinite(v) or v < 0.0 or (low is not None and v <= low):
            raise ValueError(f"recon_quality: {name} must be finite and {'positive' if low is not None else 'non-negative'}, got {v}")
    lib = _lib.load()
    nbytes = lib.vg_recon_quality_workspace_bytes(B, C, H, W, window)
    if nbytes == 0:
        raise RuntimeError(f"recon_quality: {tuple(x.shape)} needs more workgroups than one launch holds: score it in pieces")
    out = torch.empty(B, 3, dtype=torch.float64, device=x.device)
    ws = workspace(nbytes, x.device)
    check(lib.vg_recon_quality(x.data_ptr(), y.data_ptr(), out.data_ptr(), B, C, H, W, window, float(sigma),
                               float(data_range), float(k1), float(k2), ws.data_ptr(), ws.numel(), _stream()),
          "vg_recon_quality")
    return out


# ---- differentiable augmentation (csrc/diff_augment.hip) ---------------------------------------
AUGMENT_BITS = {"color": 1, "translation": 2, "cutout": 4}      # VG_AUGMENT_* of include/vaegan_hip.h
AUGMENT_UNIFORMS = 8                                            # uniforms per image: u[B, 8]


def augment_policy(policy):
    """``policy`` -- a comma-separated set of ``"color"``, ``"translation"``, ``"cutout"`` in any order, or its bit set
    1..7 -- as the C ABI's bit set.  TypeError: neither a string nor an int; ValueError: an unknown name, an empty set."""
    if isinstance(policy, bool) or not isinstance(policy, (str, int)):
        raise TypeError(f"diff_augment: policy must be a string of names or a bit set, got {policy!r}")
    if isinstance(policy, int):
        if not 1 <= policy <= 7:
            raise ValueError(f"diff_augment: a policy bit set is in 1..7, got {policy}")
        return policy
    bits = 0
    for name in (n.strip() for n in policy.split(",")):
        if not name:
            continue
        if name not in AUGMENT_BITS:
            raise ValueError(f"diff_augment: unknown policy {name!r} (known: {', '.join(AUGMENT_BITS)})")
        bits |= AUGMENT_BITS[name]
    if not bits:
        raise ValueError(f"diff_augment: the policy names no transform, got {policy!r}")
    return bits


def augment_probability(p):
    """``p`` as a float in [0, 1] (TypeError: no number; ValueError: outside the range, inf or NaN)."""
    try:
        v = float(p)
    except (TypeError, ValueError):
        raise TypeError(f"diff_augment: p must be a number, got {p!r}") from None
    if not (math.isfinite(v) and 0.0 <= v <= 1.0):
        raise ValueError(f"diff_augment: p must be in [0, 1], got {p!r}")
    return v


def _augment_word(p, device):
    """``p`` given as a tensor: the device word of the _dev entry points -- one fp32 element on ``device``."""
    if p.dtype != torch.float32 or p.numel() != 1 or not p.is_cuda or p.device != device:
        raise RuntimeError(f"diff_augment: p as a tensor is ONE float32 word on the images' device, got "
                           f"{tuple(p.shape)} {p.dtype} on {p.device}")
    return p


def _diff_augment(symbol, v, u, policy, p):
    bits, word = augment_policy(policy), isinstance(p, torch.Tensor)
    if not word:
        p = augment_probability(p)
    _req(v, symbol), _req(u, "u")
    if v.dim() != 4 or u.shape != (v.shape[0], AUGMENT_UNIFORMS) or u.device != v.device:
        raise RuntimeError(f"{symbol}: a [B, C, H, W] tensor and u [B, {AUGMENT_UNIFORMS}] on one device, got "
                           f"{tuple(v.shape)} and {tuple(u.shape)}")
    B, C, H, W = v.shape
    lib = _lib.load()
    nbytes = lib.vg_diff_augment_workspace_bytes(B, C, H, W)
    if nbytes == 0:
        raise RuntimeError(f"{symbol}: needs B >= 1, 1 <= C <= 4, H, W >= 2 and an image below 2^31 elements, got {tuple(v.shape)}")
    if word:                                            # (the kernels read it when they run: no host read here)
        symbol, p = symbol + "_dev", _augment_word(p, v.device).data_ptr()
    out = torch.empty_like(v)
    ws = workspace(nbytes, v.device) if bits & AUGMENT_BITS["color"] else None      # (the image sums: the colour step alone)
    check(getattr(lib, symbol)(v.data_ptr(), u.data_ptr(), out.data_ptr(), B, C, H, W, bits, p, _ptr(ws),
                               ws.numel() if ws is not None else 0, _stream()), symbol)
    return out


def diff_augment_fwd(x, u, policy, p=1.0):
    """The augmented batch of ``x`` [B, C, H, W] under the rows of ``u`` [B, 8], uniforms in [0, 1): colour, translation,
    cutout in that order, each if ``policy`` names it, on the images with ``u[:, 7] < p``; the others are copied
    (vg_diff_augment_fwd).  Two launches with the colour step, one without; no bound of the output
    is emitted -- its consumers, the 3-channel convolutions, ask for none.  ``p``: a float in [0, 1], a launch argument --
    or a one-element fp32 DEVICE tensor the kernels read when they run (vg_diff_augment_fwd_dev):
    for the same p the same bits, and a p that moves between replays of a capture."""
    return _diff_augment("vg_diff_augment_fwd", x, u, policy, p)


def diff_augment_bwd(gy, u, policy, p=1.0):
    """The transpose of `diff_augment_fwd`'s linear part applied to ``gy``: it reads ``gy`` and ``u`` alone.  ``p`` as
    there; a device word is read when the backward runs, so it must not change between a forward and its backward."""
    return _diff_augment("vg_diff_augment_bwd", gy, u, policy, p)


# ---- adaptive discriminator augmentation: the controller of p (vg_ada_update) --------------------
ADA_WORDS = ("p", "sign_sum", "count", "calls", "rt", "adjustments")      # vg_ada_state, words 0..5; 6 and 7 are reserved
ADA_FLOAT_WORDS = (0, 4)


def ada_state(device, p0=0.0):
    """The controller's eight words (vg_ada_state) as an int32 tensor on ``device``: word 0 holds the bits of ``p0``, the
    others 0.  ``ada_state(...)[0:1].view(torch.float32)`` is the word `diff_augment_fwd` / `_bwd` take for ``p``."""
    state = torch.zeros(8, dtype=torch.int32)
    state[0:1].view(torch.float32)[0] = augment_probability(p0)
    return state.to(device)


def _ada_state_arg(state):
    if (not isinstance(state, torch.Tensor) or state.dtype != torch.int32 or state.shape != (8,)
            or not state.is_contiguous()):
        raise RuntimeError("ada: state is the contiguous int32 tensor of 8 words that ada_state returns")
    return state


def ada_update(d_real, state, threshold=0.0, target=0.6, rate=2e-6, interval=4):
    """One call of the controller on ``d_real`` (B,), the discriminator's outputs on the real batch: the signs of
    ``d_real - threshold`` are added to ``state``; the ``interval``-th call since the last adjustment forms ``r_t = sign sum /
    count`` and moves p by ``count * rate`` towards ``r_t == target``, clamped to [0, 1] (one launch, one workgroup, no host
    read: capturable).  ``threshold``: 0 for logits, 0.5 for probabilities.  Returns ``state``."""
    _ada_state_arg(state)
    interval, threshold, target, rate = int(interval), float(threshold), float(target), float(rate)
    if interval < 1:
        raise ValueError(f"ada_update: interval must be >= 1, got {interval}")
    if math.isnan(threshold) or not math.isfinite(target) or not (math.isfinite(rate) and rate >= 0.0):
        raise ValueError(f"ada_update: threshold must be a number, target finite, rate finite and >= 0, got "
                         f"{threshold}, {target}, {rate}")
    B = d_real.numel() if isinstance(d_real, torch.Tensor) else 0
    if interval * B >= 1 << 31:
        raise ValueError(f"ada_update: interval * B must stay below 2^31 (the count is an int32), got {interval} * {B}")
    _req(d_real, "d_real")
    if d_real.dim() != 1 or B < 1 or state.device != d_real.device:
        raise RuntimeError(f"ada_update: d_real is a non-empty vector (B,) on the state's device, got {tuple(d_real.shape)}")
    check(_lib.load().vg_ada_update(d_real.data_ptr(), B, threshold, target, rate, interval, state.data_ptr(), _stream()),
          "vg_ada_update")
    return state


def ada_read(state):
    """``{"p", "sign_sum", "count", "calls", "rt", "adjustments"}`` of ``state`` as Python numbers: ONE host read."""
    host = _ada_state_arg(state).cpu()
    floats = host.view(torch.float32)
    return {name: (float(floats[i]) if i in ADA_FLOAT_WORDS else int(host[i])) for i, name in enumerate(ADA_WORDS)}


def reparam_tc_bwd(gz, mu, logvar, eps, z, lse_joint, lse_dim, gloss, beta, alpha, gamma):
    """gz: tensor or None; gloss: 0-dim device tensor (upstream gradient of the weighted loss) or None."""
    lib = _lib.load()
    for t, name in ((mu, "mu"), (logvar, "logvar"), (eps, "eps"), (z, "z"), (lse_dim, "lse_dim")):
        _req(t, name)
    if gz is not None:
        _req(gz, "gz")
    if gloss is not None:
        _req(gloss, "gloss")
    if not lse_joint.is_cuda or lse_joint.dtype != torch.float64 or not lse_joint.is_contiguous():
        raise RuntimeError("reparam_tc_bwd: lse_joint must be the contiguous float64 device tensor of reparam_tc_fwd")
    B, D = mu.shape
    gmu, glv = torch.empty_like(mu), torch.empty_like(mu)
    head = (_ptr(gz), mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), z.data_ptr(), lse_joint.data_ptr(),
            lse_dim.data_ptr(), _ptr(gloss), float(alpha))
    _objective_launch(lib.vg_reparam_tc_workspace_bytes, lib.vg_reparam_tc_bwd, lib.vg_reparam_tc_bwd_dev, mu, head, beta,
                      (float(gamma), gmu.data_ptr(), glv.data_ptr(), B, D))
    return gmu, glv


DIP_VARIANTS = {"i": 1, "ii": 2}      # the C ABI's `variant`: Cov_p[mu(x)] / Cov_q[z]


def dip_variant(variant):
    """``"i"`` / ``"ii"`` (or the C ABI's 1 / 2) -> 1 / 2."""
    v = DIP_VARIANTS.get(variant, variant)
    if isinstance(v, bool) or v not in (1, 2):
        raise ValueError(f"DIP-VAE variant must be 'i' or 'ii', got {variant!r}")
    return int(v)


def reparam_dip_fwd(mu, logvar, eps, beta, lambda_od, lambda_d, variant):
    """Reparameterisation + the DIP-VAE objective (vg_reparam_dip_fwd).  ``beta`` (the KL weight):
    a float or the device word, as `reparam_kl_fwd`; ``lambda_od`` / ``lambda_d``: the weights of the off-diagonal and the
    diagonal penalty; ``variant``: ``"i"`` or ``"ii"``.  Returns ``z``, ``out4`` = [loss, kl, od, dg] and what the backward
    reads (``cov`` [D, D], ``mean`` [D] fp64)."""
    lib = _lib.load()
    _req(mu, "mu"), _req(logvar, "logvar"), _req(eps, "eps")
    if mu.dim() != 2 or logvar.shape != mu.shape or eps.shape != mu.shape:
        raise RuntimeError("reparam_dip: mu, logvar and eps must be [B, D] tensors of one shape")
    variant = dip_variant(variant)
    B, D = mu.shape
    z = torch.empty_like(mu)
    out4 = torch.empty(4, dtype=torch.float32, device=mu.device)
    cov = torch.empty(D, D, dtype=torch.float32, device=mu.device)
    mean = torch.empty(D, dtype=torch.float64, device=mu.device)
    head = (mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), z.data_ptr(), out4.data_ptr(), cov.data_ptr(), mean.data_ptr(),
            B, D, variant)
    _objective_launch(lib.vg_reparam_dip_workspace_bytes, lib.vg_reparam_dip_fwd, lib.vg_reparam_dip_fwd_dev, mu, head, beta,
                      (float(lambda_od), float(lambda_d)))
    return z, out4, cov, mean


def reparam_dip_bwd(gz, mu, logvar, eps, cov, mean, gloss, beta, lambda_od, lambda_d, variant):
    """gz: tensor or None; gloss: 0-dim device tensor (upstream gradient of the weighted loss) or None."""
    lib = _lib.load()
    for t, name in ((mu, "mu"), (logvar, "logvar"), (eps, "eps"), (cov, "cov")):
        _req(t, name)
    if gz is not None:
        _req(gz, "gz")
    if gloss is not None:
        _req(gloss, "gloss")
    B, D = mu.shape
    if not mean.is_cuda or mean.dtype != torch.float64 or not mean.is_contiguous() or mean.numel() != D or cov.shape != (D, D):
        raise RuntimeError("reparam_dip_bwd: cov and mean must be the [D, D] fp32 and [D] float64 tensors of reparam_dip_fwd")
    variant = dip_variant(variant)
    gmu, glv = torch.empty_like(mu), torch.empty_like(mu)
    head = (_ptr(gz), mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), cov.data_ptr(), mean.data_ptr(), _ptr(gloss), variant)
    _objective_launch(lib.vg_reparam_dip_workspace_bytes, lib.vg_reparam_dip_bwd, lib.vg_reparam_dip_bwd_dev, mu, head, beta,
                      (float(lambda_od), float(lambda_d), gmu.data_ptr(), glv.data_ptr(), B, D))
    return gmu, glv


MMD_KERNELS = {"rbf": 1, "imq": 2}      # the C ABI's `kind`: sum_s exp(-d/h_s) / sum_s h_s/(h_s + d)
MMD_MAX_BANDWIDTHS = 8
MMD_IMQ_SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)      # WAE's set, times 2 D sigma_p^2


def mmd_kernel(kernel):
    """``"rbf"`` / ``"imq"`` (or the C ABI's 1 / 2) -> 1 / 2."""
    k = MMD_KERNELS.get(kernel, kernel) if isinstance(kernel, (str, int)) else None
    if isinstance(k, bool) or k not in (1, 2):
        raise ValueError(f"MMD kernel must be 'rbf' or 'imq', got {kernel!r}")
    return int(k)


def mmd_bandwidths(kind, D, bandwidths=None):
    """The bandwidths of the kernel sum as a tuple of floats.  ``None``: WAE's convention with sigma_p^2 = 1 --
    ``(2 D,)`` for rbf, ``2 D (0.1, 0.2, 0.5, 1, 2, 5, 10)`` for imq.  Otherwise 1 to 8 finite positive numbers."""
    if bandwidths is None:
        return (2.0 * D,) if mmd_kernel(kind) == 1 else tuple(2.0 * D * s for s in MMD_IMQ_SCALES)
    try:
        hs = tuple(float(h) for h in bandwidths)
    except TypeError:
        raise ValueError(f"MMD bandwidths must be a sequence of numbers, got {bandwidths!r}") from None
    if not 1 <= len(hs) <= MMD_MAX_BANDWIDTHS or not all(math.isfinite(h) and h > 0.0 for h in hs):
        raise ValueError(f"MMD bandwidths must be 1 to {MMD_MAX_BANDWIDTHS} finite positive numbers, got {bandwidths!r}")
    return hs


def _mmd_host_bandwidths(kind, D, bandwidths):
    hs = mmd_bandwidths(kind, D, bandwidths)
    return (ctypes.c_float * len(hs))(*hs), len(hs)


def reparam_mmd_fwd(mu, logvar, eps, zp, beta, lambda_mmd, kind, bandwidths=None):
    """Reparameterisation + the InfoVAE / WAE-MMD objective (vg_reparam_mmd_fwd).  ``zp``: [B, D]
    draws from the prior; ``beta`` (the KL weight): a float or the device word, as `reparam_kl_fwd`; ``lambda_mmd``: the
    weight of the MMD; ``kind``: ``"rbf"`` or ``"imq"``; ``bandwidths``: as `mmd_bandwidths`.  Returns ``z``, ``out4`` =
    [loss, kl, mmd, kzz] and what the backward reads (``w`` [2, B, B])."""
    lib = _lib.load()
    _req(mu, "mu"), _req(logvar, "logvar"), _req(eps, "eps"), _req(zp, "zp")
    if mu.dim() != 2 or logvar.shape != mu.shape or eps.shape != mu.shape or zp.shape != mu.shape:
        raise RuntimeError("reparam_mmd: mu, logvar, eps and zp must be [B, D] tensors of one shape")
    kind = mmd_kernel(kind)
    B, D = mu.shape
    if B < 2:
        raise RuntimeError("reparam_mmd: the unbiased MMD needs a batch of at least 2")
    hs, n = _mmd_host_bandwidths(kind, D, bandwidths)
    z = torch.empty_like(mu)
    out4 = torch.empty(4, dtype=torch.float32, device=mu.device)
    w = torch.empty(2, B, B, dtype=torch.float32, device=mu.device)
    head = (mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), zp.data_ptr(), z.data_ptr(), out4.data_ptr(), w.data_ptr(),
            B, D, kind)
    _objective_launch(lib.vg_reparam_mmd_workspace_bytes, lib.vg_reparam_mmd_fwd, lib.vg_reparam_mmd_fwd_dev, mu, head, beta,
                      (float(lambda_mmd), ctypes.addressof(hs), n))
    return z, out4, w


def reparam_mmd_bwd(gz, mu, logvar, eps, z, zp, w, gloss, beta, lambda_mmd, kind=None, bandwidths=None):
    """gz: tensor or None; gloss: 0-dim device tensor (upstream gradient of the weighted loss) or None.  The kernel and its
    bandwidths are already in ``w``: ``kind`` / ``bandwidths`` are accepted for symmetry with the forward and only checked."""
    lib = _lib.load()
    for t, name in ((mu, "mu"), (logvar, "logvar"), (eps, "eps"), (z, "z"), (zp, "zp"), (w, "w")):
        _req(t, name)
    if gz is not None:
        _req(gz, "gz")
    if gloss is not None:
        _req(gloss, "gloss")
    B, D = mu.shape
    if w.shape != (2, B, B) or z.shape != mu.shape or zp.shape != mu.shape:
        raise RuntimeError("reparam_mmd_bwd: z, zp and w must be the [B, D], [B, D] and [2, B, B] tensors of reparam_mmd_fwd")
    if kind is not None:
        mmd_bandwidths(mmd_kernel(kind), D, bandwidths)
    gmu, glv = torch.empty_like(mu), torch.empty_like(mu)
    head = (_ptr(gz), mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), z.data_ptr(), zp.data_ptr(), w.data_ptr(), _ptr(gloss))
    _objective_launch(lib.vg_reparam_mmd_workspace_bytes, lib.vg_reparam_mmd_bwd, lib.vg_reparam_mmd_bwd_dev, mu, head, beta,
                      (float(lambda_mmd), gmu.data_ptr(), glv.data_ptr(), B, D))
    return gmu, glv


def kl_free_bits(free_bits):
    """The per-dimension floor as the C ABI's float: finite and >= 0."""
    v = float(free_bits)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"free_bits must be finite and >= 0, got {free_bits!r}")
    return v


def reparam_klc_fwd(mu, logvar, eps, beta, capacity, free_bits):
    """Reparameterisation + the controlled KL term (vg_reparam_klc_fwd): ``loss = beta * |T - B *
    capacity|`` with ``T`` the sum over the dimensions of ``max(K[d], B * free_bits)``, ``K[d]`` the dimension's KL summed over
    the batch.  ``beta`` and ``capacity`` (nats per sample, >= 0): both floats, or both one-element fp32 device words read by
    the kernel; ``free_bits``: a float, nats per dimension per sample.  Returns ``z``, ``out4`` = [loss, kl, T, dims above the
    floor], ``gate`` [D] (what the backward reads: sgn(T - B capacity) where a dimension is above its floor, else 0) and
    ``kl_dim`` [D] = K / B."""
    lib = _lib.load()
    _req(mu, "mu"), _req(logvar, "logvar"), _req(eps, "eps")
    if mu.dim() != 2 or logvar.shape != mu.shape or eps.shape != mu.shape:
        raise RuntimeError("reparam_klc: mu, logvar and eps must be [B, D] tensors of one shape")
    B, D = mu.shape
    z = torch.empty_like(mu)
    out4 = torch.empty(4, dtype=torch.float32, device=mu.device)
    gate = torch.empty(D, dtype=torch.float32, device=mu.device)
    kl_dim = torch.empty(D, dtype=torch.float32, device=mu.device)
    head = (mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), z.data_ptr(), out4.data_ptr(), gate.data_ptr(), kl_dim.data_ptr(),
            B, D)
    _objective_launch(lib.vg_reparam_klc_workspace_bytes, lib.vg_reparam_klc_fwd, lib.vg_reparam_klc_fwd_dev, mu, head, beta,
                      (kl_free_bits(free_bits),), second=("capacity", capacity))
    return z, out4, gate, kl_dim


def reparam_klc_bwd(gz, mu, logvar, eps, gate, gloss, beta, capacity, free_bits):
    """gz: tensor or None; gloss: 0-dim device tensor (upstream gradient of the weighted loss) or None.  The sign and the
    floor are already in ``gate``: ``capacity`` / ``free_bits`` are taken for symmetry with the forward and only checked."""
    lib = _lib.load()
    for t, name in ((mu, "mu"), (logvar, "logvar"), (eps, "eps"), (gate, "gate")):
        _req(t, name)
    if gz is not None:
        _req(gz, "gz")
    if gloss is not None:
        _req(gloss, "gloss")
    B, D = mu.shape
    if gate.shape != (D,):
        raise RuntimeError("reparam_klc_bwd: gate must be the [D] tensor of reparam_klc_fwd")
    gmu, glv = torch.empty_like(mu), torch.empty_like(mu)
    head = (_ptr(gz), mu.data_ptr(), logvar.data_ptr(), eps.data_ptr(), gate.data_ptr(), _ptr(gloss))
    _objective_launch(lib.vg_reparam_klc_workspace_bytes, lib.vg_reparam_klc_bwd, lib.vg_reparam_klc_bwd_dev, mu, head, beta,
                      (kl_free_bits(free_bits), gmu.data_ptr(), glv.data_ptr(), B, D), second=("capacity", capacity))
    return gmu, glv


PERMUTE_MAX_BATCH = 2048      # VG_PERMUTE_MAX_BATCH: the rows of a 16-column strip of fp32 that fit the CU's LDS (128 of 160 KiB)


def permute_dims(z, u):
    """``z_perm[i, d] = z[pi_d[i], d]`` with ``pi_d`` the stable ascending argsort of ``u[:, d]`` (vg_permute_dims, DESIGN.md
    section 4.32): every column of ``z`` [B, D] permuted across the batch on its own, as ``z.gather(0, torch.argsort(u, dim=0,
    stable=True))`` -- in one launch, the same bits every run.  ``u``: [B, D] fp32, U[0, 1) draws.  ``ValueError`` for a batch
    above `PERMUTE_MAX_BATCH`.  Forward only."""
    lib = _lib.load()
    _req(z, "z"), _req(u, "u")
    if z.dim() != 2 or u.shape != z.shape or z.numel() == 0:
        raise RuntimeError(f"permute_dims: z and u must be [B, D] tensors of one shape, got {tuple(z.shape)} and {tuple(u.shape)}")
    B, D = z.shape
    if B > PERMUTE_MAX_BATCH:
        raise ValueError(f"permute_dims: a batch of {B} is above {PERMUTE_MAX_BATCH}, the rows of a 16-column strip that fit "
                         "the LDS of one compute unit")
    z_perm = torch.empty_like(z)
    check(lib.vg_permute_dims(z.data_ptr(), u.data_ptr(), z_perm.data_ptr(), B, D, _stream()), "vg_permute_dims")
    return z_perm


def _req_logits(logits, name):
    _req(logits, name)
    if logits.dim() != 2 or logits.shape[1] != 2 or logits.shape[0] < 1:
        raise RuntimeError(f"{name}: expected the critic's [rows, 2] logits, got {tuple(logits.shape)}")
    return logits


def factor_tc_fwd(logits, kl, beta, gamma):
    """The encoder phase's FactorVAE loss (vg_factor_tc_fwd) from the critic's ``logits`` [B, 2] on z and
    ``kl``, the 0-dim device tensor of the unweighted KL: ``out4 = [beta * kl + gamma * tc, kl, tc, rows with l0 > l1]``, ``tc =
    sum_b (l0 - l1)``.  ``beta`` and ``gamma``: both floats, or both one-element fp32 device words read by the kernel."""
    lib = _lib.load()
    _req_logits(logits, "logits"), _req(kl, "kl")
    if kl.numel() != 1:
        raise RuntimeError("factor_tc: kl is the one-element tensor of the KL summed over the batch")
    out4 = torch.empty(4, dtype=torch.float32, device=logits.device)
    head = (logits.data_ptr(), kl.data_ptr(), out4.data_ptr(), logits.shape[0])
    _objective_launch(lib.vg_factor_tc_workspace_bytes, lib.vg_factor_tc_fwd, lib.vg_factor_tc_fwd_dev, logits, head, beta, (),
                      second=("gamma", gamma))
    return out4


def factor_tc_bwd(logits, gloss, beta, gamma):
    """``(glogits, gkl)`` of `factor_tc_fwd`: the constant ``+-gamma * gloss`` per row and ``beta * gloss``.  ``logits`` gives the
    shape; ``gloss``: 0-dim device tensor, the upstream gradient of ``out4[0]``."""
    lib = _lib.load()
    _req_logits(logits, "logits"), _req(gloss, "gloss")
    glogits = torch.empty_like(logits)
    gkl = torch.empty((), dtype=torch.float32, device=logits.device)
    _objective_launch(lib.vg_factor_tc_workspace_bytes, lib.vg_factor_tc_bwd, lib.vg_factor_tc_bwd_dev, logits,
                      (gloss.data_ptr(),), beta, (glogits.data_ptr(), gkl.data_ptr(), logits.shape[0]), second=("gamma", gamma))
    return glogits, gkl


def factor_critic_loss(logits, divisor=None, want_grad=True):
    """The critic phase's cross-entropy (vg_factor_critic_loss) on ``logits`` [2B, 2] -- the first B rows
    are z (class 0), the last B permuted (class 1): ``(loss, glogits, acc)`` with ``loss = sum softplus(other - own) / divisor``
    (default: the 2B rows, a mean), its gradient (None without ``want_grad``) and the fraction of the rows on the right side
    of 0 (a tie is wrong), in one launch."""
    lib = _lib.load()
    _req_logits(logits, "logits")
    rows = logits.shape[0]
    if rows % 2:
        raise RuntimeError(f"factor_critic_loss: the rows are [z; z_perm], an even number, got {rows}")
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    acc = torch.empty((), dtype=torch.float32, device=logits.device)
    glogits = torch.empty_like(logits) if want_grad else None
    check(lib.vg_factor_critic_loss(logits.data_ptr(), loss.data_ptr(), _ptr(glogits), acc.data_ptr(), rows // 2,
                                    float(divisor if divisor is not None else rows), _stream()), "vg_factor_critic_loss")
    return loss, glogits, acc


def sqdiff_loss(a, b, scale, gscale=1.0, want_grad=True):
    lib = _lib.load()
    _req(a, "a"), _req(b, "b")
    if a.shape != b.shape:
        raise RuntimeError("sqdiff_loss: shape mismatch")
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    ga = torch.empty_like(a) if want_grad else None
    ws = workspace(lib.vg_sqdiff_workspace_bytes(a.numel()), a.device)
    check(lib.vg_sqdiff_loss(a.data_ptr(), b.data_ptr(), loss.data_ptr(), _ptr(ga), a.numel(), float(scale),
                             float(gscale), ws.data_ptr(), ws.numel(), _stream()), "vg_sqdiff_loss")
    return loss, ga


def bce_loss(p, target, divisor=None, gscale=1.0, want_grad=True):
    """``target``: a Python float, or a one-element fp32 DEVICE tensor (a label that changes between replays of a
    captured iteration: the kernel reads it from memory)."""
    lib = _lib.load()
    _req(p, "p")
    B = p.numel()
    loss = torch.empty((), dtype=torch.float32, device=p.device)
    gp = torch.empty_like(p) if want_grad else None
    div = float(divisor if divisor is not None else B)
    if isinstance(target, torch.Tensor):
        _req(target, "target")
        if target.numel() != 1:
            raise RuntimeError("bce_loss: a device label is one fp32 value")
        check(lib.vg_bce_loss_dev(p.data_ptr(), target.data_ptr(), loss.data_ptr(), _ptr(gp), B, div, float(gscale),
                                  _stream()), "vg_bce_loss_dev")
    else:
        check(lib.vg_bce_loss(p.data_ptr(), float(target), loss.data_ptr(), _ptr(gp), B, div, float(gscale), _stream()),
              "vg_bce_loss")
    return loss, gp


def dot_sigmoid_bce_fwd(feat, w, bias, target, divisor=None, want_grad=True):
    """The discriminator's head + its BCE in one launch: p = sigmoid(feat @ w + bias) (B,), the mean BCE of
    p against ``target`` (float or one-element device tensor) over ``divisor``, and dlogit = d loss / d logit."""
    lib = _lib.load()
    _req(feat, "feat"), _req(w, "w")
    B, K = feat.shape
    if w.numel() != K:
        raise RuntimeError("dot_sigmoid_bce: weight does not match the features")
    p = torch.empty(B, dtype=torch.float32, device=feat.device)
    loss = torch.empty((), dtype=torch.float32, device=feat.device)
    dlogit = torch.empty(B, dtype=torch.float32, device=feat.device) if want_grad else None
    dev = isinstance(target, torch.Tensor)
    if dev:
        _req(target, "target")
    ws = workspace(lib.vg_dot_sigmoid_bce_workspace_bytes(B), feat.device)
    check(lib.vg_dot_sigmoid_bce_fwd(feat.data_ptr(), w.data_ptr(), _ptr(bias), 0.0 if dev else float(target),
                                     target.data_ptr() if dev else None, p.data_ptr(), loss.data_ptr(), _ptr(dlogit), B, K,
                                     float(divisor if divisor is not None else B), ws.data_ptr(), ws.numel(), _stream()),
          "vg_dot_sigmoid_bce_fwd")
    return p, loss, dlogit


def dot_sigmoid_bce_bwd(dlogit, gloss, feat, w, need_feat=True, need_w=True, need_b=True, accumulate_into=None):
    """``accumulate_into`` = (gw, gb) tensors the parameter gradients are added to (see bn_act_bwd)."""
    lib = _lib.load()
    B, K = feat.shape
    gfeat = torch.empty_like(feat) if need_feat else None
    if accumulate_into is not None:
        gw, gb = accumulate_into
    else:
        gw = torch.empty(w.shape, dtype=torch.float32, device=feat.device) if need_w else None
        gb = torch.empty(1, dtype=torch.float32, device=feat.device) if need_b else None
    check(lib.vg_dot_sigmoid_bce_bwd(dlogit.data_ptr(), _ptr(gloss), feat.data_ptr(), w.data_ptr(), _ptr(gfeat), _ptr(gw),
                                     _ptr(gb), B, K, 1 if accumulate_into is not None else 0, _stream()),
          "vg_dot_sigmoid_bce_bwd")
    return gfeat, gw, gb


# adversarial losses on the logit (VG_GAN_* of include/vaegan_hip.h)
GAN_LOGISTIC, GAN_LSGAN, GAN_HINGE_REAL, GAN_HINGE_FAKE, GAN_HINGE_GEN = range(5)


def _gan_kind(kind, name):
    if isinstance(kind, bool) or not isinstance(kind, int) or not GAN_LOGISTIC <= kind <= GAN_HINGE_GEN:
        raise RuntimeError(f"{name}: kind is one of the five GAN_* codes, got {kind!r}")
    return kind


def _gan_label(target, name):
    """(host value, device pointer) of a label: a Python float, or a one-element fp32 DEVICE tensor (bce_loss)."""
    if isinstance(target, torch.Tensor):
        _req(target, "target")
        if target.numel() != 1:
            raise RuntimeError(f"{name}: a device label is one fp32 value")
        return 0.0, target.data_ptr()
    return float(target), None


def gan_loss(logit, kind, target, divisor=None, gscale=1.0, want_grad=True):
    """A GAN loss of the logit vector ``logit`` (B,) against ``target`` (as in `bce_loss`; the hinge kinds ignore it):
    (p = sigmoid(logit), loss, gscale * d loss / d logit)."""
    lib = _lib.load()
    _req(logit, "logit")
    kind = _gan_kind(kind, "gan_loss")
    B = logit.numel()
    p = torch.empty(B, dtype=torch.float32, device=logit.device)
    loss = torch.empty((), dtype=torch.float32, device=logit.device)
    glogit = torch.empty_like(logit) if want_grad else None
    host, dev = _gan_label(target, "gan_loss")
    check(lib.vg_gan_loss(logit.data_ptr(), kind, host, dev, p.data_ptr(), loss.data_ptr(), _ptr(glogit), B,
                          float(divisor if divisor is not None else B), float(gscale), _stream()), "vg_gan_loss")
    return p, loss, glogit


def dot_gan_loss_fwd(feat, w, bias, kind, target, divisor=None, want_grad=True):
    """The discriminator's head + a GAN loss of its logit in one launch: logit = feat @ w + bias (B,), p = sigmoid(logit)
    (for logging), the loss of ``kind`` against ``target`` (float or one-element device tensor) summed over the rows and
    divided by ``divisor``, and dlogit = d loss / d logit -- what `dot_sigmoid_bce_bwd` takes."""
    lib = _lib.load()
    _req(feat, "feat"), _req(w, "w")
    kind = _gan_kind(kind, "dot_gan_loss")
    B, K = feat.shape
    if w.numel() != K:
        raise RuntimeError("dot_gan_loss: weight does not match the features")
    if bias is not None:
        _req(bias, "bias")
    logit = torch.empty(B, dtype=torch.float32, device=feat.device)
    p = torch.empty(B, dtype=torch.float32, device=feat.device)
    loss = torch.empty((), dtype=torch.float32, device=feat.device)
    dlogit = torch.empty(B, dtype=torch.float32, device=feat.device) if want_grad else None
    host, dev = _gan_label(target, "dot_gan_loss")
    ws = workspace(lib.vg_dot_gan_loss_workspace_bytes(B), feat.device)
    check(lib.vg_dot_gan_loss_fwd(feat.data_ptr(), w.data_ptr(), _ptr(bias), kind, host, dev, logit.data_ptr(), p.data_ptr(),
                                  loss.data_ptr(), _ptr(dlogit), B, K, float(divisor if divisor is not None else B),
                                  ws.data_ptr(), ws.numel(), _stream()), "vg_dot_gan_loss_fwd")
    return logit, p, loss, dlogit


# ---------------------------------------------------------------- image I/O
def u8_gather_normalize(images_u8, index, mean=0.5, std=0.5):
    """images_u8 [N,H,W,C] uint8 (device), index int64 (device) -> fp32 [B,C,H,W] =
    (u8 / 255 - mean) / std  (ToTensor + Normalize, dataset.py:37-43)."""
    lib = _lib.load()
    if not (isinstance(images_u8, torch.Tensor) and images_u8.is_cuda and images_u8.dtype == torch.uint8
            and images_u8.dim() == 4 and images_u8.is_contiguous()):
        raise RuntimeError("u8_gather_normalize: image cache must be a contiguous CUDA/ROCm uint8 [N,H,W,C] tensor")
    if not (isinstance(index, torch.Tensor) and index.is_cuda and index.dtype == torch.int64 and index.dim() == 1):
        raise RuntimeError("u8_gather_normalize: index must be a 1-D CUDA/ROCm int64 tensor")
    index = index.contiguous()
    N, H, W, C = images_u8.shape
    B = index.numel()
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=images_u8.device)
    for s in range(0, B, 65535):                      # grid.y limit
        n = min(65535, B - s)
        check(lib.vg_u8_gather_normalize(images_u8.data_ptr(), index.data_ptr() + 8 * s, out[s:].data_ptr(), n, C, H, W,
                                         float(mean), float(std), _stream()), "vg_u8_gather_normalize")
    return out


def minmax(x):
    """Device tensor [min(x), max(x)] (no host sync)."""
    lib = _lib.load()
    _req(x, "x")
    n = x.numel()
    nbytes = lib.vg_minmax_workspace_bytes(n)
    ws = workspace(nbytes, x.device)
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    check(lib.vg_minmax(x.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "vg_minmax")
    return out


def image_grid_u8(x, nrow=8, padding=2, normalize=False, pad_value=0.0):
    """torchvision 0.2.1 make_grid + save_image quantisation on the device: x [B,C,H,W] (C = 1 or 3)
    -> uint8 [GH,GW,3]."""
    lib = _lib.load()
    _req(x, "x")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    B, C, H, W = x.shape
    gh, gw = ctypes.c_int(), ctypes.c_int()
    check(lib.vg_image_grid_shape(B, H, W, nrow, padding, ctypes.byref(gh), ctypes.byref(gw)), "vg_image_grid_shape")
    mm = minmax(x) if normalize else None
    grid = torch.empty((gh.value, gw.value, 3), dtype=torch.uint8, device=x.device)
    check(lib.vg_image_grid_u8(x.data_ptr(), _ptr(mm), grid.data_ptr(), B, C, H, W, nrow, padding, float(pad_value),
                               _stream()), "vg_image_grid_u8")
    return grid


# ------------------------------------- decoder output -> FID features on the device (csrc/fid_front.hip)
POOL_MAX, POOL_AVG_EXCLUDE_PAD = 0, 1      # VG_POOL_* of include/vaegan_hip.h


def _req_u8_images(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{name}: disentangle_mlp_amd ops need CUDA/ROCm tensors (no CPU fallback)")
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous uint8 [B,H,W,3] tensor, got {t.dtype} {tuple(t.shape)}")
    return t


def quantize_each_u8(x):
    """``save_image(x[i], normalize=True)`` for every image of x [B,C,H,W] (C = 1 or 3) at once -> uint8 [B,H,W,3] on the
    device: bit-identical to ``image_grid_u8(x[i], normalize=True)`` per image, in two launches for the batch."""
    _req(x, "x")
    lib = _lib.load()
    if x.dim() != 4 or x.shape[1] not in (1, 3):
        raise RuntimeError(f"quantize_each_u8: expected [B,C,H,W] with C = 1 or 3, got {tuple(x.shape)}")
    B, C, H, W = x.shape
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device)
    for s in range(0, B, 65535):                      # grid.y limit
        n = min(65535, B - s)
        ws = workspace(8 * n, x.device)
        check(lib.vg_quantize_each_u8(x[s:].data_ptr(), out[s:].data_ptr(), n, C, H, W, ws.data_ptr(), ws.numel(),
                                      _stream()), "vg_quantize_each_u8")
    return out


def resize_bilinear_u8(images_u8, size=(299, 299), scale=2.0, shift=-1.0):
    """images_u8 [B,H,W,3] uint8 (device) -> fp32 [B,3,OH,OW] = scale * bilinear(u8 / 255) + shift
    (``F.interpolate(mode="bilinear", align_corners=False)`` + ``normalize_input``); the result carries its bound."""
    _req_u8_images(images_u8, "resize_bilinear_u8")
    lib = _lib.load()
    B, H, W, _ = images_u8.shape
    OH, OW = _pair(size)
    if B > 65535:
        raise RuntimeError("resize_bilinear_u8: at most 65535 images per call")
    y = torch.empty((B, 3, OH, OW), dtype=torch.float32, device=images_u8.device)
    slot = new_amax_slot(y.device)
    check(lib.vg_resize_bilinear_u8(images_u8.data_ptr(), y.data_ptr(), B, H, W, OH, OW, float(scale), float(shift),
                                    slot.data_ptr(), _stream()), "vg_resize_bilinear_u8")
    set_amax(y, slot)
    return y


def pool3x3(x, stride, padding, mode, out=None, out_channel_offset=0, amax=None):
    """3x3 pooling of x [B,C,H,W]: ``mode`` "max" (``F.max_pool2d``: padding reads as -inf) or "avg"
    (``F.avg_pool2d(count_include_pad=False)``), stride 1 or 2, padding 0 or 1.  ``out``: a contiguous (B, Ctot, OH, OW)
    tensor; channels [out_channel_offset, out_channel_offset + C) are written, the others are not touched.  ``amax``: the
    bound slot max |out| is added to (a new one by default); the returned view of the written channels carries it."""
    _req(x, "x")
    lib = _lib.load()
    if x.dim() != 4 or mode not in ("max", "avg"):
        raise RuntimeError(f"pool3x3: expected a [B,C,H,W] input and mode 'max' or 'avg', got {tuple(x.shape)}, {mode!r}")
    B, C, H, W = x.shape
    stride, padding = int(stride), int(padding)
    if stride not in (1, 2) or padding not in (0, 1) or H + 2 * padding < 3 or W + 2 * padding < 3 or B > 65535:
        raise RuntimeError(f"pool3x3: stride {stride}, padding {padding} on {tuple(x.shape)} is not taken")
    OH, OW = (H + 2 * padding - 3) // stride + 1, (W + 2 * padding - 3) // stride + 1
    if out is None:
        out = torch.empty((B, C, OH, OW), dtype=torch.float32, device=x.device)
    else:
        _req(out, "out")
        if out.dim() != 4 or (out.shape[0], out.shape[2], out.shape[3]) != (B, OH, OW) or \
                not 0 <= out_channel_offset <= out.shape[1] - C:
            raise RuntimeError(f"pool3x3: out {tuple(out.shape)} cannot take channels [{out_channel_offset}, "
                               f"{out_channel_offset + C}) of a (B={B}, {OH}x{OW}) output")
    slot = amax if amax is not None else new_amax_slot(x.device)
    check(lib.vg_pool3x3(x.data_ptr(), out.data_ptr(), B, C, H, W, stride, padding,
                         POOL_MAX if mode == "max" else POOL_AVG_EXCLUDE_PAD, out.shape[1], out_channel_offset,
                         slot.data_ptr(), _stream()), "vg_pool3x3")
    view = out[:, out_channel_offset:out_channel_offset + C]
    set_amax(view, slot)
    return view


def global_avg_pool(x, out=None):
    """x [B,C,...] -> [B,C]: the mean over everything behind the channel axis (``adaptive_avg_pool2d(x, (1, 1))``), one
    wavefront per (b, c) in a fixed summation order.  ``out``: a contiguous [B,C] tensor to write (rows of a larger one)."""
    _req(x, "x")
    lib = _lib.load()
    if x.dim() < 3:
        raise RuntimeError(f"global_avg_pool: expected [B,C,...], got {tuple(x.shape)}")
    B, C = x.shape[0], x.shape[1]
    y = torch.empty((B, C), dtype=torch.float32, device=x.device) if out is None else _req(out, "out")
    if tuple(y.shape) != (B, C):
        raise RuntimeError(f"global_avg_pool: out {tuple(y.shape)} does not match ({B}, {C})")
    check(lib.vg_global_avg_pool(x.data_ptr(), y.data_ptr(), B, C, x.numel() // (B * C), _stream()), "vg_global_avg_pool")
    return y
