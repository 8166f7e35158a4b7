// What the three MFMA forward kernels of the 5x5 / pad 2 / stride {1,2} convolutions share (conv_igemm.hip: exact fp32;
// conv_bf16split.hip: split arithmetic, stride 1 and the thin transposed layers; conv_ring.hip: split arithmetic, stride 2):
// the tap algebra of the parity classes, workgroup -> tile placement, the fragment-pixel decode, the clamped patch address,
// the class dispatch and the host-side tile geometry.  Everything is constexpr or __forceinline__ and holds no state; the
// staging maps, LDS layouts, MFMA loops and -- measured, DESIGN.md section 4.28 -- the output epilogues stay in the kernels.
// Below them, what the weight-gradient and <= 3-channel kernels share with them and with each other (DESIGN.md section
// 4.29; conv_wgrad.hip, wgrad_bf16split.hip, conv_thin_wgrad.hip, conv_thin_fwd.hip, conv_thin_mfma.hip): the shape
// predicate and out_dim, the host side of an affine-on-load operand, the weight-gradient argument blocks, the chunk
// decode and the partial-slab store.  The arithmetic pieces (plane split, product order, affine_act) are in common.hpp.
//
// A tile configuration C (Cfg / XCfg / RCfg) names MODE, S, NB, TH, TW, TN, WC, WP, FC, FP: a workgroup computes TN output
// channels x NB * TH * TW pixels of the tile space (forward: the output; transposed: the input, one output-parity class at
// a time) with WC x WP wavefronts of FC x FP fragments of 32 x 32.
#pragma once
#include "common.hpp"
#include "vaegan_hip.h"

enum { CONV_FWD = 0, CONV_TR = 1 };

// ---- tap algebra ------------------------------------------------------------------------------------------------------
// The stride-S transposed convolution runs as its S * S output-parity classes: output (S*i + R, S*j + SS) sums the taps
// (kh, kw) = (R + S*a, SS + S*b) only -- 3x3, 3x2, 2x3, 2x2 taps for S = 2: no zero insertion, no atomics.  Classes are
// ordered (R, SS) row-major, in the packed filters and in the grid (class 0, the heaviest, first).
__host__ __device__ constexpr int class_taps(int S, int r) { return (5 - r + S - 1) / S; }      // taps along one dimension
__host__ __device__ constexpr int class_taps_before(int S, int R, int SS) {                    // taps of the classes before (R, SS)
  int n = 0;
  for (int r = 0; r < S; ++r)
    for (int s = 0; s < S; ++s) {
      if (r == R && s == SS) return n;
      n += class_taps(S, r) * class_taps(S, s);
    }
  return n;
}

// Taps and input patch of a TH x TW tile.  The forward convolution walks all 25 taps as one class.
template <int MODE, int S, int TH, int TW>
struct TileTaps {
  static constexpr int NCLS = (MODE == CONV_FWD) ? 1 : S * S;
  static constexpr int NTMAX = (MODE == CONV_FWD) ? 5 : class_taps(S, 0);      // taps per dimension, largest class
  static constexpr int PH = (MODE == CONV_FWD) ? S * (TH - 1) + 5 : TH + NTMAX - 1;
  static constexpr int PW = (MODE == CONV_FWD) ? S * (TW - 1) + 5 : TW + NTMAX - 1;
  static constexpr int PSTEP = (MODE == CONV_FWD) ? S : 1;                     // patch rows / columns per tile pixel
  static constexpr int ORG = (MODE == CONV_FWD) ? 2 : NTMAX - 1 - 2 / S;       // patch origin = PSTEP * tile origin - ORG
  static constexpr int nth(int R) { return (MODE == CONV_FWD) ? 5 : class_taps(S, R); }      // taps along h / w of a class
};

// 16-byte units per patch row of the channel-innermost split-arithmetic patches.  Chosen so that the patch rows a
// 32-pixel fragment spans start on disjoint groups of 16 units (= 256 B, one LDS bank row):
// fragments of 2 rows x 16 pixels need the two rows 0 (mod 16) apart, 4 rows x 8 pixels 8 (mod 16).
constexpr int row_units(int TW, int PW) {
  if (TW == 16) return (PW + 15) & ~15;
  if (TW == 8) { int c = PW; while ((c & 15) != 8) ++c; return c; }
  return (PW + 3) & ~3;
}

// Padded cout extent of every packed filter: whole 128-channel tiles.
__host__ __device__ constexpr int packed_cout(int Cout) { return (Cout + 127) & ~127; }

// ---- what every kernel's argument block starts with (filled by fill_geom) ----------------------------------------------
struct ConvGeom {
  const float* x;
  const float* bias;
  float* y;
  int B, Cin, XH, XW, Cout, YH, YW;
  int ntiles_n, tiles_w, tiles_hw, blocks_per_cls;
};

// ---- placement ---------------------------------------------------------------------------------------------------------
// Workgroup `bid` of a class -> (cout tile nt, pixel tile pt).  XCD-aware: workgroups are dealt round-robin over the 8
// XCDs (bid % 8 labels the XCD, each with its own L2).  The ntiles_n cout tiles that read the SAME input patch are given
// to ONE XCD, back to back, so the patch is fetched from HBM once and re-read from that L2; every XCD streams the whole
// (L2-sized) filter.  RUNS (conv_ring.hip): an XCD works through a contiguous run of pixel tiles -- neighbours in the
// image (shared halo rows, shared cache lines of a row) follow each other through the same L2.  Placement affects speed only.
template <bool RUNS>
__device__ __forceinline__ void place_tile(int bid, int ntn, int blocks_per_cls, int& nt, int& pt) {
  const int npatch = blocks_per_cls / ntn, full = (npatch / 8) * 8 * ntn;
  if (bid < full) {
    const int xcd = bid & 7, j = bid >> 3;
    pt = RUNS ? xcd * (npatch / 8) + j / ntn : (j / ntn) * 8 + xcd;
    nt = j % ntn;
  } else {
    const int t = bid - full;
    pt = (npatch / 8) * 8 + t / ntn;
    nt = t % ntn;
  }
}

struct TileOrigin {
  int th0, tw0;      // first row / column of the tile (tile space)
  int b0, n0;        // first image, first output channel
  int ih0, iw0;      // patch origin in input coordinates
};
template <class C>
__device__ __forceinline__ TileOrigin tile_origin(int pt, int nt, const ConvGeom& A) {
  using T = TileTaps<C::MODE, C::S, C::TH, C::TW>;
  const int sp = pt % A.tiles_hw, bg = pt / A.tiles_hw;
  TileOrigin org;
  org.th0 = (sp / A.tiles_w) * C::TH;
  org.tw0 = (sp % A.tiles_w) * C::TW;
  org.b0 = bg * C::NB;
  org.n0 = nt * C::TN;
  org.ih0 = org.th0 * T::PSTEP - T::ORG;
  org.iw0 = org.tw0 * T::PSTEP - T::ORG;
  return org;
}

// ---- fragment pixel: lane l32 of pixel fragment f of wavefront column wp -> (image, row, column) within the tile -------
struct FragPixel { int nb, row, col; };
template <class C>
__device__ __forceinline__ FragPixel frag_pixel(int wp, int f, int l32) {
  const int m = (wp * C::FP + f) * 32 + l32;
  const int r = m % (C::TH * C::TW);
  return {m / (C::TH * C::TW), r / C::TW, r % C::TW};
}

// ---- patch element (nb, r, col) of the tile's input patch: offset of its channel 0 from image b0, and validity.  Every
// load address is CLAMPED into the tensor (distinct, always valid) instead of being predicated: the prefetch is
// straight-line code with no dependent or merged loads (predicated loads made hipcc merge the dummy loads and drain vmcnt
// in the middle of the prefetch); halo / tail elements (`in` false: not an element of the patch) are replaced by 0 when
// the registers are written to LDS.
struct PatchElem { int ofs; bool ok; };
__device__ __forceinline__ PatchElem patch_elem(const ConvGeom& A, const TileOrigin& org, int nb, int r, int col, bool in) {
  const int ih = org.ih0 + r, iw = org.iw0 + col;
  PatchElem e;
  e.ok = in && ih >= 0 && ih < A.XH && iw >= 0 && iw < A.XW && (org.b0 + nb) < A.B;
  const int nbc = min(nb, A.B - 1 - org.b0), ihc = min(max(ih, 0), A.XH - 1), iwc = min(max(iw, 0), A.XW - 1);
  e.ofs = nbc * A.Cin * (A.XH * A.XW) + ihc * A.XW + iwc;
  return e;
}

// ---- run-time value -> compile-time argument of a generic lambda --------------------------------------------------------
// class 0..3 of the stride-2 transposed convolution -> f(IntC<R>, IntC<SS>)
template <class F>
__device__ __forceinline__ void for_class(int cls, F&& f) {
  switch (cls) {
    case 0: f(IntC<0>{}, IntC<0>{}); break;
    case 1: f(IntC<0>{}, IntC<1>{}); break;
    case 2: f(IntC<1>{}, IntC<0>{}); break;
    default: f(IntC<1>{}, IntC<1>{}); break;
  }
}

// `planes` of the C ABI (2 / 3 bf16 planes, or VG_PLANES_F16 | 2) -> f(IntC<NP>, IntC<F16>); stride 1 / 2 -> f(IntC<S>)
inline int planes_ok(int planes) { return planes == 2 || planes == 3 || planes == (VG_PLANES_F16_FLAG | 2); }
template <class F>
int for_planes(int planes, F&& f) {
  if (planes & VG_PLANES_F16_FLAG) return f(IntC<2>{}, IntC<1>{});
  if (planes == 2) return f(IntC<2>{}, IntC<0>{});
  return f(IntC<3>{}, IntC<0>{});
}
template <class F>
int for_stride(int stride, F&& f) {
  return stride == 2 ? f(IntC<2>{}) : f(IntC<1>{});
}

// ---- host geometry -----------------------------------------------------------------------------------------------------
// the shape every 5x5 / pad 2 entry point takes (each adds its own conditions), and the output extent of a stride-S
// convolution along a dimension of X input elements
inline bool conv_shape_ok(int B, int Cin, int H, int W, int Cout, int stride) {
  return B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2);
}
constexpr int out_dim(int X, int S) { return (X - 1) / S + 1; }
// extent of the tile space / of the output along a dimension of X input elements
constexpr int tile_extent(int mode, int S, int X) { return (mode == CONV_FWD) ? out_dim(X, S) : X; }
constexpr int out_extent(int mode, int S, int X) { return (mode == CONV_FWD) ? out_dim(X, S) : X * S; }

// An operand with an affine + activation applied on load (common.hpp, affine_act): scale and shift come together, act is
// a VG_ACT_*.  Returns the slope act_slope takes -- 1 where there is nothing to apply -- or a negative value: bad argument.
inline float affine_on_load_slope(const float* scale, const float* shift, int act) {
  if ((scale == nullptr) != (shift == nullptr) || act < VG_ACT_NONE || act > VG_ACT_LRELU) return -1.f;
  return (!scale || act == VG_ACT_NONE) ? 1.f : (act == VG_ACT_RELU ? 0.f : 0.2f);
}

// A tile configuration C at run time, and THE tile-count formula: every plan of the three files (ring_plan, ig_plan,
// x_plan) and, through the plan, every kernel argument block, statistics size and grid counts its tiles here.
struct Tile { int mode, S, NB, TH, TW, TN, WP; };
template <class C>
constexpr Tile tile_of() { return {C::MODE, C::S, C::NB, C::TH, C::TW, C::TN, C::WP}; }
constexpr bool same_tile(const Tile& a, const Tile& b) {
  return a.mode == b.mode && a.S == b.S && a.NB == b.NB && a.TH == b.TH && a.TW == b.TW && a.TN == b.TN && a.WP == b.WP;
}
struct TileCounts { int tiles_w, tiles_hw, ntiles_n; long per_cls; };      // per_cls: workgroups per class (and per K split)
constexpr TileCounts tile_counts(const Tile& t, int B, int XH, int XW, int Cout) {
  const int tiles_w = cdiv(tile_extent(t.mode, t.S, XW), t.TW);
  const int tiles_hw = cdiv(tile_extent(t.mode, t.S, XH), t.TH) * tiles_w, ntiles_n = cdiv(Cout, t.TN);
  return {tiles_w, tiles_hw, ntiles_n, (long)ntiles_n * tiles_hw * cdiv(B, t.NB)};
}
// floats of a statistics buffer [slot][Cout][2]: one slot per (class, pixel tile, wavefront row)
constexpr size_t tile_stats_floats(const Tile& t, const TileCounts& n, int Cout) {
  return (size_t)(n.per_cls / n.ntiles_n) * t.WP * ((t.mode == CONV_FWD) ? 1 : t.S * t.S) * Cout * 2;
}
// the size measure of the tile heuristics (not a tile count): pixel tiles of `px` pixels, the images in whole 8 x 8 blocks
inline long px_tiles(int mode, int S, int B, int XH, int XW, int px) {
  return (long)cdiv(B * cdiv(tile_extent(mode, S, XH), 8) * cdiv(tile_extent(mode, S, XW), 8) * 64, px);
}
inline size_t slab_bytes(int mode, int S, int B, int XH, int XW, int Cout, int ksplit) {      // the partial outputs of a K split
  return ksplit <= 1 ? 0 : (size_t)ksplit * B * Cout * out_extent(mode, S, XH) * out_extent(mode, S, XW) * sizeof(float);
}

// Fills the shared fields for tile configuration C from the counts of the launch's plan (tile_counts of tile_of<C>()).
template <class C>
void fill_geom(ConvGeom& A, const float* x, const float* bias, float* y, int B, int Cin, int XH, int XW, int Cout, const TileCounts& n) {
  A.x = x; A.bias = bias; A.y = y;
  A.B = B; A.Cin = Cin; A.XH = XH; A.XW = XW; A.Cout = Cout;
  A.YH = out_extent(C::MODE, C::S, XH); A.YW = out_extent(C::MODE, C::S, XW);
  A.tiles_w = n.tiles_w; A.tiles_hw = n.tiles_hw; A.ntiles_n = n.ntiles_n; A.blocks_per_cls = (int)n.per_cls;
}
inline bool grid_ok(long grid) { return grid > 0 && grid <= 0x7fffffffL; }

// The split-arithmetic kernels: packed filter with its fp16 trailer, grid-level K split into partial output slabs.
struct SplitGeom : ConvGeom {
  const bf16x8* w;       // packed filter (vg_conv5x5_pack_bf16split)
  int CoutP;
  int cps;               // channel chunks per K split
  size_t ysplit;         // elements per partial output slab (ksplit > 1: y points at the slabs)
  // fp16 planes: in_amax[0] >= max |(activated) input| (device); w_unscale[0] = the inverse of the power of two the pack
  // kernel multiplied the filter by (the pack's trailer, common.hpp).  in_amax is NULL for bf16 planes.
  const float* in_amax;
  const float* w_unscale;
};
template <class C>
void fill_split(SplitGeom& A, const float* x, const bf16x8* w, const float* bias, float* y, int B, int Cin, int XH, int XW,
                int Cout, int ksplit, float* slabs, const float* in_amax, const TileCounts& n) {
  fill_geom<C>(A, x, bias, ksplit > 1 ? slabs : y, B, Cin, XH, XW, Cout, n);
  A.w = w;
  A.CoutP = packed_cout(Cout);
  A.cps = cdiv(Cin / 16, ksplit);
  A.ysplit = (size_t)B * Cout * A.YH * A.YW;
  A.in_amax = in_amax;
  A.w_unscale = (const float*)(w + vg_pack_trailer_units(Cin / 16 * 25, C::NP, A.CoutP));
}
// conv_ring.hip, called by the entry points of conv_bf16split.hip: stride-2 convolution (mode CONV_FWD) / transposed
// convolution (CONV_TR) on the 8-wave ring kernel.  planes may carry VG_PLANES_F16 (then fuse->in_amax is required);
// fuse may be NULL.
size_t vg_internal_ring_workspace_bytes(int mode, int B, int Cin, int H, int W, int Cout, int planes);
size_t vg_internal_ring_stats_floats(int mode, int B, int Cin, int H, int W, int Cout, int planes);
int vg_internal_ring_conv(int mode, const float* x, const void* packed, const float* bias, float* y, int B, int Cin, int H,
                          int W, int Cout, int planes, void* workspace, size_t workspace_bytes, const vg_conv_fusion* fuse,
                          hipStream_t st);

// ---- the weight-gradient kernels (conv_wgrad.hip, wgrad_bf16split.hip, conv_thin_wgrad.hip) -----------------------------
// dw[co][ci][kh][kw] = sum_{b,oh,ow} gy[b][co][oh][ow] * x[b][ci][S*oh+kh-2][S*ow+kw-2]: what every argument block starts
// with (filled by fill_wgrad from the plan's OH / OW) ...
struct WgradGeom {
  const float* x;
  int B, Cin, H, W, Cout, OH, OW;
};
template <class P>
void fill_wgrad(WgradGeom& A, const float* x, int B, int Cin, int H, int W, int Cout, const P& plan) {
  A.x = x;
  A.B = B; A.Cin = Cin; A.H = H; A.W = W; A.Cout = Cout; A.OH = plan.OH; A.OW = plan.OW;
}
// ... and, for the two implicit GEMMs D[co][ci * 25 + tap], the tiling: mtiles x ntiles output tiles, the reduction cut
// into `chunks` = (image or image group) x tiles_hw pixel tiles, tiles_w of them across a row.
struct WgradTiles : WgradGeom {
  int mtiles, ntiles, tiles_w, tiles_hw, chunks;
};
template <class P>
void fill_wgrad_tiles(WgradTiles& A, const float* x, int B, int Cin, int H, int W, int Cout, const P& plan) {
  fill_wgrad(A, x, B, Cin, H, W, Cout, plan);
  A.mtiles = plan.mtiles; A.ntiles = plan.ntiles; A.tiles_w = plan.tiles_w; A.tiles_hw = plan.tiles_hw; A.chunks = plan.chunks;
}
// chunk -> (image or image group, first output row, first output column) of its TH x TW pixel tile
template <int TH, int TW>
__device__ __forceinline__ void chunk_pos(const WgradTiles& A, int chunk, int& b, int& oh0, int& ow0) {
  b = chunk / A.tiles_hw;
  const int sp = chunk % A.tiles_hw;
  oh0 = (sp / A.tiles_w) * TH;
  ow0 = (sp % A.tiles_w) * TW;
}
// One 32 x 32 accumulator fragment into a partial slab ws[co][ci * 25 + tap]: rows co0 + acc_row, column n of the tile
// of CIT input channels from ci0 (lanes = consecutive n: coalesced); columns past the tile or Cin and rows past Cout stay.
template <int CIT>
__device__ __forceinline__ void store_slab_frag(float* ws, const f32x16& acc, int co0, int ci0, int n, int lane, int Cin, int Cout) {
  const bool nok = n < CIT * 25 && (ci0 + n / 25) < Cin;
#pragma unroll
  for (int r16 = 0; r16 < 16; ++r16) {
    const int co = co0 + acc_row(r16, lane);
    if (nok && co < Cout) ws[((size_t)co * Cin + ci0) * 25 + n] = acc[r16];
  }
}

// after the launch: fixed-order sum of the K split's slabs into y
inline int reduce_slabs(const SplitGeom& A, float* slabs, float* y, int ksplit, hipStream_t st) {
  if (ksplit <= 1) return 0;
  if (A.ysplit > 0x7fffffffUL) return VG_ERR_BAD_ARG;
  return vg_internal_wgrad_reduce(slabs, y, (int)A.ysplit, ksplit, st);
}
