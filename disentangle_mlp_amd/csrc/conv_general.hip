// General forward convolution in the fp16x3 arithmetic (vg_conv_general_fwd) for gfx950: the 94 convolutions of the FID
// Inception network (/root/reference/scoring/inception.py:16-310) -- 1x1, 3x3, 5x5, 1x7, 7x1, 1x3 and 3x1 filters,
// stride 1 or 2, any zero padding, 3 ... 2048 channels, 149 x 149 down to 8 x 8 pixels -- inference only:
//
//     y[b][co][oh][ow] = act( sum_{ci,kh,kw} x[b][ci][oh*sh + kh - ph][ow*sw + kw - pw] * w[co][ci][kh][kw] + bias[co] )
//
// as an implicit GEMM on v_mfma_f32_32x32x16_f16: rows = output channels (the filter, pre-packed), columns = output
// pixels of the whole batch, reduction index k = (kh * KW + kw) * Cin + ci, zero padded to a multiple of 32.  Same
// arithmetic as the training convolutions (common.hpp): each operand times an exact power of two
// from a device-side bound of its largest magnitude, split into fp16 hi + lo, the products lo*hi, hi*lo, hi*hi with fp32
// accumulation, the two scales undone on the accumulators.
//
//   * The filter never touches LDS: vg_conv_general_pack writes it once as [K step][plane][k-block][cout] x 8 fp16, so a
//     lane's A operand is one 16-byte global load (32 consecutive cout = 512 contiguous bytes), fetched one stage ahead.
//     Behind the planes the pack keeps a table k -> (ci, kh, kw) and, in a 16-byte trailer, the inverse of the filter's
//     scale.
//   * The activations are gathered from NCHW while they are staged: nothing im2col-shaped exists in HBM.  A thread
//     stages 8 reduction indices of ONE output pixel (consecutive lanes = consecutive pixels: for a fixed k they read
//     addresses a stride apart, the "row index contiguous" path of gemm_split.hip); its pixel coordinates are
//     computed once, a stage's (ci, kh, kw) come from the table through scalar loads (the k-block is uniform over a
//     wavefront).  Padding: the address is clamped to the image's first element and the value selected to zero.
//     One stage ahead in registers, split into planes, double-buffered in LDS, one barrier per stage.
//   * One workgroup = 4 wavefronts (2 x 2) on a TM x TN tile, TM, TN in {64, 128}, chosen on the host: the 17 x 17 and
//     8 x 8 layers take the smaller tiles to fill the CUs.  The reduction is never split: results are reproducible bit
//     for bit; the only atomic is the order-independent maximum of |y| for the next layer's bound.
#include "common.hpp"
#include "vaegan_hip.h"

namespace {

constexpr int CG_NT = 256, CG_KC = 32, CG_PAD = 2;
constexpr int CG_COUT_ALIGN = 128;       // the pack pads Cout to the largest tile
constexpr int CG_NO_TAP = 0x4000;        // kh of the table's entries beyond K: never inside an image (H <= CG_MAX_EXTENT)
constexpr int CG_MAX_EXTENT = 8192;      // H, W
constexpr int CG_MAX_FILTER = 15;        // KH, KW
constexpr int CG_CUS = 256;

struct CGArgs {
  const float* x;
  const f32x4* wp;          // [nsteps][2 planes][4 k-blocks][CoutP] units of 8 fp16
  const int2* tab;          // [nsteps * 32] (ci, kh << 16 | kw)
  const float* w_unscale;   // the pack's trailer
  const float* bias;
  float* y;
  const float* x_amax;
  unsigned* y_amax;
  int B, Cin, H, W, Cout, CoutP, OH, OW, sh, sw, ph, pw, nsteps, npix, tiles_m, relu;
  long y_img_stride;
};

__host__ __device__ constexpr size_t cg_plane_units(int nsteps, int CoutP) { return (size_t)nsteps * 8 * CoutP; }
__host__ __device__ constexpr size_t cg_table_units(int nsteps) { return (size_t)nsteps * CG_KC * sizeof(int2) / 16; }

template <int TM, int TN, bool PAD>
__global__ __launch_bounds__(CG_NT, 2) void conv_general_kernel(CGArgs G) {
  constexpr int FM = TM / 64, FN = TN / 64;            // 32 x 32 fragments per wavefront
  constexpr int KB = TN + CG_PAD, PL = 4 * KB, BUFU = 2 * PL;
  constexpr int NU = TN / 64;                          // staged units (8 reduction indices of one pixel) per thread
  __shared__ f32x4 lds[2 * BUFU];                      // [buffer][plane][k-block][pixel]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kb = lane >> 5, l32 = lane & 31;
  const int wm = wid & 1, wn = wid >> 1;
  // cout tiles of one pixel tile follow each other: they gather the same activations
  const int nt = blockIdx.x / G.tiles_m, mt = blockIdx.x - nt * G.tiles_m;
  const int m0 = mt * TM, n0 = nt * TN;
  const int ohw = G.OH * G.OW, HW = G.H * G.W;

  // ---- this thread's pixel: the divisions happen here, once
  const int pix = tid & (TN - 1);
  const int kblk0 = (wid * 64) / TN;                   // uniform over the wavefront; unit u: k-block kblk0 + u * (CG_NT / TN)
  const bool pix_ok = n0 + pix < G.npix;
  const int np = min(n0 + pix, G.npix - 1);
  const int pb = np / ohw, pr = np - pb * ohw, poh = pr / G.OW, pow_ = pr - poh * G.OW;
  const int ih0 = poh * G.sh - G.ph, iw0 = pow_ * G.sw - G.pw;
  const float* xb = G.x + (size_t)pb * ((size_t)G.Cin * HW);
  const int pixoff = ih0 * G.W + iw0;
  // pixels beyond the last one (clamped re-reads) are multiplied by zero: they only meet columns that are not stored
  const float xs = pix_ok ? f16_scale_of(*G.x_amax) : 0.f;

  float rg[NU][8];
  auto load_stage = [&](int st) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int2* t = G.tab + (st * CG_KC + (kblk0 + u * (CG_NT / TN)) * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int2 e = t[j];
        const int kw = e.y & 0xffff;
        if constexpr (PAD) {
          const int kh = e.y >> 16;
          const bool in = (unsigned)(ih0 + kh) < (unsigned)G.H && (unsigned)(iw0 + kw) < (unsigned)G.W;
          const int idx = in ? pixoff + (e.x * HW + kh * G.W + kw) : 0;      // clamped address, selected value
          const float v = xb[idx];
          rg[u][j] = in ? v : 0.f;
        } else {
          const int kh = (e.y >> 16) & 0xff;           // entries beyond K: tap (0, 0) of channel 0, times a zero filter
          rg[u][j] = xb[pixoff + (e.x * HW + kh * G.W + kw)];
        }
      }
    }
  };
  auto store_stage = [&](f32x4* base) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = rg[u][j] * xs;
      f32x4 pl[2];
      split_planes16<2, true>(v, pl);
      const int d = (kblk0 + u * (CG_NT / TN)) * KB + pix;
      base[d] = pl[0];
      base[d + PL] = pl[1];
    }
  };
  // filter fragments of a stage: [row fragment][K step of 16][plane]
  auto load_filter = [&](f32x4 (&af)[FM][2][2], int st) {
#pragma unroll
    for (int g = 0; g < FM; ++g)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int p = 0; p < 2; ++p)
          af[g][s2][p] = G.wp[((size_t)(st * 2 + p) * 4 + 2 * s2 + kb) * G.CoutP + m0 + wm * (TM / 2) + g * 32 + l32];
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int g = 0; g < FM; ++g)
#pragma unroll
    for (int h = 0; h < FN; ++h)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][h][r] = 0.f;

  f32x4 acur[FM][2][2], anxt[FM][2][2];
  load_stage(0);
  load_filter(acur, 0);
  store_stage(lds);
  __syncthreads();
  const int nst = G.nsteps;
  for (int st = 0; st < nst; ++st) {
    const f32x4* base = lds + (st & 1) * BUFU;
    // the stage past the end re-loads the last one (never consumed): no branch around the loads
    const int sn = min(st + 1, nst - 1);
    load_stage(sn);
    load_filter(anxt, sn);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      f32x4 bv[FN][2];
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int h = 0; h < FN; ++h) bv[h][p] = base[p * PL + (2 * s2 + kb) * KB + wn * (TN / 2) + h * 32 + l32];
#pragma unroll
      for (int sum = 1; sum >= 0; --sum)               // lo*hi, hi*lo, then hi*hi: small terms first
#pragma unroll
        for (int pa = sum; pa >= 0; --pa)
#pragma unroll
          for (int g = 0; g < FM; ++g)
#pragma unroll
            for (int h = 0; h < FN; ++h)
              acc[g][h] = mfma_split16<true>(__builtin_bit_cast(bf16x8, acur[g][s2][pa]),
                                             __builtin_bit_cast(bf16x8, bv[h][sum - pa]), acc[g][h]);
    }
    store_stage(lds + ((st & 1) ^ 1) * BUFU);          // stage st + 1 (after the last stage: a re-store nobody reads)
#pragma unroll
    for (int g = 0; g < FM; ++g)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int p = 0; p < 2; ++p) acur[g][s2][p] = anxt[g][s2][p];
    __syncthreads();
  }

  // ---- epilogue: undo the two scales (exact), bias, ReLU, store with the caller's image stride, bound of |y|
  const float ua = f16_unscale_of(*G.x_amax), ub = *G.w_unscale;
  unsigned am = 0;
#pragma unroll
  for (int h = 0; h < FN; ++h) {
    const int n = n0 + wn * (TN / 2) + h * 32 + l32;
    const bool n_ok = n < G.npix;
    const int nb = min(n, G.npix - 1) / ohw, nr = min(n, G.npix - 1) - nb * ohw;
    float* yp = G.y + (size_t)nb * G.y_img_stride + nr;
#pragma unroll
    for (int g = 0; g < FM; ++g)
#pragma unroll
      for (int r16 = 0; r16 < 16; ++r16) {
        const int co = m0 + wm * (TM / 2) + g * 32 + acc_row(r16, lane);
        if (n_ok && co < G.Cout) {
          float v = acc[g][h][r16] * ua * ub + (G.bias ? G.bias[co] : 0.f);
          if (G.relu) v = act_slope(v, 0.f);           // a NaN stays a NaN
          yp[(size_t)co * ohw] = v;
          am = max(am, abs_bits(v));
        }
      }
  }
  if (G.y_amax) block_amax_atomic<CG_NT>(am, G.y_amax);
}

// One thread = one (K step, k-block, cout) unit of both planes; the first nsteps * 32 threads also write the table.
__global__ __launch_bounds__(256) void conv_general_pack_kernel(const float* __restrict__ w, f32x4* __restrict__ p, int Cout,
                                                                int Cin, int KH, int KW, int CoutP, int nsteps,
                                                                const float* __restrict__ w_amax) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int taps = KH * KW, K = Cin * taps;
  if (e < (long)nsteps * 4 * CoutP) {
    const int co = (int)(e % CoutP), kblk = (int)(e / CoutP) & 3, step = (int)(e / (4L * CoutP));
    const float scale = f16_scale_of(*w_amax);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = step * CG_KC + kblk * 8 + j;
      const bool in = k < K && co < Cout;
      const int kc = min(k, K - 1), tap = kc / Cin, ci = kc - tap * Cin;
      const float t = w[((size_t)min(co, Cout - 1) * Cin + ci) * taps + tap];     // read, then select
      v[j] = in ? t * scale : 0.f;
    }
    f32x4 pl[2];
    split_planes16<2, true>(v, pl);
    p[((size_t)(step * 2 + 0) * 4 + kblk) * CoutP + co] = pl[0];
    p[((size_t)(step * 2 + 1) * 4 + kblk) * CoutP + co] = pl[1];
  }
  int2* tab = (int2*)(p + cg_plane_units(nsteps, CoutP));
  if (e < (long)nsteps * CG_KC) {
    const int k = (int)e;
    int2 t = {0, CG_NO_TAP << 16};
    if (k < K) {
      const int tap = k / Cin, kh = tap / KW;
      t = {k - tap * Cin, kh << 16 | (tap - kh * KW)};
    }
    tab[k] = t;
  }
  if (e == 0) {
    float* tr = (float*)(p + cg_plane_units(nsteps, CoutP) + cg_table_units(nsteps));
    tr[0] = f16_unscale_of(*w_amax);
    tr[1] = tr[2] = tr[3] = 0.f;
  }
}

bool cg_filter_ok(int Cout, int Cin, int KH, int KW) {
  if (Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0 || KH > CG_MAX_FILTER || KW > CG_MAX_FILTER) return false;
  const long K = (long)Cin * KH * KW;
  if (K > 0x7fffffffL - CG_KC) return false;
  const long CoutP = ((long)Cout + CG_COUT_ALIGN - 1) / CG_COUT_ALIGN * CG_COUT_ALIGN;
  // the pack kernel's thread index and every unit index stay inside 2^31 * 256
  return (K + CG_KC - 1) / CG_KC * 4 * CoutP <= 0x7fffffffL * 128;
}

// Tile of a launch: 128 output channels unless padding Cout to 128 wastes more than a fifth over padding it to 64; 128
// pixels unless that leaves fewer workgroups than CUs.
VG_KNOB(int, g_cg_tm, 0);   // tuning build only: forced tile (64 / 128; 0: the heuristic), vg_debug_set_conv_general_tile
VG_KNOB(int, g_cg_tn, 0);
void cg_tile(int Cout, int npix, int* tm, int* tn) {
  const int p64 = cdiv(Cout, 64) * 64, p128 = cdiv(Cout, 128) * 128;
  *tm = g_cg_tm ? g_cg_tm : (5 * p128 <= 6 * p64) ? 128 : 64;
  *tn = g_cg_tn ? g_cg_tn : ((long)cdiv(Cout, *tm) * cdiv(npix, 128) >= CG_CUS) ? 128 : 64;
}

}  // namespace

#ifdef VG_TUNING
extern "C" int vg_debug_set_conv_general_tile(int tm, int tn) {
  if ((tm != 0 && tm != 64 && tm != 128) || (tn != 0 && tn != 64 && tn != 128)) return VG_ERR_BAD_ARG;
  g_cg_tm = tm;
  g_cg_tn = tn;
  return 0;
}

extern "C" int vg_debug_conv_general_tile(int Cout, long npix, int pad, int* out) {
  if (!out || Cout <= 0 || npix <= 0 || npix > 0x7fffffffL - 128) return VG_ERR_BAD_ARG;
  cg_tile(Cout, (int)npix, &out[0], &out[1]);
  out[2] = pad ? 1 : 0;
  return 0;
}
#endif

extern "C" size_t vg_conv_general_packed_bytes(int Cout, int Cin, int KH, int KW) {
  if (!cg_filter_ok(Cout, Cin, KH, KW)) return 0;
  const int nsteps = cdiv(Cin * KH * KW, CG_KC), CoutP = cdiv(Cout, CG_COUT_ALIGN) * CG_COUT_ALIGN;
  return (cg_plane_units(nsteps, CoutP) + cg_table_units(nsteps) + 1) * 16;
}

extern "C" int vg_conv_general_pack(const float* w, void* packed, int Cout, int Cin, int KH, int KW, const float* w_amax,
                                    void* stream) {
  if (!w || !packed || !w_amax || ((uintptr_t)packed & 15) || !cg_filter_ok(Cout, Cin, KH, KW)) return VG_ERR_BAD_ARG;
  const int nsteps = cdiv(Cin * KH * KW, CG_KC), CoutP = cdiv(Cout, CG_COUT_ALIGN) * CG_COUT_ALIGN;
  const long threads = (long)nsteps * 4 * CoutP;       // >= nsteps * 32: the table's threads are among them
  hipLaunchKernelGGL(conv_general_pack_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                     (f32x4*)packed, Cout, Cin, KH, KW, CoutP, nsteps, w_amax);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_conv_general_fwd(const float* x, const void* packed, const float* bias, float* y, int B, int Cin, int H,
                                   int W, int Cout, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w,
                                   long y_image_stride, int relu, const float* x_amax, float* y_amax, void* stream) {
  if (!x || !packed || !y || !x_amax || ((uintptr_t)packed & 15)) return VG_ERR_BAD_ARG;
  if (B <= 0 || H <= 0 || W <= 0 || H > CG_MAX_EXTENT || W > CG_MAX_EXTENT || !cg_filter_ok(Cout, Cin, KH, KW))
    return VG_ERR_BAD_ARG;
  if ((stride_h != 1 && stride_h != 2) || (stride_w != 1 && stride_w != 2)) return VG_ERR_BAD_ARG;
  if (pad_h < 0 || pad_w < 0 || pad_h > CG_MAX_FILTER || pad_w > CG_MAX_FILTER) return VG_ERR_BAD_ARG;
  if (H + 2 * pad_h < KH || W + 2 * pad_w < KW) return VG_ERR_BAD_ARG;
  const int OH = (H + 2 * pad_h - KH) / stride_h + 1, OW = (W + 2 * pad_w - KW) / stride_w + 1;
  // 32-bit index ranges: an element inside one input image (with the filter's reach), an output pixel of the batch, an
  // element inside one output image; image offsets are 64-bit
  if ((long)Cin * H * W + (long)(CG_MAX_FILTER + 1) * (W + 1) > 0x7fffffffL) return VG_ERR_BAD_ARG;
  if ((long)B * OH * OW > 0x7fffffffL - 128 || (long)Cout * OH * OW > 0x7fffffffL) return VG_ERR_BAD_ARG;
  if (y_image_stride < (long)Cout * OH * OW) return VG_ERR_BAD_ARG;
  CGArgs G;
  G.nsteps = cdiv(Cin * KH * KW, CG_KC);
  G.CoutP = cdiv(Cout, CG_COUT_ALIGN) * CG_COUT_ALIGN;
  G.x = x;
  G.wp = (const f32x4*)packed;
  G.tab = (const int2*)(G.wp + cg_plane_units(G.nsteps, G.CoutP));
  G.w_unscale = (const float*)(G.wp + cg_plane_units(G.nsteps, G.CoutP) + cg_table_units(G.nsteps));
  G.bias = bias; G.y = y; G.x_amax = x_amax; G.y_amax = (unsigned*)y_amax;
  G.B = B; G.Cin = Cin; G.H = H; G.W = W; G.Cout = Cout; G.OH = OH; G.OW = OW;
  G.sh = stride_h; G.sw = stride_w; G.ph = pad_h; G.pw = pad_w;
  G.npix = B * OH * OW; G.relu = relu ? 1 : 0; G.y_img_stride = y_image_stride;
  int tm, tn;
  cg_tile(Cout, G.npix, &tm, &tn);
  G.tiles_m = cdiv(Cout, tm);
  const long grid = (long)G.tiles_m * cdiv(G.npix, tn);
  if (grid > 0x7fffffffL) return VG_ERR_BAD_ARG;
  const dim3 g((unsigned)grid), b(CG_NT);
  hipStream_t st = (hipStream_t)stream;
  const bool pad = pad_h || pad_w;
#define VG_CG_LAUNCH(TM_, TN_)                                                                      \
  do {                                                                                              \
    if (pad) hipLaunchKernelGGL((conv_general_kernel<TM_, TN_, true>), g, b, 0, st, G);             \
    else hipLaunchKernelGGL((conv_general_kernel<TM_, TN_, false>), g, b, 0, st, G);                \
  } while (0)
  if (tm == 128 && tn == 128) VG_CG_LAUNCH(128, 128);
  else if (tm == 128) VG_CG_LAUNCH(128, 64);
  else if (tn == 128) VG_CG_LAUNCH(64, 128);
  else VG_CG_LAUNCH(64, 64);
#undef VG_CG_LAUNCH
  VG_CHECK_LAUNCH();
  return 0;
}
