// Split-arithmetic 5x5 convolution / transposed convolution forward kernels (vg_conv5x5_fwd_bf16split,
// vg_convT5x5_fwd_bf16split) for gfx950: the product path of every split arithmetic (`planes`), the default
// fp16x3 included.  Every fp32 operand is split into 16-bit planes and each product is a sum of plane products on
// the 32x32x16 MFMA with fp32 accumulation:
//   fp16x3 (default)  fp16 hi + lo of the operand times an exact power of two (from a bound of the tensor's largest
//                     magnitude), 3 products hi*hi, hi*lo, lo*hi: fp32-equivalent, 4e-7 .. 6e-7 against fp64;
//   bf16x6            3 bf16 planes (8 + 8 + 8 mantissa bits), 6 products: fp32-equivalent at any dynamic range;
//   bf16x3            2 bf16 planes, 3 products: ~4.5e-6 relative (exact-fp32 path, conv_igemm.hip: 5e-7 .. 1e-6).
// 3 MFMAs per 16 k take 96 cycles where the exact-fp32 MFMA needs 8 x 64.  DESIGN.md sections 2 and 8 have the
// measurements.  The entry points hand the shapes conv_ring.hip takes to it (every stride-2 forward convolution,
// the wide transposed ones); the kernels of this file run the stride-1 forward convolution and the remaining
// transposed ones.
//
// Same computations as vg_conv5x5_fwd / vg_convT5x5_fwd (nn.Conv2d / nn.ConvTranspose2d forward of
// /root/reference/models/model.py:389-398, 450-456, 495-507 and each other's data gradients);
// requires Cin % 16 == 0.
//
// Structure (one workgroup = 4 wavefronts as WC x WP, FC x FP fragments of 32 x 32 per wavefront):
//   * K step = 16 input channels of one tap (MFMA k-block 0 / 1 = channels 0-7 / 8-15).
//   * The input patch of a 16-channel chunk lives in LDS channel-innermost, [plane hi/lo][k-block]
//     [image][row][column] x 8 bf16 (16 B): a lane's B operand is one ds_read_b128 at a per-lane
//     base + tap offset.  Row strides are chosen so that the rows a fragment spans fall on disjoint
//     banks.  The fp32 -> hi/lo split happens once per element, when the prefetched registers are
//     written to LDS.
//   * The filter never touches LDS: it comes pre-split and pre-packed (vg_conv5x5_pack_bf16split) as
//     [parity class][chunk][tap][plane][k-block][cout] x 8 bf16, so a lane's A operand is one 16-byte
//     global load (32 consecutive cout = 512 contiguous bytes), prefetched one tap ahead.
//   * The stride-2 transposed convolution runs as its 4 output-parity classes (3x3, 3x2, 2x3, 2x2
//     taps; conv_tile.hpp): one workgroup per (pixel tile, class).
//   * Tap algebra, tile placement, fragment decode, patch address and host geometry are
//     conv_tile.hpp's, shared with conv_igemm.hip and conv_ring.hip.
//   * Quad form (conv5x5_bf16split_quad_kernel; <= 32 output channels, 2 planes, grids of >= 256 workgroups): one
//     workgroup per 8 x 32 input tile computes all four classes.  The four per-class workgroups of a tile stage the
//     same patch; here it is loaded, scaled, split and written to LDS once, the 25 taps of a chunk run between one
//     pair of barriers on four accumulator sets (128 registers; 234 VGPRs in all, no scratch), a pixel fragment read
//     from LDS serves every class with a tap at that patch offset (9 reads per chunk, not 25), and a lane stores the
//     2 x 2 output block of its pixel as two 8-byte pairs: 32 lanes write 256 contiguous bytes where a class wrote
//     every other dword.  Every output element sums in the order of the per-class kernel (chunks, tap rows, tap
//     columns, plane products): the results are bit-identical.  113 -> 85 us per launch at B = 128, 128 -> 32
//     channels, 32 x 32 -> 64 x 64; WRITE_SIZE 129.5 -> 65.5 MB for the 65.5 MB (2^26 B) output
//     (profiles/r08_convT_quad.json).
#include "conv_tile.hpp"

namespace {

constexpr int XNT = 256;

// WC x WP wavefronts (WC * WP = 4), FC x FP fragments each: cout tile 32*WC*FC, pixel tile 32*WP*FP
// NP_: operand planes -- 2: hi/lo split, 3 products ("bf16x3", ~4.5e-6); 3: exact hi/mid/lo split of the fp32
// mantissa (8 + 8 + 8 bits), 6 products, every dropped term below 2^-24 ("bf16x6", fp32-equivalent)
template <int MODE_, int S_, int NB_, int TH_, int TW_, int WC_, int FC_, int FP_, int NP_, bool F16_ = false>
struct XCfg {
  static constexpr int MODE = MODE_, S = S_, NB = NB_, TH = TH_, TW = TW_, WC = WC_, WP = 4 / WC_, FC = FC_, FP = FP_;
  static constexpr int NP = NP_;
  static constexpr bool F16 = F16_;       // fp16 planes (NP = 2): common.hpp, "split arithmetics"
  static_assert(!F16_ || NP_ == 2, "fp16 planes: hi + lo");
  static constexpr int TN = 32 * WC * FC, TM = NB * TH * TW;
  using Taps = TileTaps<MODE, S, TH, TW>;
  static constexpr int NTMAX = Taps::NTMAX, PH = Taps::PH, PW = Taps::PW, NCLS = Taps::NCLS;
  static_assert(MODE == CONV_TR || S == 1, "the stride-2 forward convolution runs in conv_ring.hip");
  static constexpr int ROWU = row_units(TW, PW);                  // units per patch row
  static constexpr int IMGU = NB * PH * ROWU;                     // units per (plane, k-block) image
  static constexpr int NUNIT = 2 * NB * PH * PW;                  // staged units per chunk
  static constexpr int NQ = cdiv(NUNIT, XNT);
  static_assert(TM == 32 * WP * FP, "pixel tile");
  static_assert(WC == 1 || WC == 2 || WC == 4, "wavefront grid");
};

using XArgs = SplitGeom;      // the K split (cps, ysplit) is forward only: deep-K, small-grid layers

// Quad form of the stride-2 transposed convolution: one workgroup runs the 25 taps of a chunk for all four parity
// classes.  Step i is tap (a, b) of class cls = 2 R + SS; the steps walk the 3 x 3 patch offsets (2 - a, 2 - b) row by
// row, and at each offset the classes that have a tap there (a < 3 - R, b < 3 - SS) in class order: 4 + 4 + 2, twice,
// then 2 + 2 + 1.  A class meets its own taps rows first, then columns -- the order of the per-class kernel.
struct XQStep { int a, b, cls; };
constexpr XQStep x_quad_step(int i) {
  int n = 0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b)
      for (int cls = 0; cls < 4; ++cls)
        if (a < 3 - cls / 2 && b < 3 - cls % 2) {
          if (n == i) return {a, b, cls};
          ++n;
        }
  return {0, 0, 0};     // i = 25: the next chunk's first step
}
static_assert(x_quad_step(24).a == 2 && x_quad_step(24).b == 2 && x_quad_step(24).cls == 0 && x_quad_step(9).cls == 2 && x_quad_step(17).cls == 3, "25 steps");

template <int I, int N, class F>
__device__ __forceinline__ void x_static_for(F&& f) {      // f(IntC<I>) ... f(IntC<N - 1>): the index is a constant in f
  if constexpr (I < N) {
    f(IntC<I>{});
    x_static_for<I + 1, N>(f);
  }
}

// QUAD (with R = SS = 0): all four classes of the tile, see x_quad_step
template <class C, int R, int SS, bool QUAD = false>
__device__ __forceinline__ void bf16split_body(const XArgs& A, f32x4* lds, int bid, int split) {
  constexpr int MODE = C::MODE, S = C::S, NB = C::NB, TH = C::TH, TW = C::TW, PH = C::PH, PW = C::PW;
  constexpr int ROWU = C::ROWU, IMGU = C::IMGU, NQ = C::NQ, FC = C::FC, FP = C::FP, NP = C::NP;
  constexpr int NTMAX = C::NTMAX;
  constexpr bool F16 = C::F16;
  constexpr int NTH = C::Taps::nth(R), NTW = C::Taps::nth(SS);     // taps along h / w in this class
  constexpr int NTAP = NTH * NTW;
  constexpr int PSTEP = C::Taps::PSTEP;
  constexpr int NACC = QUAD ? 4 : FC;                              // accumulator sets: one per class / per cout fragment
  static_assert(!QUAD || (MODE == CONV_TR && S == 2 && C::WC == 1 && FC == 1 && NP == 2 && R == 0 && SS == 0), "quad form");

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kb = lane >> 5, l32 = lane & 31;
  const int wc = wid % C::WC, wp = wid / C::WC;
  int nt, pt;
  place_tile<false>(bid, A.ntiles_n, A.blocks_per_cls, nt, pt);
  const TileOrigin org = tile_origin<C>(pt, nt, A);
  const int b0 = org.b0, n0 = org.n0;
  const int Cin = A.Cin, Cout = A.Cout, HW = A.XH * A.XW;
  const float* xb = A.x + (size_t)b0 * Cin * HW;

  // ---- staging map: unit e = (k-block, image, row, column); addresses clamped, validity masked
  int pofs[NQ], pdst[NQ];
  unsigned pvalid = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = tid + q * XNT;
    const int col = e % PW;
    int t = e / PW;
    const int r = t % PH;
    t /= PH;
    const int nb = t % NB, kbs = min(t / NB, 1);
    const PatchElem pe = patch_elem(A, org, nb, r, col, e < C::NUNIT);
    pofs[q] = pe.ofs + kbs * 8 * HW;
    pdst[q] = (e < C::NUNIT) ? kbs * IMGU + (nb * PH + r) * ROWU + col : -1;
    pvalid |= pe.ok ? (1u << q) : 0u;
  }
  static_assert(NQ <= 32, "validity mask");

  float x_scale = 1.f, x_unscale = 1.f;     // fp16 planes: exact power of two from the caller's bound on max |x|
  if constexpr (F16) {
    const float amax = *A.in_amax;
    x_scale = f16_scale_of(amax);
    x_unscale = f16_unscale_of(amax);
  }
  float preg[NQ][8];
  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int j = 0; j < 8; ++j) preg[q][j] = xb[pofs[q] + (c0 + j) * HW];
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const bool ok = (pvalid >> q) & 1u;
      f32x4 pl[NP];
      float vv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = ok ? preg[q][j] : 0.f;
        vv[j] = F16 ? v * x_scale : v;
      }
      split_planes16<NP, F16>(vv, pl);
      if (pdst[q] >= 0) {
#pragma unroll
        for (int p = 0; p < NP; ++p) lds[pdst[q] + p * 2 * IMGU] = pl[p];
      }
    }
  };

  // ---- per-lane operand bases
  int base_b[FP];
#pragma unroll
  for (int f = 0; f < FP; ++f) {
    const FragPixel fp = frag_pixel<C>(wp, f, l32);
    base_b[f] = kb * IMGU + (fp.nb * PH + PSTEP * fp.row) * ROWU + PSTEP * fp.col;
  }
  const int CoutP = A.CoutP;
  const size_t wstep = (size_t)2 * NP * CoutP;    // units per (chunk, tap) step
  const int nchunks = Cin / 16;
  const bf16x8* wa[FC];                      // this class' first step, this lane's cout and k-block
#pragma unroll
  for (int g = 0; g < FC; ++g)
    wa[g] = A.w + (size_t)class_taps_before(S, R, SS) * nchunks * wstep + (size_t)kb * CoutP + n0 + (wc * FC + g) * 32 + l32;

  f32x16 acc[NACC][FP];
#pragma unroll
  for (int g = 0; g < NACC; ++g)
#pragma unroll
    for (int f = 0; f < FP; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][f][r] = 0.f;

  const int c_begin = split * A.cps, c_end = min(c_begin + A.cps, nchunks);   // this workgroup's channel chunks
  load_chunk(c_begin * 16);
  store_chunk();
  bf16x8 av[2][FC][NP];     // [buffer][fragment][plane]
#pragma unroll
  for (int g = 0; g < FC; ++g)
#pragma unroll
    for (int p = 0; p < NP; ++p) av[0][g][p] = wa[g][(size_t)c_begin * NTAP * wstep + (size_t)p * 2 * CoutP];
  __syncthreads();

  for (int ch = c_begin; ch < c_end; ++ch) {
    const bool more = (ch + 1) < c_end;
    if (more) load_chunk((ch + 1) * 16);
    if constexpr (QUAD) {
      // The 25 steps unrolled, pinned like the per-class pipeline below: a step issues the next step's filter fragments
      // (the step after the last one is the next chunk's first; after the last chunk it reads class 1's first step,
      // unused), the first step at a patch offset also the next offset's pixel fragments, which every class with a tap
      // there shares: 9 fragment reads per chunk where the four per-class workgroups made 25.
      bf16x8 bv[2][FP][NP];
      auto read_b = [&](int buf, int o) {
        const int off = (NTMAX - 1 - o / 3) * ROWU + (NTMAX - 1 - o % 3);
#pragma unroll
        for (int f = 0; f < FP; ++f)
#pragma unroll
          for (int p = 0; p < NP; ++p) bv[buf][f][p] = __builtin_bit_cast(bf16x8, lds[base_b[f] + off + p * 2 * IMGU]);
      };
      read_b(0, 0);
      x_static_for<0, 25>([&](auto idx) {
        constexpr int i = decltype(idx)::value;
        constexpr XQStep s = x_quad_step(i), n = x_quad_step(i + 1), before = x_quad_step(i > 0 ? i - 1 : 0);
        constexpr int cur = i & 1, nxt = cur ^ 1, o = s.a * 3 + s.b;
        constexpr bool first = i == 0 || before.a != s.a || before.b != s.b;
        constexpr int nntw = 3 - n.cls % 2, nntap = (3 - n.cls / 2) * nntw;
        const size_t nstep = (size_t)class_taps_before(S, n.cls / 2, n.cls % 2) * nchunks + (size_t)(ch + (i == 24 ? 1 : 0)) * nntap +
                             n.a * nntw + n.b;
#pragma unroll
        for (int p = 0; p < NP; ++p) av[nxt][0][p] = wa[0][nstep * wstep + (size_t)p * 2 * CoutP];
        if constexpr (first && o + 1 < 9) read_b((o + 1) & 1, o + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int sum = NP - 1; sum >= 0; --sum)
#pragma unroll
          for (int pa = sum; pa >= 0; --pa)
#pragma unroll
            for (int f = 0; f < FP; ++f) acc[s.cls][f] = mfma_split16<F16>(av[cur][0][pa], bv[o & 1][f][sum - pa], acc[s.cls][f]);
        __builtin_amdgcn_sched_barrier(0);
      });
#pragma unroll
      for (int p = 0; p < NP; ++p) av[0][0][p] = av[1][0][p];      // 25 steps: the prefetched one is back in buffer 0
    } else {
      // one filter row (NTW taps) per trip of a rolled loop: keeps the filter prefetch one tap deep
      // (fully unrolled, hipcc hoists every tap's loads and spills).  When NTW is odd the prefetched
      // step is moved back into buffer 0 at the end of the row, so `cur` stays compile-time.
#pragma unroll 1
      for (int ta = 0; ta < NTH; ++ta) {
        const bf16x8* wrow[FC];
#pragma unroll
        for (int g = 0; g < FC; ++g) wrow[g] = wa[g] + ((size_t)ch * NTAP + ta * NTW) * wstep;
        const int rowoff = (MODE == CONV_FWD) ? ta * ROWU : (NTMAX - 1 - ta) * ROWU;
        // Pinned software pipeline (hipcc otherwise sinks the prefetch loads next to their first use, one
        // vmcnt wait per MFMA pair): at the top of a tap issue the NEXT tap's filter fragments (global) and
        // pixel fragments (LDS, within the row), then run this tap's MFMAs on registers loaded a tap ago.
        constexpr bool BPF = (NP == 2);      // pixel fragments one tap ahead too (3 planes: no registers left for it)
        constexpr bool PIN = (NP == 2) || C::WC == 4;   // 3 planes, 2 x 2 fragments: pinning makes the allocator spill
        bf16x8 bv[BPF ? 2 : 1][FP][NP];
        auto read_b = [&](int buf, int t) {
          const int imm = (MODE == CONV_TR) ? (NTMAX - 1 - t) : t;
#pragma unroll
          for (int f = 0; f < FP; ++f)
#pragma unroll
            for (int p = 0; p < NP; ++p) bv[buf][f][p] = __builtin_bit_cast(bf16x8, lds[base_b[f] + rowoff + imm + p * 2 * IMGU]);
        };
        if (BPF) read_b(0, 0);
#pragma unroll
        for (int tb = 0; tb < NTW; ++tb) {
          const int cur = tb & 1, nxt = cur ^ 1;
          // next tap's filter fragments (the pack has one spare step after the last one)
#pragma unroll
          for (int g = 0; g < FC; ++g)
#pragma unroll
            for (int p = 0; p < NP; ++p) av[nxt][g][p] = wrow[g][(size_t)(tb + 1) * wstep + (size_t)p * 2 * CoutP];
          if (BPF) {
            if (tb + 1 < NTW) read_b(nxt, tb + 1);
          } else {
            read_b(0, tb);
          }
          if (PIN) __builtin_amdgcn_sched_barrier(0);
          // products with plane index sum <= NP - 1, smallest terms first; product-major so that independent
          // accumulators sit between dependent MFMAs
#pragma unroll
          for (int sum = NP - 1; sum >= 0; --sum)
#pragma unroll
            for (int pa = sum; pa >= 0; --pa)
#pragma unroll
              for (int g = 0; g < FC; ++g)
#pragma unroll
                for (int f = 0; f < FP; ++f) acc[g][f] = mfma_split16<F16>(av[cur][g][pa], bv[BPF ? cur : 0][f][sum - pa], acc[g][f]);
          if (PIN) __builtin_amdgcn_sched_barrier(0);
        }
        if (NTW & 1) {
#pragma unroll
          for (int g = 0; g < FC; ++g)
#pragma unroll
            for (int p = 0; p < NP; ++p) av[0][g][p] = av[1][g][p];
        }
      }
    }
    __syncthreads();
    if (more) {
      store_chunk();
      __syncthreads();
    }
  }

  if constexpr (F16) {   // undo the two operands' power-of-two scales (two exact multiplications)
    const float w_unscale = *A.w_unscale;
#pragma unroll
    for (int g = 0; g < NACC; ++g)
#pragma unroll
      for (int f = 0; f < FP; ++f)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[g][f][r] = acc[g][f][r] * x_unscale * w_unscale;
  }
  // ---- epilogue: + bias, NCHW store
  if constexpr (QUAD) {
    // A lane holds the 2 x 2 output block of its pixel for 16 channels: the two columns of a row go out as one 8-byte
    // store (32 lanes = 256 contiguous bytes per row and channel) where the row has both and the address allows it.
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const int YH = A.YH, YW = A.YW;
    const bool pair8 = ((uintptr_t)A.y & 7) == 0 && (YW & 1) == 0;
    float bq[16];
#pragma unroll
    for (int r16 = 0; r16 < 16; ++r16) bq[r16] = A.bias ? A.bias[min(n0 + acc_row(r16, lane), Cout - 1)] : 0.f;
#pragma unroll
    for (int f = 0; f < FP; ++f) {
      const FragPixel fp = frag_pixel<C>(wp, f, l32);
      const int th = org.th0 + fp.row, tw = org.tw0 + fp.col, b = b0 + fp.nb, ow = S * tw;
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int oh = S * th + rr;
        const bool pok = b < A.B && oh < YH;
        float* yb = A.y + ((size_t)b * Cout * YH + oh) * YW + ow;
#pragma unroll
        for (int r16 = 0; r16 < 16; ++r16) {
          const int co = n0 + acc_row(r16, lane);
          const float v0 = acc[2 * rr][f][r16] + bq[r16], v1 = acc[2 * rr + 1][f][r16] + bq[r16];
          float* yp = yb + (size_t)co * YH * YW;
          if (pok && co < Cout) {
            if (pair8 && ow + 1 < YW) {
              *(f32x2*)yp = f32x2{v0, v1};
            } else {
              if (ow < YW) yp[0] = v0;
              if (ow + 1 < YW) yp[1] = v1;
            }
          }
        }
      }
    }
  } else {
    const int YH = A.YH, YW = A.YW;
#pragma unroll
  for (int f = 0; f < FP; ++f) {
    const int m = (wp * FP + f) * 32 + l32;
    const int nb = m / (TH * TW), r = m % (TH * TW);
    const int th = org.th0 + r / TW, tw = org.tw0 + r % TW, b = b0 + nb;
    const int oh = (MODE == CONV_FWD) ? th : S * th + R;
    const int ow = (MODE == CONV_FWD) ? tw : S * tw + SS;
    const bool pok = b < A.B && oh < YH && ow < YW;
    float* yb = A.y + (size_t)split * A.ysplit + ((size_t)b * Cout * YH + oh) * YW + ow;
#pragma unroll
    for (int g = 0; g < FC; ++g) {
      float bv[16];
#pragma unroll
      for (int r16 = 0; r16 < 16; ++r16) {
        const int co = min(n0 + (wc * FC + g) * 32 + acc_row(r16, lane), Cout - 1);
        bv[r16] = (A.bias && split == 0) ? A.bias[co] : 0.f;     // partial slabs: the bias goes in once
      }
#pragma unroll
      for (int r16 = 0; r16 < 16; ++r16) {
        const int co = n0 + (wc * FC + g) * 32 + acc_row(r16, lane);
        if (pok && co < Cout) yb[(size_t)co * YH * YW] = acc[g][f][r16] + bv[r16];
      }
    }
  }
  }
}

template <class C>
__global__ __launch_bounds__(XNT, 2) void conv5x5_bf16split_kernel(XArgs A) {
  __shared__ f32x4 lds[2 * C::NP * C::IMGU];     // [plane][k-block][image][row][(parity)][column]
  int bid = blockIdx.x;
  if constexpr (C::NCLS == 1) {
    const int split = bid / A.blocks_per_cls;
    bf16split_body<C, 0, 0>(A, lds, bid - split * A.blocks_per_cls, split);
  } else {
    const int cls = bid / A.blocks_per_cls;   // class 0 (3x3 taps) first: longest blocks start earliest
    bid -= cls * A.blocks_per_cls;
    for_class(cls, [&](auto R, auto SS) __attribute__((always_inline)) {
      bf16split_body<C, decltype(R)::value, decltype(SS)::value>(A, lds, bid, 0);
    });
  }
}

template <class C>
__global__ __launch_bounds__(XNT, 2) void conv5x5_bf16split_quad_kernel(XArgs A) {
  __shared__ f32x4 lds[2 * C::NP * C::IMGU];     // the per-class kernel's patch, staged once for the four classes
  bf16split_body<C, 0, 0, true>(A, lds, blockIdx.x, 0);
}

// What a launch does, decided once (x_plan).  ksplit 1: none (forward only); slab_bytes: of the ksplit partial outputs.
struct XPlan { int var, ksplit; Tile tile; TileCounts n; long grid; size_t slab_bytes; };

// Launches what the plan says; decides nothing.
template <class C, bool QUAD>
int launch_x(const XPlan& p, const float* x, const bf16x8* w, const float* bias, float* y, int B, int Cin, int XH, int XW,
             int Cout, float* slabs, const float* in_amax, hipStream_t st) {
  if (!same_tile(p.tile, tile_of<C>()) || !grid_ok(p.grid)) return VG_ERR_BAD_ARG;
  XArgs A;
  fill_split<C>(A, x, w, bias, y, B, Cin, XH, XW, Cout, p.ksplit, slabs, in_amax, p.n);
  if constexpr (QUAD)
    hipLaunchKernelGGL(conv5x5_bf16split_quad_kernel<C>, dim3((unsigned)p.grid), dim3(XNT), 0, st, A);
  else
    hipLaunchKernelGGL(conv5x5_bf16split_kernel<C>, dim3((unsigned)p.grid), dim3(XNT), 0, st, A);
  VG_CHECK_LAUNCH();
  return reduce_slabs(A, slabs, y, p.ksplit, st);
}

// diagnostics: 0 = 128 cout x 128 px, 1 = 64 x 128, 2 = 64 x 64, 3 = 32 cout x 128 px, 4 = 32 x 256 (transposed, one workgroup
// per parity class), 5 = 128 x 128 along cout, 6 = 32 x 256 quad (transposed, stride 2, 2 planes: all four classes per workgroup)
VG_KNOB(int, g_x_tile_override, -1);

// the quad form has one geometry: the 8 x 32 tile, whatever the image (narrower ones are masked)
constexpr bool x_has_quad(int mode, int S, int NP) { return mode == CONV_TR && S == 2 && NP == 2; }
template <int MODE, int S, int NP, bool F16>
using XQuadCfg = XCfg<MODE, S, 1, 8, 32, 1, 1, 2, NP, F16>;

// (variant, width of the tile space) -> f(XCfg{}, IntC<quad form>{}).  The pixel tile of TM = 64 / 128 / 256 pixels by the
// width -- rows of 32 or 16 pixels of one image (TM / 32, TM / 16 of them), or 8 x 8 pixels of TM / 64 images -- of the
// variant's WC, FC, FP
template <int MODE, int S, int WC, int FC, int FP, int NP, bool F16, class F>
int x_with_geom(int tsw, F&& f) {
  auto width = [&](auto tw) {
    constexpr int TW = decltype(tw)::value, TM = 32 * (4 / WC) * FP, NB = (TW == 8) ? TM / 64 : 1;
    return f(XCfg<MODE, S, NB, TM / (NB * TW), TW, WC, FC, FP, NP, F16>{}, IntC<0>{});
  };
  return tsw >= 32 ? width(IntC<32>{}) : (tsw >= 16 ? width(IntC<16>{}) : width(IntC<8>{}));
}
template <int MODE, int S, int NP, bool F16, class F>
int x_for_cfg(int var, int tsw, F&& f) {
  if (var == 0) return x_with_geom<MODE, S, 2, 2, 2, NP, F16>(tsw, f);
  if (var == 1) return x_with_geom<MODE, S, 2, 1, 2, NP, F16>(tsw, f);
  if (var == 3) return x_with_geom<MODE, S, 1, 1, 1, NP, F16>(tsw, f);
  if (var == 5) return x_with_geom<MODE, S, 4, 1, 4, NP, F16>(tsw, f);   // 4 wavefronts along cout
  if constexpr (MODE == CONV_TR) {
    if (var == 4) return x_with_geom<MODE, S, 1, 1, 2, NP, F16>(tsw, f);
  }
  if constexpr (x_has_quad(MODE, S, NP)) {
    if (var == 6) return f(XQuadCfg<MODE, S, NP, F16>{}, IntC<1>{});
  }
  return x_with_geom<MODE, S, 2, 1, 1, NP, F16>(tsw, f);
}

// Forward, deep K on a small grid (the 8 x 8-pixel layers): the 128 x 128 tile with the channel chunks split
// over k workgroups, partial outputs summed in a fixed order.  1 = no split.  wgs: workgroups of that tile.
int fwd_ksplit(long wgs, int nchunks, int Cout) {
  if (g_x_tile_override >= 0 || Cout <= 64 || wgs >= 512 || nchunks < 8) return 1;
  int k = 2;     // every split must own at least one chunk: (k - 1) * ceil(nchunks / k) < nchunks
  while (wgs * k < 512 && k < 8 && nchunks / (2 * k) >= 2 && (2 * k - 1) * cdiv(nchunks, 2 * k) < nchunks) k *= 2;
  return k;
}

// Biggest tile that still gives every CU two workgroups (256 CUs): 128 cout x 128 px, else 64 cout x
// 128 px, else 64 x 64; 32 cout x 128 px (4 wavefronts along the pixels) for thin outputs.
template <int MODE, int S, int NP, bool F16>
XPlan x_plan(int B, int Cin, int XH, int XW, int Cout) {
  const int tsw = tile_extent(MODE, S, XW), ncls = (MODE == CONV_TR) ? S * S : 1;
  const long px128 = px_tiles(MODE, S, B, XH, XW, 128) * ncls;
  XPlan p;
  p.ksplit = (MODE == CONV_FWD) ? fwd_ksplit(px128 * cdiv(Cout, 128), Cin / 16, Cout) : 1;
  int var = 2;
  if (Cout <= 32) var = (MODE == CONV_TR && px128 >= 1024) ? 4 : 3;      // transposed, large grid: 256 pixels per workgroup
  else if (MODE == CONV_FWD && Cout > 64 && px128 * cdiv(Cout, 128) >= 512) var = 0;   // transposed: 64 x 128 measured faster
  else if (px128 * cdiv(Cout, 64) >= 512) var = 1;
  // 3 planes: the 128 x 128 tile with the four wavefronts along cout (each loads only its own filter fragment)
  // measured 0-15 % faster than the 2 x 2 arrangement, never slower
  if (NP == 3 && (var == 0 || var == 1) && Cout >= 128 && px128 * cdiv(Cout, 128) >= 256) var = 5;
  // stride 2, 2 planes, images at least one 8 x 32 tile wide: the quad form of that tile (bit-identical to variant 4),
  // once its grid -- a quarter of the per-class one -- has a workgroup for every CU.  Measured (profiles/r08_convT_quad.json):
  // 0.56 - 0.89 of the per-class time at 256 and 512 workgroups, 1.0 - 1.5 of it at 128.
  constexpr bool HAS_QUAD = x_has_quad(MODE, S, NP);
  if constexpr (HAS_QUAD)
    if (var == 4 && tsw >= 32 && tile_counts(tile_of<XQuadCfg<MODE, S, NP, F16>>(), B, XH, XW, Cout).per_cls >= 256) var = 6;
  if (p.ksplit > 1) var = 0;             // split-K is sized for the 128 x 128 tile
  else if (g_x_tile_override >= 0 && g_x_tile_override <= 6 && !(g_x_tile_override == 4 && MODE == CONV_FWD) &&
           !(g_x_tile_override == 6 && !HAS_QUAD))
    var = g_x_tile_override;
  p.var = var;
  x_for_cfg<MODE, S, NP, F16>(var, tsw, [&](auto c, auto) { p.tile = tile_of<decltype(c)>(); return 0; });
  p.n = tile_counts(p.tile, B, XH, XW, Cout);
  p.grid = p.n.per_cls * (var == 6 ? 1 : ncls) * p.ksplit;
  p.slab_bytes = slab_bytes(MODE, S, B, XH, XW, Cout, p.ksplit);
  return p;
}

template <int MODE, int S, int NP, bool F16>
int dispatch_x(const float* x, const bf16x8* w, const float* bias, float* y, int B, int Cin, int XH, int XW, int Cout,
               void* workspace, size_t workspace_bytes, const float* in_amax, hipStream_t st) {
  const XPlan p = x_plan<MODE, S, NP, F16>(B, Cin, XH, XW, Cout);
  if (p.ksplit > 1 && (!workspace || workspace_bytes < p.slab_bytes)) return VG_ERR_WORKSPACE;
  if (F16 && !in_amax) return VG_ERR_BAD_ARG;
  return x_for_cfg<MODE, S, NP, F16>(p.var, tile_extent(MODE, S, XW), [&](auto c, auto quad) {
    return launch_x<decltype(c), decltype(quad)::value != 0>(p, x, w, bias, y, B, Cin, XH, XW, Cout, (float*)workspace, in_amax, st);
  });
}

// packed[class][chunk][step][plane][k-block][CoutP] x 8 bf16 (+ VG_PACK_SPARE zero steps at the end: the ring
// kernel's DMA runs up to VG_RING_SLOTS steps ahead of the MFMAs; + the fp16 trailer, common.hpp).
//   transposed = 0, S = 1: w is [Cout][Cin][5][5], one class of 25 taps (kh*5 + kw); a step is one tap, its two
//                   k-blocks are channels 0-7 / 8-15 of the chunk;
//   transposed = 0, S = 2 (conv_ring.hip): a step is 8 channels x 2 consecutive taps -- steps 0-11 taps (2s, 2s+1)
//                   of channels 0-7, step 12 tap 24 of channels 0-7 | 8-15, steps 13-24 taps of channels 8-15;
//   transposed = 1: w is [Cin][Cout][5][5], S*S parity classes, tap (a, b) of class (R, SS) is
//                   (kh, kw) = (R + S*a, SS + S*b).
constexpr int PK_CO = 8, PK_PITCH = 401;         // channels per workgroup (512 workgroups for a 256 x 256 filter: with 32
                                                 // channels and 128 workgroups it ran 21 us); floats per channel in LDS (400 + 1)
// One workgroup = PK_CO output channels x one 16-channel chunk: the PK_CO x 16 x 25 filter values are read with contiguous
// loads into LDS (400 contiguous floats per channel, or 800 per input channel for the transposed layout) and every
// (channel, step, k-block) unit is built from there.  (The first version read each value with its own 4-byte load, a
// lane's 16 values 100 bytes apart and the lanes 12.8 KB apart: 12.7 us for the 6.5 MB filter, 0.29 ms per iteration.)
// planes & VG_PLANES_F16_FLAG: fp16 planes -- the filter is multiplied by f16_scale_of(w_amax[0]) first and the inverse of
// that power of two is left in the pack's trailer (one float behind the spare steps) for the convolution's epilogue.
__device__ __forceinline__ void pack_bf16split_body(float* T, const float* __restrict__ w, bf16x8* __restrict__ p,
                                                    int Cout, int Cin, int CoutP, int nsteps, int transposed, int S,
                                                    int planes, const float* __restrict__ w_amax, int bx, int by) {
  const int tid = threadIdx.x;
  const bool f16 = (planes & VG_PLANES_F16_FLAG) != 0;
  planes &= 0xff;
  const float wscale = f16 ? f16_scale_of(*w_amax) : 1.f;
  // the trailer at vg_pack_trailer_units(nsteps, planes, CoutP), written out (a call compiles to another instruction order)
  if (f16 && bx == 0 && by == 0 && tid == 0)
    *(float*)(p + (size_t)(nsteps + VG_PACK_SPARE) * planes * 2 * CoutP) = f16_unscale_of(*w_amax);
  const int co0 = bx * PK_CO, c16 = by, nchunks = Cin / 16;
  if (!transposed) {
    for (int e0 = tid; e0 < PK_CO * 400; e0 += 4 * 256) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = min(e0 + k * 256, PK_CO * 400 - 1), col = e / 400, r = e - col * 400;
        const float t = w[((size_t)min(co0 + col, Cout - 1) * Cin + c16 * 16) * 25 + r];      // read, then select
        v[k] = (co0 + col < Cout) ? t : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k * 256, col = e / 400, r = e - col * 400;
        if (e < PK_CO * 400) T[col * PK_PITCH + r] = v[k];
      }
    }
  } else {
    for (int e0 = tid; e0 < 16 * PK_CO * 25; e0 += 4 * 256) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = min(e0 + k * 256, 16 * PK_CO * 25 - 1), ci = e / (PK_CO * 25), r = e - ci * (PK_CO * 25);
        const int col = r / 25;
        const float t = w[((size_t)(c16 * 16 + ci) * Cout + min(co0 + col, Cout - 1)) * 25 + (r - col * 25)];
        v[k] = (co0 + col < Cout) ? t : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = e0 + k * 256, ci = e / (PK_CO * 25), r = e - ci * (PK_CO * 25), col = r / 25;
        if (e < 16 * PK_CO * 25) T[col * PK_PITCH + ci * 25 + (r - col * 25)] = v[k];
      }
    }
  }
  __syncthreads();
  // units: (local step q, k-block kb, channel): lanes = consecutive channels (contiguous 16-byte stores)
  const int col = tid & (PK_CO - 1);
  const bool cok = co0 + col < CoutP;
  for (int it = tid / PK_CO; it < 50; it += 256 / PK_CO) {
    const int q = it >> 1, kb = it & 1;
    int half = kb, tap = q, step = c16 * 25 + q;
    if (!transposed && S == 2) {                 // ring layout: half-chunk pairing (two taps per step)
      half = (q < 12) ? 0 : (q == 12 ? kb : 1);
      tap = (q < 12) ? 2 * q + kb : (q == 12 ? 24 : 2 * (q - 13) + kb);
    } else if (transposed) {                     // parity classes, class-major step order
      const int kh = q / 5, kw = q - 5 * kh;
      const int R = kh % S, SS = kw % S, ntw = class_taps(S, SS);
      step = class_taps_before(S, R, SS) * nchunks + c16 * (class_taps(S, R) * ntw) + (kh / S) * ntw + kw / S;
    }
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = T[col * PK_PITCH + (half * 8 + j) * 25 + tap] * wscale;
    f32x4 pl[3];                                 // hi, (mid,) lo
    if (f16) split_planes16<2, true>(v, pl);
    else if (planes == 2) split_planes16<2, false>(v, pl);
    else split_planes16<3, false>(v, pl);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (cok && k < planes) p[((size_t)step * planes * 2 + k * 2 + kb) * CoutP + co0 + col] = __builtin_bit_cast(bf16x8, pl[k]);
  }
  // the spare steps (the DMA ring's run-ahead reads them): zeros, written by the first chunk's workgroups
  if (c16 == 0 && cok) {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
    for (int u = tid / PK_CO; u < VG_PACK_SPARE * planes * 2; u += 256 / PK_CO) p[((size_t)nsteps * planes * 2 + u) * CoutP + co0 + col] = z;
  }
}

__global__ __launch_bounds__(256) void pack_bf16split_kernel(const float* __restrict__ w, bf16x8* __restrict__ p,
                                                         int Cout, int Cin, int CoutP, int nsteps, int transposed,
                                                         int S, int planes, const float* __restrict__ w_amax) {
  __shared__ float T[PK_CO * PK_PITCH];          // [channel][ci16 * 25 + tap]
  pack_bf16split_body(T, w, p, Cout, Cin, CoutP, nsteps, transposed, S, planes, w_amax, blockIdx.x, blockIdx.y);
}

// Several filters in ONE launch (every filter an optimizer step has just changed): a pack is latency-bound (8 us for
// 0.2-6.5 MB), so 6-16 of them side by side take about as long as one.
constexpr int PK_MAXE = 24;
struct PackBatch {
  const float* w[PK_MAXE];
  const float* w_amax[PK_MAXE];
  bf16x8* p[PK_MAXE];
  int Cout[PK_MAXE], Cin[PK_MAXE], transposed[PK_MAXE], S[PK_MAXE];
  unsigned first_block[PK_MAXE + 1];
  int count;
};

__global__ __launch_bounds__(256) void pack_bf16split_multi_kernel(PackBatch P, int planes) {
  __shared__ float T[PK_CO * PK_PITCH];
  int t = 0;
  while (t + 1 < P.count && blockIdx.x >= P.first_block[t + 1]) ++t;
  const int CoutP = packed_cout(P.Cout[t]), nbx = CoutP / PK_CO;
  const int b = blockIdx.x - P.first_block[t];
  pack_bf16split_body(T, P.w[t], P.p[t], P.Cout[t], P.Cin[t], CoutP, P.Cin[t] / 16 * 25, P.transposed[t], P.S[t], planes,
                      P.w_amax[t], b % nbx, b / nbx);
}

// the shape every entry point of the split arithmetics takes
bool shape_ok(int B, int Cin, int H, int W, int Cout, int stride, int planes) {
  return conv_shape_ok(B, Cin, H, W, Cout, stride) && Cin % 16 == 0 && planes_ok(planes);
}

bool x_args_ok(const float* x, const void* packed, float* y, int B, int Cin, int H, int W, int Cout, int stride, int planes) {
  return x && packed && y && ((uintptr_t)packed & 15) == 0 && shape_ok(B, Cin, H, W, Cout, stride, planes);
}

// Stride 2 runs on the 8-wave ring kernel (conv_ring.hip) -- except transposed convolutions with <= 64 output
// channels, whose thin tiles (32 cout x 128 / 256 pixels) live here; stride 1 runs here.
bool on_ring(int mode, int Cout, int stride) { return stride == 2 && (mode == CONV_FWD || Cout > 64); }

// The layers that stay here take no fusion (vg_conv5x5_bf16split_fusable says which do); in_amax is not one.
bool fuse_empty(const vg_conv_fusion* f) { return !f || (!f->in_scale && !f->in_shift && !f->stats); }

// (planes, stride) -> dispatch_x<MODE, S, NP, F16>
template <int MODE>
int dispatch_planes(const float* x, const void* packed, const float* bias, float* y, int B, int Cin, int H, int W, int Cout,
                    int stride, int planes, void* workspace, size_t workspace_bytes, const vg_conv_fusion* fuse, hipStream_t st) {
  return for_planes(planes, [&](auto np, auto f16) {
    auto run = [&](auto s) {
      return dispatch_x<MODE, decltype(s)::value, decltype(np)::value, decltype(f16)::value != 0>(
          x, (const bf16x8*)packed, bias, y, B, Cin, H, W, Cout, workspace, workspace_bytes, fuse ? fuse->in_amax : nullptr, st);
    };
    if constexpr (MODE == CONV_FWD) return run(IntC<1>{});
    else return for_stride(stride, run);
  });
}

}  // namespace

#ifdef VG_TUNING
extern "C" int vg_debug_set_conv_bf16split_tile(int variant) {
  g_x_tile_override = variant;
  return 0;
}

extern "C" int vg_debug_set_conv_ring_tile(int variant) {
  vg_internal_ring_set_variant(variant);
  return 0;
}
#endif

extern "C" size_t vg_conv5x5_packed_bf16split_bytes(int Cout, int Cin, int planes) {
  if (Cout <= 0 || Cin <= 0 || Cin % 16 || !planes_ok(planes)) return 0;
  // fp16 planes: + a 16-byte trailer holding the inverse of the filter's power-of-two scale
  return vg_pack_trailer_units(Cin / 16 * 25, planes & 0xff, packed_cout(Cout)) * 16 +
         ((planes & VG_PLANES_F16_FLAG) ? 16 : 0);
}

extern "C" int vg_conv5x5_pack_bf16split(const float* w, void* packed, int Cout, int Cin, int transposed, int stride,
                                      int planes, const float* w_amax, void* stream) {
  if (!w || !packed || Cout <= 0 || Cin <= 0 || Cin % 16 || ((uintptr_t)packed & 15)) return VG_ERR_BAD_ARG;
  if ((stride != 1 && stride != 2) || !planes_ok(planes)) return VG_ERR_BAD_ARG;
  if ((planes & VG_PLANES_F16_FLAG) && !w_amax) return VG_ERR_BAD_ARG;
  const int CoutP = packed_cout(Cout), nsteps = Cin / 16 * 25;
  hipLaunchKernelGGL(pack_bf16split_kernel, dim3(CoutP / PK_CO, Cin / 16), dim3(256), 0,
                     (hipStream_t)stream, w, (bf16x8*)packed, Cout, Cin, CoutP, nsteps, transposed ? 1 : 0, stride, planes,
                     w_amax);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_conv5x5_pack_bf16split_multi(const VgPackEntry* entries, int count, int planes, void* stream) {
  if (count < 0 || (count > 0 && !entries) || !planes_ok(planes)) return VG_ERR_BAD_ARG;
  int i = 0;
  while (i < count) {
    PackBatch P;
    P.count = 0;
    unsigned blocks = 0;
    while (i < count && P.count < PK_MAXE) {
      const VgPackEntry& E = entries[i++];
      if (!E.w || !E.packed || E.Cout <= 0 || E.Cin <= 0 || E.Cin % 16 || ((uintptr_t)E.packed & 15) ||
          (E.stride != 1 && E.stride != 2) || ((planes & VG_PLANES_F16_FLAG) && !E.w_amax))
        return VG_ERR_BAD_ARG;
      const int k = P.count++;
      P.w_amax[k] = E.w_amax;
      P.w[k] = E.w; P.p[k] = (bf16x8*)E.packed; P.Cout[k] = E.Cout; P.Cin[k] = E.Cin;
      P.transposed[k] = E.transposed ? 1 : 0; P.S[k] = E.stride;
      P.first_block[k] = blocks;
      blocks += (unsigned)(packed_cout(E.Cout) / PK_CO) * (unsigned)(E.Cin / 16);
    }
    P.first_block[P.count] = blocks;
    hipLaunchKernelGGL(pack_bf16split_multi_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, P, planes);
    VG_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" size_t vg_conv5x5_fwd_bf16split_workspace_bytes(int B, int Cin, int H, int W, int Cout, int stride, int planes) {
  if (!shape_ok(B, Cin, H, W, Cout, stride, planes)) return 0;
  if (stride == 2) return vg_internal_ring_workspace_bytes(CONV_FWD, B, Cin, H, W, Cout, planes);
  return x_plan<CONV_FWD, 1, 2, false>(B, Cin, H, W, Cout).slab_bytes;      // (the K split does not look at the planes)
}

extern "C" int vg_conv5x5_bf16split_fusable(int transposed, int Cin, int Cout, int stride) {
  if (Cin <= 0 || Cin % 16 || Cout <= 0) return 0;
  return on_ring(transposed ? CONV_TR : CONV_FWD, Cout, stride) ? 1 : 0;
}

extern "C" size_t vg_conv5x5_fwd_bf16split_stats_floats(int B, int Cin, int H, int W, int Cout, int stride, int planes) {
  if (!shape_ok(B, Cin, H, W, Cout, stride, planes) || !on_ring(CONV_FWD, Cout, stride)) return 0;
  return vg_internal_ring_stats_floats(CONV_FWD, B, Cin, H, W, Cout, planes);
}

extern "C" size_t vg_convT5x5_fwd_bf16split_stats_floats(int B, int Cin, int H, int W, int Cout, int stride, int planes) {
  if (!shape_ok(B, Cin, H, W, Cout, stride, planes) || !on_ring(CONV_TR, Cout, stride)) return 0;
  return vg_internal_ring_stats_floats(CONV_TR, B, Cin, H, W, Cout, planes);
}

extern "C" int vg_conv5x5_fwd_bf16split(const float* x, const void* packed, const float* bias, float* y, int B, int Cin,
                                     int H, int W, int Cout, int stride, int planes, void* workspace,
                                     size_t workspace_bytes, const vg_conv_fusion* fuse, void* stream) {
  if (!x_args_ok(x, packed, y, B, Cin, H, W, Cout, stride, planes)) return VG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (on_ring(CONV_FWD, Cout, stride))
    return vg_internal_ring_conv(CONV_FWD, x, packed, bias, y, B, Cin, H, W, Cout, planes, workspace, workspace_bytes, fuse, st);
  if (!fuse_empty(fuse)) return VG_ERR_BAD_ARG;
  return dispatch_planes<CONV_FWD>(x, packed, bias, y, B, Cin, H, W, Cout, stride, planes, workspace, workspace_bytes, fuse, st);
}

extern "C" size_t vg_convT5x5_fwd_bf16split_workspace_bytes(int B, int Cin, int H, int W, int Cout, int stride, int planes) {
  if (!shape_ok(B, Cin, H, W, Cout, stride, planes)) return 0;
  return on_ring(CONV_TR, Cout, stride) ? vg_internal_ring_workspace_bytes(CONV_TR, B, Cin, H, W, Cout, planes) : 0;
}

extern "C" int vg_convT5x5_fwd_bf16split(const float* x, const void* packed, const float* bias, float* y, int B, int Cin,
                                      int H, int W, int Cout, int stride, int planes, void* workspace,
                                      size_t workspace_bytes, const vg_conv_fusion* fuse, void* stream) {
  if (!x_args_ok(x, packed, y, B, Cin, H, W, Cout, stride, planes)) return VG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (on_ring(CONV_TR, Cout, stride))
    return vg_internal_ring_conv(CONV_TR, x, packed, bias, y, B, Cin, H, W, Cout, planes, workspace, workspace_bytes, fuse, st);
  if (!fuse_empty(fuse)) return VG_ERR_BAD_ARG;
  return dispatch_planes<CONV_TR>(x, packed, bias, y, B, Cin, H, W, Cout, stride, planes, workspace, workspace_bytes, fuse, st);
}
