// Linear layers in the fp16x3 arithmetic (vg_gemm_nt_f16x3) for gfx950: the three GEMMs of nn.Linear's forward /
// backward on the big layers of the path (encoder 16384 -> 2048, /root/reference/models/model.py:460-471; discriminator
// lth_features 16384 -> 2048, :402-404; decoder 128 -> 16384, :490-492), where the vendor's fp32 GEMM is bound by the
// fp32 MFMA (~100-150 TFLOP/s: 62-83 us per launch) and the 134 MB weight could stream in a third of that time:
//
//     C[m][n] = sum_k A(m, k) * B(n, k) (+ bias[n]),      A(m, k) = A[m * ars + k * aks],  B(n, k) = B[n * brs + k * bks]
//
// with, per operand, either the reduction index contiguous (k stride 1) or the row index contiguous (row stride 1):
//   forward   y  = x W^T   : A = x  (ars = K,  aks = 1),   B = W (brs = K, bks = 1)
//   data grad gx = gy W    : A = gy (ars = N', aks = 1),   B = W read as [k_in][n] (brs = 1, bks = K_in)
//   weight gr gW = gy^T x  : A = gy read as [n][b] (ars = 1, aks = N'),   B = x read as [k][b] (brs = 1, bks = K_in)
// Same arithmetic as the convolutions (conv_ring.hip): each fp32 operand times an exact power of two
// from a device-side bound of its largest magnitude, split into fp16 hi + lo, the products lo*hi, hi*lo, hi*hi on
// v_mfma_f32_32x32x16_f16, fp32 accumulation, the two scales undone on the accumulators.  (Rounds 2-3 had this kernel
// with three bf16 planes -- 6 MFMAs per multiply, matrix-bound, level with the vendor library -- and removed it; at 3
// MFMAs the weight stream is the bound.)
//
// One workgroup = 8 wavefronts (2 x 4 of 64 x 32) owns a 128 x 128 output tile and a
// slice of the reduction (K split over workgroups; partial tiles go to slabs summed in a fixed order: no atomics).  A
// stage = 32 reduction indices: a thread stages one 8-index unit of A and one of B -- two 16-byte loads each where the
// reduction index is contiguous, eight 4-byte loads (a row apart; consecutive lanes = consecutive rows, coalesced)
// where it is not -- G_PD stages ahead in registers, splits them into planes and writes two 16-byte LDS units each
// ([plane][k-block][row], k-blocks padded by two units so that the 4 lanes that share a row do not share banks);
// stages are double-buffered in LDS, ONE barrier per stage.  Plain loads only: hipcc counts vmcnt itself.
//
// Grouped form (vg_gemm_nt_f16x3_grouped, template parameter NG = 1..3): NG activations A_g against the SAME B -- the
// discriminator's passes of one phase over its unchanged 16384 x 2048 weight.  A workgroup owns its (tile, K slice) for
// all groups: a stage loads, scales, splits and writes the B unit once, stages NG A units and runs each group's 12
// MFMAs against the same B fragments into the group's own accumulators.  Tiling, K slicing, the order of a group's
// MFMAs, the epilogue and the slab sum are those of a single call, so C_g is bit for bit vg_gemm_nt_f16x3 on A_g.
#include "common.hpp"
#include "vaegan_hip.h"

namespace {

// M16 (template parameter of the kernel): the products on v_mfma_f32_16x16x32_f16 (a stage IS one K = 32 step: the four
// k-blocks of the LDS layout are the four k-groups of its operands) instead of two K = 16 steps of 32x32x16; the output tile
// is computed transposed (D[n][m]) so that a lane holds four consecutive n of one row m: 16-byte stores.  Measured
// (profiles/r04_logs/r4_abl_gemm6.log): data gradient 61-62 us against 66-67, forward 62 against 62-67; but 154 VGPRs
// instead of 126-137 -- one workgroup per CU instead of two -- and the weight gradient, whose grids are thousands of
// short workgroups, 78-80 us against 75-76 (111 against 101 at batch 256): G_M16 = 2 picks it for grids of <= 512
// workgroups (the whole benchmark: 13.52-13.57 ms against 14.02-14.05 with the vendor GEMMs, r4_lin_ab4.log; the 32x32x16
// form: 13.69-13.71 against 14.07-14.13).  OFF in the product (G_M16 = 0 / 1 / 2: never / always / by grid): its different
// summation order moved one fused-vs-two-pass gradient comparison at batch 8 (tests/test_step_gpu.py, convs.0.weight) from
// under its 1e-3 bound to 1.25e-3 with no counted unit flip; that bound is re-derived before this becomes the default.
#ifndef G_M16
#define G_M16 0
#endif
// 8 wavefronts (2 x 4 of 64 x 32) per tile rather than 4 (2 x 2 of 64 x 64): two wavefronts per SIMD on the grids that
// give every CU one workgroup only (forward / data gradient at batch 128), half the staging per thread
constexpr int GNT = 512, GTM = 128, GTN = 128, GKC = 32;     // threads, tile rows / columns, reduction indices per stage
constexpr int G_HN = 1;                                      // 32-column fragments per wavefront
constexpr int GPAD = 2;
constexpr int G_KB = GTM + GPAD;                             // units per k-block (A and B tiles have the same height)
constexpr int G_PL = 4 * G_KB;                               // units per plane
constexpr int G_NP = 2;                                      // fp16 hi + lo
constexpr int G_PD = 3;                                      // register slots: two stages in flight, one being split
constexpr int G_NU = 1;                                      // staged units per thread and operand
static_assert(GTM == GTN && GTM * 4 == G_NU * GNT, "staging map");

constexpr int G_MAXG = VG_GEMM_MAX_GROUPS;

struct GArgs {
  const float* A[G_MAXG];   // per group
  const float* B;
  const float* bias;
  float* C[G_MAXG];         // per group; ksplit == 1: the output [M][N]; else the group's slabs [ksplit][M][N]
  int M, N, K;
  long ars, aks, brs, bks;
  int kper;            // reduction indices per split (multiple of GKC)
  int ksplit;
  int tiles_m, tiles_n;
  const float* a_amax[G_MAXG];   // device: upper bounds of max |A_g|, max |B|
  const float* b_amax;
};

// The Adam half of the fused weight-gradient step (vg_linear_wgrad_adam, _dev): the tile's gradient never leaves the
// workgroup (g_out apart) -- it is the g of the plain Adam step on the tile's p, m, v (row-major [G.M][G.N], as C).
struct WAdam {
  float* p;
  float* m;
  float* v;
  unsigned* amax;           // may be NULL: max |p| after the update is added here (atomic max)
  unsigned* flag;           // may be NULL: VG_NONFINITE_* bits are ORed in here
  float* g_out;             // may be NULL: the gradient is stored here as well
  float omb1, b2, omb2, step_size, bc2s, eps;
  const float* scalars;     // NULL, or the device words [step_size, bc2s] of vg_adam_prepare
};
constexpr int G_TSTR = GTN / 4 + 1;      // fused step: 16-byte units per row of the gradient tile in LDS (one of padding)
constexpr int G_TIT = GTM * (GTN / 4) / GNT;      // ... and 16-byte units of it per thread

__device__ __forceinline__ void load8(float* r, const float* p, long ks, bool strided) {
  if (strided) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = p[(size_t)j * ks];
  } else {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  }
}

// AT / BT: the operand's ROW index is the contiguous one (reduction index strided); NG: groups (A_g, C_g) sharing B.
// NG > 1: one workgroup per CU (LDS: 2 x (NG + 1) x 16.6 KB; NG accumulator sets)
//
// ADAM (the fused weight-gradient step; AT, BT, no K split, one group): the tile is not stored.  A thread owns G_TIT
// 16-byte units of the tile's p, m, v -- unit (row it * 16 + tid / 32, columns 4 (tid % 32) ..): a wavefront covers two
// whole 512-byte row segments.  After the last stage the accumulators go through LDS (the staging buffers are free
// then) into that layout: 16-byte accesses on p, m, v, whole rows of the tile per wavefront.  The gradient element is the
// epilogue's own expression; the update is adam_one_as' "body" form: p, m, v, the amax word and the flag bits are those
// of vg_gemm_nt_f16x3 followed by the plain Adam step.
template <bool AT, bool BT, bool M16, int NG, bool ADAM>
__device__ __forceinline__ void gemm_nt_f16x3_body(const GArgs& G, const WAdam& W) {
  static_assert(!ADAM || (AT && BT && !M16 && NG == 1 && G_HN == 1), "the fused step is the weight gradient's orientation");
  constexpr int NA = NG * G_NU, NUN = NA + G_NU;       // staged units per thread: [0, NA) A of group u / G_NU; then B
  constexpr int BOFF = G_NP * NG * G_PL;               // B planes follow the groups' A planes
  constexpr int BUFU = BOFF + G_NP * G_PL;
  constexpr int LDSU = (ADAM && GTM * G_TSTR > 2 * BUFU) ? GTM * G_TSTR : 2 * BUFU;
  __shared__ f32x4 lds[LDSU];                          // [buffer][A_0 planes | .. | A_{NG-1} planes | B planes][k-block][row]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kb = lane >> 5, l32 = lane & 31;
  const int wm = wid & 1, wn = wid >> 1;                // 2 x 4 wavefronts of 64 rows x 32 columns
  const int wcol = wn * 32 * G_HN;
  // workgroup -> (row tile, column tile, split).  Splits are dealt to the XCDs (blockIdx round-robins over the 8 of
  // them): the workgroups of one split -- they read the same reduction slice of A -- follow each other through one L2,
  // row tiles of one column tile (same slice of B) back to back.
  int mt, nt, split;
  {
    const int per = G.tiles_m * G.tiles_n;             // workgroups per split
    int bid = blockIdx.x;
    if (G.ksplit % 8 == 0) {
      const int xcd = bid & 7, j = bid >> 3;
      split = xcd + 8 * (j / per);
      bid = j % per;
    } else {
      split = bid / per;
      bid -= split * per;
    }
    nt = bid / G.tiles_m;
    mt = bid - nt * G.tiles_m;
  }
  const int m0 = mt * GTM, n0 = nt * GTN;
  const int k_begin = split * G.kper, k_end = min(k_begin + G.kper, G.K);
  const int nst = (k_end - k_begin) / GKC;
  const float b_scale = f16_scale_of(*G.b_amax);
  float a_scale[NG];
#pragma unroll
  for (int gi = 0; gi < NG; ++gi) a_scale[gi] = f16_scale_of(*G.a_amax[gi]);

  // ---- staging map: unit (row, k-block) -> thread.  Reduction contiguous: 4 consecutive lanes cover the 32 indices
  // (128 B) of a row; row contiguous: consecutive lanes = consecutive rows, the unit's 8 indices a k-stride apart.
  // the groups' A units share one map (same M and strides): slots [0, G_NU) describe A, [G_NU, 2 G_NU) B
  size_t u_off[2 * G_NU];
  int u_dst[2 * G_NU];
  bool u_ok[2 * G_NU];
#pragma unroll
  for (int u = 0; u < 2 * G_NU; ++u) {
    const bool isb = u >= G_NU, tr = isb ? BT : AT;
    const int e = tid + GNT * (u % G_NU);
    const int row = tr ? (e & (GTM - 1)) : (e >> 2), kblk = tr ? (e >> 7) : (e & 3);
    const int r0 = isb ? n0 : m0, rmax = isb ? G.N : G.M;
    const long rs = isb ? G.brs : G.ars, ks = isb ? G.bks : G.aks;
    u_ok[u] = (r0 + row) < rmax;
    u_off[u] = (size_t)min(r0 + row, rmax - 1) * rs + (size_t)(k_begin + kblk * 8) * ks;
    u_dst[u] = kblk * G_KB + row;
  }

  float rg[G_PD][NUN][8];
  auto load_stage = [&](int slot, int st) {            // st: stage index within this split
#pragma unroll
    for (int u = 0; u < NUN; ++u) {
      const bool isb = u >= NA;
      const float* p = (isb ? G.B : G.A[isb ? 0 : u / G_NU]) + u_off[isb ? G_NU + (u - NA) : u % G_NU];
      load8(rg[slot][u], p + (size_t)st * GKC * (isb ? G.bks : G.aks), isb ? G.bks : G.aks, isb ? BT : AT);
    }
  };
  // one staged unit: scale, split into hi / lo, two LDS units
  auto piece = [&](int slot, int u, f32x4* base) {
    float* v = rg[slot][u];
    const bool isb = u >= NA;
    const int m = isb ? G_NU + (u - NA) : u % G_NU;
    // rows beyond M / N (clamped re-reads of the last row) are multiplied by zero: they only ever meet output rows /
    // columns that are not stored
    const float sc = u_ok[m] ? (isb ? b_scale : a_scale[isb ? 0 : u / G_NU]) : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= sc;
    f32x4 pl[G_NP];
    split_planes16<G_NP, true>(v, pl);
    const int dst = u_dst[m] + (isb ? BOFF : (u / G_NU) * G_NP * G_PL);
    base[dst] = pl[0];
    base[dst + G_PL] = pl[1];
  };
  auto read_a = [&](bf16x8 (&av)[2][G_NP], const f32x4* base, int gi, int s2) {
#pragma unroll
    for (int p = 0; p < G_NP; ++p)
#pragma unroll
      for (int g = 0; g < 2; ++g)
        av[g][p] = __builtin_bit_cast(bf16x8, base[(gi * G_NP + p) * G_PL + (2 * s2 + kb) * G_KB + wm * 64 + g * 32 + l32]);
  };
  auto read_b = [&](bf16x8 (&bv)[G_HN][G_NP], const f32x4* base, int s2) {
#pragma unroll
    for (int p = 0; p < G_NP; ++p)
#pragma unroll
      for (int h = 0; h < G_HN; ++h)
        bv[h][p] = __builtin_bit_cast(bf16x8, base[BOFF + p * G_PL + (2 * s2 + kb) * G_KB + wcol + h * 32 + l32]);
  };

  f32x16 acc[NG][2][G_HN];
#pragma unroll
  for (int gi = 0; gi < NG; ++gi)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int h = 0; h < G_HN; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[gi][g][h][r] = 0.f;
  // 16x16x32 form: 4 row blocks x 2 G_HN column blocks of 16 x 16, lane = (k-group q, index l16 within the block)
  const int q16 = lane >> 4, l16 = lane & 15;
  f32x4 acc4[NG][4][2 * G_HN];
#pragma unroll
  for (int gi = 0; gi < NG; ++gi)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int h = 0; h < 2 * G_HN; ++h) acc4[gi][g][h] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto read_a16 = [&](bf16x8 (&xa)[4][G_NP], const f32x4* base, int gi) {
#pragma unroll
    for (int p = 0; p < G_NP; ++p)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        xa[g][p] = __builtin_bit_cast(bf16x8, base[(gi * G_NP + p) * G_PL + q16 * G_KB + wm * 64 + g * 16 + l16]);
  };
  auto read_b16 = [&](bf16x8 (&xb)[2 * G_HN][G_NP], const f32x4* base) {
#pragma unroll
    for (int p = 0; p < G_NP; ++p)
#pragma unroll
      for (int h = 0; h < 2 * G_HN; ++h)
        xb[h][p] = __builtin_bit_cast(bf16x8, base[BOFF + p * G_PL + q16 * G_KB + wcol + h * 16 + l16]);
  };

  // fused step: this thread's units of the tile
  const int t_row = tid >> 5, t_col = n0 + 4 * (tid & 31);      // (G.N % 4 == 0: a unit is inside the row or outside)
  auto t_ok = [&](int it) { return m0 + it * (GNT / 32) + t_row < G.M && t_col < G.N; };
  auto t_off = [&](int it) { return (size_t)(m0 + it * (GNT / 32) + t_row) * G.N + t_col; };

  if (nst > 0) {
    // stages past the end re-load the last one (never consumed): every register slot always holds valid data
#pragma unroll
    for (int j = 0; j < G_PD; ++j) load_stage(j, min(j, nst - 1));
#pragma unroll
    for (int u = 0; u < NUN; ++u) piece(0, u, lds);
    __syncthreads();
    // One stage: per group 6 batches of 2 MFMAs (2 steps of 16 x the 3 plane products), ordered step, group, product:
    // the B fragments of a step serve every group.  The split of stage st + 1 (NG + 1 units) rides on the first
    // batches, one unit each; the A fragments of the next (step, group) -- and the B fragments of the next step -- are
    // read during the second batch of the one before.  `j`: the
    // register slot that held stage st (compile-time: the loop below is unrolled by G_PD with no branch inside -- with
    // a per-stage `if (st < nst)` hipcc's vmcnt bookkeeping lost track across the joins and drained every load in
    // front of the next stage's address arithmetic).
    auto stage = [&](int st, int j) {
      const int buf = st & 1;
      const f32x4* base = lds + buf * BUFU;
      f32x4* nxt = lds + (buf ^ 1) * BUFU;           // stage st + 1 (loaded G_PD - 1 stages ago) goes here --
                                                     // after the last stage too (a re-store nobody reads): no branch
      load_stage(j, min(st + G_PD, nst - 1));        // slot j held stage st: split during stage st - 1
      if constexpr (M16) {
      bf16x8 xa[4][G_NP], xb[2 * G_HN][G_NP];
      read_b16(xb, base);
      int grp16 = 0;
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
      read_a16(xa, base, gi);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int sum = G_NP - 1; sum >= 0; --sum)
#pragma unroll
        for (int pa = sum; pa >= 0; --pa) {           // 3 batches of 8 G_HN MFMAs per group, the split of stage st + 1 rides on them
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int h = 0; h < 2 * G_HN; ++h)
              acc4[gi][g][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, xb[h][sum - pa]),
                                                                     __builtin_bit_cast(f16x8, xa[g][pa]), acc4[gi][g][h], 0, 0, 0);
#pragma unroll
          for (int u = grp16; u < NUN; u += 3 * NG) piece((j + 1) % G_PD, u, nxt);
          __builtin_amdgcn_sched_barrier(0);
          ++grp16;
        }
      }
      __syncthreads();
      return;
      }
      bf16x8 av[2][2][G_NP], bv[2][G_HN][G_NP];      // A: [parity of (step, group)], B: [step]
      read_a(av[0], base, 0, 0);
      read_b(bv[0], base, 0);
      __builtin_amdgcn_sched_barrier(0);
      int grp = 0;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
          const int sg = s2 * NG + gi, cur = sg & 1;
          int sub = 0;
#pragma unroll
          for (int sum = G_NP - 1; sum >= 0; --sum)
#pragma unroll
            for (int pa = sum; pa >= 0; --pa) {
#pragma unroll
              for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int h = 0; h < G_HN; ++h)
                  acc[gi][g][h] = mfma_split16<true>(av[cur][g][pa], bv[s2][h][sum - pa], acc[gi][g][h]);
              if (grp < NUN) piece((j + 1) % G_PD, grp, nxt);
              if (sub == 1 && sg + 1 < 2 * NG) {
                read_a(av[cur ^ 1], base, (sg + 1) % NG, (sg + 1) / NG);
                if (gi == NG - 1) read_b(bv[1], base, 1);
              }
              __builtin_amdgcn_sched_barrier(0);
              ++grp, ++sub;
            }
        }
      __syncthreads();
    };
    int st = 0;
    for (; st + G_PD <= nst; st += G_PD) {
#pragma unroll
      for (int j = 0; j < G_PD; ++j) stage(st + j, j);
    }
    // the last nst % G_PD stages (slots 0, 1 in turn: the loop above left at a multiple of G_PD)
    if (st < nst) stage(st, 0);
    if (st + 1 < nst) stage(st + 1, 1);
    static_assert(G_PD == 3, "tail above");
  }

  // ---- epilogue: undo the two scales (exact), C (or this split's slab) row-major [M][N]; the bias goes in with split 0
  const float ub = f16_unscale_of(*G.b_amax);
  if constexpr (ADAM) {
    const float ua = f16_unscale_of(*G.a_amax[0]);
    float* const tile = reinterpret_cast<float*>(lds);      // (every stage ends with a barrier: the buffers are free)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int r16 = 0; r16 < 16; ++r16)
        tile[(wm * 64 + g * 32 + acc_row(r16, lane)) * (4 * G_TSTR) + wcol + l32] = acc[0][g][0][r16] * ua * ub + 0.f;
    __syncthreads();
    float step_size = W.step_size, bc2s = W.bc2s;
    if (W.scalars) {
      step_size = W.scalars[0];
      bc2s = W.scalars[1];
    }
    unsigned am = 0, gm = 0;
    // G_TB units at a time: their p, m, v loads are issued together, in the registers the accumulators have left
    constexpr int G_TB = 4;
    static_assert(G_TIT % G_TB == 0, "batches of the fused step");
#pragma unroll
    for (int it0 = 0; it0 < G_TIT; it0 += G_TB) {
    f32x4 sp[G_TB], sm[G_TB], sv[G_TB];
#pragma unroll
    for (int j = 0; j < G_TB; ++j) {
      sp[j] = sm[j] = sv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t_ok(it0 + j)) {
        sp[j] = *reinterpret_cast<const f32x4*>(W.p + t_off(it0 + j));
        sm[j] = *reinterpret_cast<const f32x4*>(W.m + t_off(it0 + j));
        sv[j] = *reinterpret_cast<const f32x4*>(W.v + t_off(it0 + j));
      }
    }
#pragma unroll
    for (int it = it0; it < it0 + G_TB; ++it) {
      if (!t_ok(it)) continue;
      const f32x4 gv = lds[(it * (GNT / 32) + t_row) * G_TSTR + (tid & 31)];
      f32x4 pv = sp[it - it0], mv = sm[it - it0], vv = sv[it - it0];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        adam_one_as(true, pj, gv[j], mj, vj, W.omb1, W.b2, W.omb2, step_size, bc2s, W.eps);
        pv[j] = pj; mv[j] = mj; vv[j] = vj;
        am = max(am, abs_bits(pj));
        gm = max(gm, abs_bits(gv[j]));
      }
      *reinterpret_cast<f32x4*>(W.p + t_off(it)) = pv;
      *reinterpret_cast<f32x4*>(W.m + t_off(it)) = mv;
      *reinterpret_cast<f32x4*>(W.v + t_off(it)) = vv;
      if (W.g_out) *reinterpret_cast<f32x4*>(W.g_out + t_off(it)) = gv;
    }
    }
    emit_amax_and_flags<GNT>(am, gm, W.amax, W.flag);
    return;
  }
#pragma unroll
  for (int gi = 0; gi < NG; ++gi) {
  const float ua = f16_unscale_of(*G.a_amax[gi]);
  float* out = G.C[gi] + (G.ksplit > 1 ? (size_t)split * G.M * G.N : 0);
  if constexpr (M16) {
    const bool vec = (G.N & 3) == 0;
#pragma unroll
    for (int h = 0; h < 2 * G_HN; ++h) {
      const int n = n0 + wcol + h * 16 + 4 * q16;      // this lane's four consecutive columns
      float bvv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) bvv[r] = (G.bias && split == 0 && n + r < G.N) ? G.bias[n + r] : 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int m = m0 + wm * 64 + g * 16 + l16;
        if (m >= G.M) continue;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc4[gi][g][h][r] * ua * ub + bvv[r];
        float* o = out + (size_t)m * G.N + n;
        if (vec && n + 3 < G.N) *reinterpret_cast<f32x4*>(o) = v;
        else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < G.N) o[r] = v[r];
        }
      }
    }
    continue;
  }
#pragma unroll
  for (int h = 0; h < G_HN; ++h) {
    const int n = n0 + wcol + h * 32 + l32;
    const float bvv = (G.bias && split == 0 && n < G.N) ? G.bias[n] : 0.f;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int r16 = 0; r16 < 16; ++r16) {
        const int m = m0 + wm * 64 + g * 32 + acc_row(r16, lane);
        if (m < G.M && n < G.N) out[(size_t)m * G.N + n] = acc[gi][g][h][r16] * ua * ub + bvv;
      }
  }
  }
}

template <bool AT, bool BT, bool M16, int NG>
__global__ __launch_bounds__(GNT, NG == 1 ? 2 : 1) void gemm_nt_f16x3_kernel(GArgs G) {
  gemm_nt_f16x3_body<AT, BT, M16, NG, false>(G, WAdam{});
}

// The fused weight-gradient step: two workgroups per CU, as the GEMM -- one streams its p, m, v while the other is in its
// reduction or in the update's divisions and square roots (one workgroup per CU with the tile's state loaded under the
// reduction left the memory pipe idle through both: DESIGN.md section 4.19).
__global__ __launch_bounds__(GNT, 2) void linear_wgrad_adam_kernel(GArgs G, WAdam W) {
  gemm_nt_f16x3_body<true, true, false, 1, true>(G, W);
}

// One thread: the weight's bound word back to zero in front of the fused step's atomic maxima -- in stream order behind
// the layer's data-gradient GEMM, which still scales the weight by the old bound.
__global__ void zero_word_kernel(unsigned* __restrict__ w) { w[0] = 0u; }

// K split: as many splits as keep >= 8 stages each and bring the grid to about G_TARGET_WGS workgroups
constexpr int G_TARGET_WGS = 256;
int gemm_ksplit(int M, int N, int K) {
  const long tiles = (long)cdiv(M, GTM) * cdiv(N, GTN);
  int ks = 1;
  while (tiles * ks * 2 <= G_TARGET_WGS && K % (GKC * ks * 2) == 0 && K / (ks * 2) >= 8 * GKC) ks *= 2;
  return ks;
}

bool gemm_ok(int M, int N, int K, long ars, long aks, long brs, long bks) {
  if (M <= 0 || N <= 0 || K <= 0 || K % GKC) return false;
  if (!((aks == 1 && ars % 4 == 0) || ars == 1)) return false;      // 16-byte loads need aligned rows
  if (!((bks == 1 && brs % 4 == 0) || brs == 1)) return false;
  return true;
}

// ng groups (A[g], C[g], a_amax[g]) against one B; the single call is ng == 1
int gemm_launch(int ng, const float* const* A, const float* B, const float* bias, float* const* C, int M, int N, int K,
                long a_row_stride, long a_k_stride, long b_row_stride, long b_k_stride, const float* const* a_amax,
                const float* b_amax, void* workspace, size_t workspace_bytes, void* stream) {
  if (ng < 1 || ng > G_MAXG || !A || !B || !C || !a_amax || !b_amax) return VG_ERR_BAD_ARG;
  for (int g = 0; g < ng; ++g)
    if (!A[g] || !C[g] || !a_amax[g]) return VG_ERR_BAD_ARG;
  if (!gemm_ok(M, N, K, a_row_stride, a_k_stride, b_row_stride, b_k_stride)) return VG_ERR_BAD_ARG;
  for (int g = 0; g < ng; ++g)
    if (a_k_stride == 1 && ((uintptr_t)A[g] & 15)) return VG_ERR_BAD_ARG;
  if (b_k_stride == 1 && ((uintptr_t)B & 15)) return VG_ERR_BAD_ARG;
  const int ks = gemm_ksplit(M, N, K);
  const size_t slabs = (size_t)ks * M * N;               // floats per group
  if (ks > 1 && (!workspace || workspace_bytes < ng * slabs * sizeof(float))) return VG_ERR_WORKSPACE;
  if ((size_t)M * N > 0x7fffffffUL) return VG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  GArgs G = {};
  for (int g = 0; g < ng; ++g) {
    G.A[g] = A[g];
    G.C[g] = ks > 1 ? (float*)workspace + g * slabs : C[g];
    G.a_amax[g] = a_amax[g];
  }
  G.B = B; G.bias = bias;
  G.M = M; G.N = N; G.K = K;
  G.ars = a_row_stride; G.aks = a_k_stride; G.brs = b_row_stride; G.bks = b_k_stride;
  G.kper = K / ks; G.ksplit = ks;
  G.tiles_m = cdiv(M, GTM); G.tiles_n = cdiv(N, GTN);
  G.b_amax = b_amax;
  const long grid = (long)G.tiles_m * G.tiles_n * ks;
  if (grid > 0x7fffffffL) return VG_ERR_BAD_ARG;
  const bool at = a_k_stride != 1, bt = b_k_stride != 1;
  const dim3 g((unsigned)grid), b(GNT);
  const bool m16 = G_M16 == 1 || (G_M16 == 2 && grid <= 512);
#define VG_GEMM_LAUNCH_NG(AT_, BT_, NG_)                                                                      \
  do {                                                                                                        \
    if (m16) hipLaunchKernelGGL((gemm_nt_f16x3_kernel<AT_, BT_, G_M16 != 0, NG_>), g, b, 0, st, G);           \
    else hipLaunchKernelGGL((gemm_nt_f16x3_kernel<AT_, BT_, false, NG_>), g, b, 0, st, G);                    \
  } while (0)
#define VG_GEMM_LAUNCH(AT_, BT_)                                                                              \
  do {                                                                                                        \
    if (ng == 1) VG_GEMM_LAUNCH_NG(AT_, BT_, 1);                                                              \
    else if (ng == 2) VG_GEMM_LAUNCH_NG(AT_, BT_, 2);                                                         \
    else VG_GEMM_LAUNCH_NG(AT_, BT_, 3);                                                                      \
  } while (0)
  if (at && bt) VG_GEMM_LAUNCH(true, true);
  else if (at) VG_GEMM_LAUNCH(true, false);
  else if (bt) VG_GEMM_LAUNCH(false, true);
  else VG_GEMM_LAUNCH(false, false);
#undef VG_GEMM_LAUNCH
#undef VG_GEMM_LAUNCH_NG
  static_assert(G_MAXG == 3, "dispatch above");
  VG_CHECK_LAUNCH();
  if (ks > 1)                                            // fixed-order sum of each group's slabs
    for (int gi = 0; gi < ng; ++gi) {
      const int rc = vg_internal_wgrad_reduce((const float*)workspace + gi * slabs, C[gi], M * N, ks, st);
      if (rc) return rc;
    }
  return 0;
}

}  // namespace

extern "C" size_t vg_gemm_nt_f16x3_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || K % GKC) return 0;
  const int ks = gemm_ksplit(M, N, K);
  return ks > 1 ? (size_t)ks * M * N * sizeof(float) : 0;
}

extern "C" int vg_gemm_nt_f16x3(const float* A, const float* B, const float* bias, float* C, int M, int N, int K,
                                long a_row_stride, long a_k_stride, long b_row_stride, long b_k_stride,
                                const float* a_amax, const float* b_amax, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (!A || !C || !a_amax) return VG_ERR_BAD_ARG;
  return gemm_launch(1, &A, B, bias, &C, M, N, K, a_row_stride, a_k_stride, b_row_stride, b_k_stride, &a_amax, b_amax,
                     workspace, workspace_bytes, stream);
}

extern "C" size_t vg_gemm_nt_f16x3_grouped_workspace_bytes(int groups, int M, int N, int K) {
  if (groups < 1 || groups > G_MAXG) return 0;
  return groups * vg_gemm_nt_f16x3_workspace_bytes(M, N, K);
}

extern "C" int vg_gemm_nt_f16x3_grouped(int groups, const float* const* A, const float* B, const float* bias,
                                        float* const* C, int M, int N, int K, long a_row_stride, long a_k_stride,
                                        long b_row_stride, long b_k_stride, const float* const* a_amax,
                                        const float* b_amax, void* workspace, size_t workspace_bytes, void* stream) {
  return gemm_launch(groups, A, B, bias, C, M, N, K, a_row_stride, a_k_stride, b_row_stride, b_k_stride, a_amax, b_amax,
                     workspace, workspace_bytes, stream);
}

// ---- the weight gradient of a Linear layer and its Adam step in one kernel -------------------------------------------
namespace {

int wgrad_adam_launch(const float* gy, const float* x, int M, int N, int K, const float* gy_amax, const float* x_amax,
                      float* p, float* m, float* v, float* amax, unsigned* nonfinite, double beta1, double beta2,
                      double eps, float step_size, float bc2s, const float* scalars, float* g_out, void* stream) {
  if (!gy || !x || !gy_amax || !x_amax || !p || !m || !v) return VG_ERR_BAD_ARG;
  // the GEMM is C[N][K] = sum over M: A = gy read as [n][b], B = x read as [k][b]
  if (!gemm_ok(N, K, M, 1, N, 1, K)) return VG_ERR_BAD_ARG;      // (the reduction M is a multiple of 32)
  if (gemm_ksplit(N, K, M) != 1) return VG_ERR_BAD_ARG;          // slabs: the gradient is not complete in one workgroup
  if (K % 4 || ((size_t)N * K) % 4) return VG_ERR_BAD_ARG;       // every element on the step's 16-byte body
  if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g_out) & 15) return VG_ERR_BAD_ARG;
  if ((size_t)N * K > 0x7fffffffUL) return VG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  GArgs G = {};
  G.A[0] = gy; G.B = x; G.a_amax[0] = gy_amax; G.b_amax = x_amax;
  G.M = N; G.N = K; G.K = M;
  G.ars = 1; G.aks = N; G.brs = 1; G.bks = K;
  G.kper = M; G.ksplit = 1;
  G.tiles_m = cdiv(N, GTM); G.tiles_n = cdiv(K, GTN);
  WAdam W = {p, m, v, reinterpret_cast<unsigned*>(amax), nonfinite, g_out, (float)(1.0 - beta1), (float)beta2,
             (float)(1.0 - beta2), step_size, bc2s, (float)eps, scalars};
  if (amax) {
    hipLaunchKernelGGL(zero_word_kernel, dim3(1), dim3(1), 0, st, reinterpret_cast<unsigned*>(amax));
    VG_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(linear_wgrad_adam_kernel, dim3((unsigned)(G.tiles_m * G.tiles_n)), dim3(GNT), 0, st, G, W);
  VG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int vg_linear_wgrad_adam(const float* gy, const float* x, int M, int N, int K, const float* gy_amax,
                                    const float* x_amax, float* p, float* m, float* v, float* amax, unsigned* nonfinite,
                                    double lr, double beta1, double beta2, double eps, double bias_correction1,
                                    double bias_correction2_sqrt, float* g_out, void* stream) {
  if (!(bias_correction1 > 0.0) || !(bias_correction2_sqrt > 0.0)) return VG_ERR_BAD_ARG;
  // scalars formed in double and rounded once, as vg_adam_step forms them
  return wgrad_adam_launch(gy, x, M, N, K, gy_amax, x_amax, p, m, v, amax, nonfinite, beta1, beta2, eps,
                           (float)(lr / bias_correction1), (float)bias_correction2_sqrt, nullptr, g_out, stream);
}

extern "C" int vg_linear_wgrad_adam_dev(const float* gy, const float* x, int M, int N, int K, const float* gy_amax,
                                        const float* x_amax, float* p, float* m, float* v, float* amax,
                                        unsigned* nonfinite, double beta1, double beta2, double eps, const float* scalars,
                                        float* g_out, void* stream) {
  if (!scalars) return VG_ERR_BAD_ARG;
  return wgrad_adam_launch(gy, x, M, N, K, gy_amax, x_amax, p, m, v, amax, nonfinite, beta1, beta2, eps, 0.f, 0.f, scalars,
                           g_out, stream);
}
