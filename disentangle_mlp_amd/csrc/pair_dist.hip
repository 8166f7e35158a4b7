// All-pairs squared Euclidean distances between two feature sets a[M, D] and b[N, D], reduced on the fly to what the
// sample-quality metrics need (k-nearest-neighbour radii, ball-membership counts) for gfx950: DESIGN.md section 4.25,
// include/vaegan_hip.h "vg_pair_*".  Nothing of size M x N ever exists in memory.
//
// A workgroup of 256 threads owns a block of 64 rows of `a` and walks a range of column tiles (64 rows of `b` each).
// Both blocks go through LDS in chunks of 32 dimensions, TRANSPOSED ([d][row], pitch 68): a thread's 4 rows, and its 4
// columns, of one d are one 16-byte LDS read each, and every thread keeps a 4 x 4 tile of pairs in registers -- 32 lane
// operations (16 subtractions, 16 FMAs; the compiler pairs them into 2-wide packed fp32 instructions) per two reads.
// The rows a wavefront reads are 4 addresses (broadcast), its columns 16 consecutive 16-byte slots: one bank row, no
// conflict.  The global -> LDS stage reads 8 consecutive floats of 4 rows per half-wavefront (no alignment beyond a
// float's is assumed: D is arbitrary) and its transposed 4-byte stores fall on 32 different banks (4 d + row); the
// next chunk is fetched into registers while the current one is consumed.
//
// Arithmetic (the house rule of reparam_mmd.hip): d2 = sum_d (a_d - b_d)^2 from the DIFFERENCES, one fp32 FMA chain in
// ascending d, acc = fma(a_d - b_d, a_d - b_d, acc), starting from 0.  A padding dimension adds fma(0, 0, acc) = acc.
// The chain does not depend on the tile, on the split or on the thread; (b_d - a_d) is the exact negation of
// (a_d - b_d), so swapping the operands gives the same bits too, and identical rows give exactly 0.
//
// After the last chunk the 64 x 64 tile of distances goes through LDS (the staging buffer, reused) to the first
// wavefront: lane r owns row r and keeps the running sorted list of the 8 smallest distances, or the running count,
// in registers across its column tiles.  N is cut into `splits` ranges of whole column tiles; every (row block, range)
// writes its partial list / count to the workspace and a merge kernel folds them in range order.  No atomics: the same
// bits every run, and -- the k smallest of a multiset, a sum of integers -- the same bits for every `splits`.
#include "common.hpp"
#include "vaegan_hip.h"

#include <math.h>

namespace {

constexpr int TILE = VG_PAIR_TILE;      // rows of a per workgroup = rows of b per column tile
constexpr int DK = 32;                  // dimensions per LDS chunk
constexpr int PITCH = TILE + 4;         // floats per d in the staged blocks: 16-byte rows, stores on 32 different banks
constexpr int DPITCH = TILE + 1;        // floats per row of the distance tile: a lane per row reads conflict-free
constexpr int NT = 256;
constexpr int KMAX = VG_PAIR_MAX_K;
constexpr int MAX_D = 4096;
constexpr int MAX_MN = 1 << 20;
constexpr int MAX_SPLITS = 1024;
constexpr int AUTO_WGS = 1024;          // splits = 0: enough ranges for four workgroups per CU (256 CUs)

static_assert(TILE == 64 && NT == 256, "16 x 16 threads of 4 x 4 pairs; a lane of the first wavefront per row");
static_assert(KMAX == 8, "the list is eight registers");
static_assert(TILE * DPITCH <= 2 * DK * PITCH, "the distance tile reuses the staging buffer");

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct Plan {
  int row_blocks, col_tiles, splits, tps;      // tps: column tiles per range
  size_t Mpad, bytes;
};

bool dims_ok(int M, int N, int D, int K, int splits) {
  return M >= 1 && M <= MAX_MN && N >= 1 && N <= MAX_MN && D >= 1 && D <= MAX_D && K >= 1 && K <= KMAX && splits >= 0;
}

// The range count for (M, N, requested): a function of the sizes only.  A request above the number of column tiles (or
// above MAX_SPLITS) is CLAMPED; the ranges are then ceil(col_tiles / splits) tiles each and empty ranges are dropped.
Plan make_plan(int M, int N, int K, int splits) {
  Plan p;
  p.row_blocks = cdiv(M, TILE);
  p.col_tiles = cdiv(N, TILE);
  p.Mpad = (size_t)p.row_blocks * TILE;
  int s = splits == 0 ? cdiv(AUTO_WGS, min(p.row_blocks, AUTO_WGS)) : splits;
  s = min(s, min(p.col_tiles, MAX_SPLITS));
  p.tps = cdiv(p.col_tiles, s);
  p.splits = cdiv(p.col_tiles, p.tps);
  p.bytes = ((size_t)p.splits * p.Mpad * K * sizeof(float) + 255) / 256 * 256;      // (an int32 count is a K = 1 list's size)
  return p;
}

// v ascending; x takes its place and the largest of the nine falls out
__device__ __forceinline__ void knn_insert(float (&v)[KMAX], float x) {
#pragma unroll
  for (int s = 0; s < KMAX; ++s) {
    const float lo = fminf(v[s], x);
    x = fmaxf(v[s], x);
    v[s] = lo;
  }
}

// this thread's 8 elements of a [64 rows x 32 d] chunk: element r is (row (2 r + tid / 128) * 4 + (tid / 8) % 4,
// d (tid / 32 % 4) * 8 + tid % 8); rows past `rows` and dimensions past D read as 0
__device__ __forceinline__ void fetch_chunk(const float* __restrict__ x, int row0, int rows, int d0, int D, float (&r)[8]) {
  const int tid = threadIdx.x, d = d0 + ((tid >> 5) & 3) * 8 + (tid & 7);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = row0 + (2 * i + (tid >> 7)) * 4 + ((tid >> 3) & 3);
    r[i] = (row < rows && d < D) ? x[(size_t)row * D + d] : 0.f;
  }
}

__device__ __forceinline__ void stage_chunk(float* __restrict__ s, const float (&r)[8]) {
  const int tid = threadIdx.x, d = ((tid >> 5) & 3) * 8 + (tid & 7);
#pragma unroll
  for (int i = 0; i < 8; ++i) s[d * PITCH + (2 * i + (tid >> 7)) * 4 + ((tid >> 3) & 3)] = r[i];
}

// partial: HITS ? int32 [splits][Mpad] : fp32 [splits][Mpad][K]
template <bool HITS>
__global__ __launch_bounds__(NT) void pair_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                  const float* __restrict__ thr, void* __restrict__ partial, int M, int N,
                                                  int D, int K, int exclude_self, int col_tiles, int tps, size_t Mpad) {
  __shared__ __attribute__((aligned(16))) float lds[2 * DK * PITCH];
  float* As = lds;
  float* Bs = lds + DK * PITCH;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = blockIdx.x * TILE;
  const int t0 = blockIdx.y * tps, t1 = min(t0 + tps, col_tiles);
  float best[KMAX];
#pragma unroll
  for (int s = 0; s < KMAX; ++s) best[s] = INFINITY;
  int count = 0;

  for (int t = t0; t < t1; ++t) {
    const int col0 = t * TILE;
    f32x2 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = f32x2{0.f, 0.f};
    float ra[8], rb[8];
    fetch_chunk(a, row0, M, 0, D, ra);
    fetch_chunk(b, col0, N, 0, D, rb);
    for (int d0 = 0; d0 < D; d0 += DK) {
      __syncthreads();      // the previous chunk, or the previous tile's distances, are consumed
      stage_chunk(As, ra);
      stage_chunk(Bs, rb);
      __syncthreads();
      if (d0 + DK < D) {
        fetch_chunk(a, row0, M, d0 + DK, D, ra);
        fetch_chunk(b, col0, N, d0 + DK, D, rb);
      }
#pragma unroll
      for (int k = 0; k < DK; ++k) {
        const f32x4 av = *(const f32x4*)(As + k * PITCH + 4 * ty);
        const f32x4 bv = *(const f32x4*)(Bs + k * PITCH + 4 * tx);
        const f32x2 b01 = {bv[0], bv[1]}, b23 = {bv[2], bv[3]};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x2 ai = {av[i], av[i]};
          const f32x2 u = ai - b01, w = ai - b23;
          acc[i][0] = __builtin_elementwise_fma(u, u, acc[i][0]);
          acc[i][1] = __builtin_elementwise_fma(w, w, acc[i][1]);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float* row = lds + (4 * ty + i) * DPITCH + 4 * tx;
      row[0] = acc[i][0][0];
      row[1] = acc[i][0][1];
      row[2] = acc[i][1][0];
      row[3] = acc[i][1][1];
    }
    __syncthreads();
    if (tid < TILE) {
      const int gi = row0 + tid, cols = min(TILE, N - col0);
      const float* row = lds + tid * DPITCH;
      for (int c = 0; c < cols; ++c) {
        const float x = row[c];
        const bool take = !(exclude_self && col0 + c == gi);      // by index: a duplicate row elsewhere still counts
        if constexpr (HITS) {
          count += (take && x <= thr[col0 + c]) ? 1 : 0;
        } else {
          knn_insert(best, take ? x : INFINITY);
        }
      }
    }
  }
  if (tid < TILE) {
    const size_t slot = (size_t)blockIdx.y * Mpad + row0 + tid;      // rows past M: padding of the workspace
    if constexpr (HITS) {
      ((int*)partial)[slot] = count;
    } else {
#pragma unroll
      for (int s = 0; s < KMAX; ++s)
        if (s < K) ((float*)partial)[slot * K + s] = best[s];
    }
  }
}

__global__ __launch_bounds__(256) void pair_merge_knn_kernel(const float* __restrict__ partial, float* __restrict__ out, int M,
                                                             int K, int splits, size_t Mpad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  float best[KMAX];
#pragma unroll
  for (int s = 0; s < KMAX; ++s) best[s] = INFINITY;
  for (int k = 0; k < splits; ++k) {
    const float* p = partial + ((size_t)k * Mpad + i) * K;
    for (int s = 0; s < K; ++s) knn_insert(best, p[s]);
  }
#pragma unroll
  for (int s = 0; s < KMAX; ++s)
    if (s < K) out[(size_t)i * K + s] = best[s];
}

__global__ __launch_bounds__(256) void pair_merge_hits_kernel(const int* __restrict__ partial, int* __restrict__ count, int M,
                                                              int splits, size_t Mpad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  int c = 0;
  for (int k = 0; k < splits; ++k) c += partial[(size_t)k * Mpad + i];
  count[i] = c;
}

}  // namespace

extern "C" int vg_pair_splits(int M, int N, int D, int splits) {
  return dims_ok(M, N, D, 1, splits) ? make_plan(M, N, 1, splits).splits : 0;
}

extern "C" size_t vg_pair_workspace_bytes(int M, int N, int D, int K, int splits) {
  return dims_ok(M, N, D, K, splits) ? make_plan(M, N, K, splits).bytes : 0;
}

extern "C" int vg_pair_knn(const float* a, const float* b, int exclude_self, float* out, int M, int N, int D, int K,
                           int splits, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a || !b || !out || !workspace || !dims_ok(M, N, D, K, splits)) return VG_ERR_BAD_ARG;
  if (exclude_self != 0 && (exclude_self != 1 || a != b || M != N)) return VG_ERR_BAD_ARG;
  if (((uintptr_t)workspace & 255u) != 0) return VG_ERR_BAD_ARG;
  const Plan p = make_plan(M, N, K, splits);
  if (workspace_bytes < p.bytes) return VG_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pair_kernel<false>, dim3(p.row_blocks, p.splits), dim3(NT), 0, st, a, b, (const float*)nullptr, workspace,
                     M, N, D, K, exclude_self, p.col_tiles, p.tps, p.Mpad);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(pair_merge_knn_kernel, dim3(cdiv(M, 256)), dim3(256), 0, st, (const float*)workspace, out, M, K,
                     p.splits, p.Mpad);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_pair_hits(const float* a, const float* b, const float* thr, int* count, int M, int N, int D, int splits,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!a || !b || !thr || !count || !workspace || !dims_ok(M, N, D, 1, splits)) return VG_ERR_BAD_ARG;
  if (((uintptr_t)workspace & 255u) != 0) return VG_ERR_BAD_ARG;
  const Plan p = make_plan(M, N, 1, splits);
  if (workspace_bytes < p.bytes) return VG_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pair_kernel<true>, dim3(p.row_blocks, p.splits), dim3(NT), 0, st, a, b, thr, workspace, M, N, D, 1, 0,
                     p.col_tiles, p.tps, p.Mpad);
  VG_CHECK_LAUNCH();
  hipLaunchKernelGGL(pair_merge_hits_kernel, dim3(cdiv(M, 256)), dim3(256), 0, st, (const int*)workspace, count, M, p.splits,
                     p.Mpad);
  VG_CHECK_LAUNCH();
  return 0;
}
