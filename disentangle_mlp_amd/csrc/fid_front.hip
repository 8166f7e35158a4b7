// From the decoder's output to the FID Inception network and through its pooling layers, for gfx950: the four
// streaming kernels (HBM / L2 bound, no MFMA) that keep the FID path on the device between the generator and the
// Frechet arithmetic ("FID on the device").
//
//   vg_quantize_each_u8    save_image(x[i], normalize=True) for every image of a batch at once: the per-image
//       min / max, then the arithmetic of image_grid_u8_kernel (data.hip) in the same operation order -- bit-identical
//       to vg_minmax + vg_image_grid_u8 on each image alone.
//   vg_resize_bilinear_u8  F.interpolate(img / 255, (OH, OW), "bilinear", align_corners=False) of a uint8 HWC batch
//       into fp32 NCHW, times scale plus shift (normalize_input: 2, -1), with max |y| for the first convolution.
//   vg_pool3x3             the three 3x3 poolings of the FID Inception (max s2 p0, max s1 p1, average s1 p1 that does
//       not count the padding) into a channel slice of a block's concatenated output, with max |out|.
//   vg_global_avg_pool     adaptive_avg_pool2d(x, (1, 1)): one wavefront per (b, c), fixed summation order.
//
// Every kernel is correct for any base alignment and any width; 16-byte accesses are taken where the addresses allow
// and where they were not measured slower (the pooling).
#include "common.hpp"
#include "vaegan_hip.h"

namespace {

constexpr int NT = 256;

// ---- per-image min / max: one workgroup per image -> mm[2 b], mm[2 b + 1] (exact in any order)
__global__ __launch_bounds__(NT) void minmax_each_kernel(const float* __restrict__ x, int n, float* __restrict__ mm) {
  __shared__ float red[2][NT / 64];
  const float* xb = x + (size_t)blockIdx.x * n;
  float lo = INFINITY, hi = -INFINITY;
  if (((uintptr_t)xb & 15) == 0) {
    const int n4 = n / 4;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(xb);
    for (int i = threadIdx.x; i < n4; i += NT) {
      const f32x4 a = x4[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) { lo = fminf(lo, a[e]); hi = fmaxf(hi, a[e]); }
    }
    for (int i = n4 * 4 + threadIdx.x; i < n; i += NT) { lo = fminf(lo, xb[i]); hi = fmaxf(hi, xb[i]); }
  } else {
    for (int i = threadIdx.x; i < n; i += NT) { lo = fminf(lo, xb[i]); hi = fmaxf(hi, xb[i]); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_down(lo, o, 64));
    hi = fmaxf(hi, __shfl_down(hi, o, 64));
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { red[0][wid] = lo; red[1][wid] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) { lo = fminf(lo, red[0][i]); hi = fmaxf(hi, red[1][i]); }
    mm[2 * blockIdx.x] = lo;
    mm[2 * blockIdx.x + 1] = hi;
  }
}

// the arithmetic of image_grid_u8_kernel (data.hip), operation for operation
__device__ __forceinline__ uint8_t quantize_one(float v, float lo, float hi, float den) {
  v = (fminf(fmaxf(v, lo), hi) + (-lo)) / den;
  v = fminf(fmaxf(v * 255.0f, 0.f), 255.0f);
  return (uint8_t)v;
}

// VEC: 4 consecutive pixels per thread -- one 16-byte load per channel plane, 12 contiguous bytes out (HW % 4 == 0,
// x 16-byte and out 4-byte aligned); otherwise one pixel per thread
template <bool VEC>
__global__ __launch_bounds__(NT) void quantize_each_kernel(const float* __restrict__ x, const float* __restrict__ mm,
                                                          uint8_t* __restrict__ out, int C, int HW) {
  const int b = blockIdx.y;
  const float lo = mm[2 * b], hi = mm[2 * b + 1];
  const float den = (float)((double)hi - (double)lo + 1e-5);   // python: max - min + 1e-5, then an fp32 divide
  const float* xb = x + (size_t)b * C * HW;
  uint8_t* ob = out + (size_t)b * HW * 3;
  const int t = blockIdx.x * NT + threadIdx.x;
  if constexpr (VEC) {
    if (t * 4 >= HW) return;
    uint8_t px[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xb + (size_t)(C == 1 ? 0 : c) * HW + (size_t)t * 4);
#pragma unroll
      for (int p = 0; p < 4; ++p) px[p * 3 + c] = quantize_one(v[p], lo, hi, den);
    }
    uint32_t* o32 = reinterpret_cast<uint32_t*>(ob + (size_t)t * 12);
#pragma unroll
    for (int w = 0; w < 3; ++w)
      o32[w] = (uint32_t)px[4 * w] | ((uint32_t)px[4 * w + 1] << 8) | ((uint32_t)px[4 * w + 2] << 16) |
               ((uint32_t)px[4 * w + 3] << 24);
  } else {
    if (t >= HW) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) ob[(size_t)t * 3 + c] = quantize_one(xb[(size_t)(C == 1 ? 0 : c) * HW + t], lo, hi, den);
  }
}

// ---- bilinear resize of uint8 HWC into fp32 NCHW.  One thread per output pixel and all three channels: the four
// neighbours' 3 bytes each are read once, the three plane stores are consecutive over the lanes (the planes of a
// 299 x 299 output start at odd offsets: no 16-byte store fits).  ATen's align_corners=False rule in fp32:
// src = max(0, (o + 0.5) * (in / out) - 0.5), upper neighbour clamped to in - 1, weights (1 - l, l).
__device__ __forceinline__ void source_index(int o, float ratio, int in, int& i0, int& i1, float& l1) {
  const float s = fmaxf(ratio * ((float)o + 0.5f) - 0.5f, 0.f);
  i0 = min((int)s, in - 1);
  i1 = min(i0 + 1, in - 1);
  l1 = s - (float)i0;
}

__global__ __launch_bounds__(NT) void resize_bilinear_u8_kernel(const uint8_t* __restrict__ img, float* __restrict__ y,
                                                               int H, int W, int OH, int OW, float rh, float rw,
                                                               float scale, float shift, unsigned* __restrict__ amax) {
  const int b = blockIdx.y;
  const int e = blockIdx.x * NT + threadIdx.x;
  const int OHW = OH * OW;
  unsigned m = 0;
  if (e < OHW) {
    const int oy = e / OW, ox = e - oy * OW;
    int y0, y1, x0, x1;
    float ly, lx;
    source_index(oy, rh, H, y0, y1, ly);
    source_index(ox, rw, W, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const uint8_t* ib = img + (size_t)b * H * W * 3;
    const uint8_t* p00 = ib + ((size_t)y0 * W + x0) * 3;
    const uint8_t* p01 = ib + ((size_t)y0 * W + x1) * 3;
    const uint8_t* p10 = ib + ((size_t)y1 * W + x0) * 3;
    const uint8_t* p11 = ib + ((size_t)y1 * W + x1) * 3;
    float* yb = y + (size_t)b * 3 * OHW + e;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = (float)p00[c] / 255.0f, bb = (float)p01[c] / 255.0f;
      const float cc = (float)p10[c] / 255.0f, d = (float)p11[c] / 255.0f;
      const float v = hy * (hx * a + lx * bb) + ly * (hx * cc + lx * d);
      const float r = scale * v + shift;
      yb[(size_t)c * OHW] = r;
      m = max(m, abs_bits(r));
    }
  }
  if (amax) block_amax_atomic<NT>(m, amax);
}

// ---- 3x3 pooling.  The channels [offset, offset + C) of image b of `out` are one contiguous run of C * OH * OW floats:
// one thread per element of that run, so that the lanes of a wavefront read consecutive addresses for each of the 9
// taps (which overlap between neighbours and come from the L1 / L2) and store 256 contiguous bytes.  Four elements per
// thread with one 16-byte store was measured 1.5 x slower than ATen's one-per-thread kernels on the Inception shapes:
// every load instruction then touches four times the cache lines.  AVG = false: maximum, padding reads as -inf (taps
// outside the image are skipped), a NaN wins as in torch; AVG = true: sum of the taps inside the image in (h, w) order
// over their count.
template <bool AVG>
__device__ __forceinline__ float pool_one(const float* __restrict__ xc, int H, int W, int oy, int ox, int stride, int pad) {
  const int h0 = oy * stride - pad, w0 = ox * stride - pad;
  float acc = AVG ? 0.f : -INFINITY;
  int cnt = 0;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int h = h0 + kh;
    if (h < 0 || h >= H) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int w = w0 + kw;
      if (w < 0 || w >= W) continue;
      const float v = xc[(size_t)h * W + w];
      if constexpr (AVG) {
        acc += v;
        ++cnt;
      } else {
        if (v > acc || v != v) acc = v;
      }
    }
  }
  return AVG ? acc / (float)cnt : acc;
}

template <bool AVG>
__global__ __launch_bounds__(NT) void pool3x3_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H,
                                                    int W, int OH, int OW, int stride, int pad, size_t out_image_stride,
                                                    unsigned* __restrict__ amax) {
  const int b = blockIdx.y;
  const int OHW = OH * OW, n = C * OHW;
  const int e = blockIdx.x * NT + threadIdx.x;
  unsigned m = 0;
  if (e < n) {
    const int c = e / OHW, r = e - c * OHW;
    const int oy = r / OW, ox = r - oy * OW;
    const float v = pool_one<AVG>(x + ((size_t)b * C + c) * H * W, H, W, oy, ox, stride, pad);
    out[(size_t)b * out_image_stride + e] = v;
    m = abs_bits(v);
  }
  if (amax) block_amax_atomic<NT>(m, amax);
}

// ---- mean over HW of every (b, c) row: one wavefront per row.  Lane l sums the quads l, l + 64, ... of its row,
// element by element, then the 64 lanes are summed by the shuffle tree: the order depends on HW alone, not on the
// alignment (an unaligned row reads the same quads with scalar loads).
__global__ __launch_bounds__(NT) void global_avg_pool_kernel(const float* __restrict__ x, float* __restrict__ y, int rows,
                                                            int HW) {
  const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;                       // whole wavefronts leave together
  const float* xr = x + (size_t)row * HW;
  const bool vec = ((uintptr_t)xr & 15) == 0;
  float acc = 0.f;
  for (int q = lane; q * 4 < HW; q += 64) {
    const int i = q * 4;
    if (vec && i + 4 <= HW) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(xr + i);
      acc += a[0]; acc += a[1]; acc += a[2]; acc += a[3];
    } else {
      for (int j = i; j < min(i + 4, HW); ++j) acc += xr[j];
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) y[row] = acc / (float)HW;
}

}  // namespace

extern "C" int vg_quantize_each_u8(const float* x, uint8_t* out, int B, int C, int H, int W, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!x || !out || B <= 0 || B > 65535 || (C != 1 && C != 3) || H <= 0 || W <= 0) return VG_ERR_BAD_ARG;
  if ((long)H * W * 3 > 0x7fffffffL) return VG_ERR_BAD_ARG;
  if (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < (size_t)B * 2 * sizeof(float)) return VG_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  float* mm = (float*)workspace;
  hipLaunchKernelGGL(minmax_each_kernel, dim3(B), dim3(NT), 0, st, x, C * HW, mm);
  VG_CHECK_LAUNCH();
  if ((HW & 3) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 3) == 0) {
    hipLaunchKernelGGL(quantize_each_kernel<true>, dim3(cdiv(HW / 4, NT), B), dim3(NT), 0, st, x, mm, out, C, HW);
  } else {
    hipLaunchKernelGGL(quantize_each_kernel<false>, dim3(cdiv(HW, NT), B), dim3(NT), 0, st, x, mm, out, C, HW);
  }
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_resize_bilinear_u8(const uint8_t* img, float* y, int B, int H, int W, int OH, int OW, float scale,
                                     float shift, float* amax, void* stream) {
  if (!img || !y || B <= 0 || B > 65535 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return VG_ERR_BAD_ARG;
  if ((long)H * W * 3 > 0x7fffffffL || (long)OH * OW * 3 > 0x7fffffffL) return VG_ERR_BAD_ARG;
  hipLaunchKernelGGL(resize_bilinear_u8_kernel, dim3(cdiv(OH * OW, NT), B), dim3(NT), 0, (hipStream_t)stream, img, y, H, W,
                     OH, OW, (float)H / (float)OH, (float)W / (float)OW, scale, shift, (unsigned*)amax);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_pool3x3(const float* x, float* out, int B, int C, int H, int W, int stride, int pad, int mode,
                          int out_channels_total, int out_channel_offset, float* amax, void* stream) {
  if (!x || !out || B <= 0 || B > 65535 || C <= 0 || H <= 0 || W <= 0) return VG_ERR_BAD_ARG;
  if ((stride != 1 && stride != 2) || (pad != 0 && pad != 1) || (mode != VG_POOL_MAX && mode != VG_POOL_AVG_EXCLUDE_PAD))
    return VG_ERR_BAD_ARG;
  if (H + 2 * pad < 3 || W + 2 * pad < 3) return VG_ERR_BAD_ARG;
  if (out_channel_offset < 0 || (long)out_channel_offset + C > out_channels_total) return VG_ERR_BAD_ARG;
  const int OH = (H + 2 * pad - 3) / stride + 1, OW = (W + 2 * pad - 3) / stride + 1;
  if ((long)C * H * W > 0x7fffffffL || (long)C * OH * OW > 0x7fffffffL - NT) return VG_ERR_BAD_ARG;
  const size_t image = (size_t)out_channels_total * OH * OW;
  float* o = out + (size_t)out_channel_offset * OH * OW;
  const dim3 grid(cdiv(C * OH * OW, NT), B);
  hipStream_t st = (hipStream_t)stream;
  if (mode == VG_POOL_MAX)
    hipLaunchKernelGGL(pool3x3_kernel<false>, grid, dim3(NT), 0, st, x, o, C, H, W, OH, OW, stride, pad, image, (unsigned*)amax);
  else
    hipLaunchKernelGGL(pool3x3_kernel<true>, grid, dim3(NT), 0, st, x, o, C, H, W, OH, OW, stride, pad, image, (unsigned*)amax);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_global_avg_pool(const float* x, float* y, int B, int C, int HW, void* stream) {
  if (!x || !y || B <= 0 || C <= 0 || HW <= 0 || (long)B * C > 0x7fffffffL - NT) return VG_ERR_BAD_ARG;
  const int rows = B * C;
  hipLaunchKernelGGL(global_avg_pool_kernel, dim3(cdiv(rows, NT / 64)), dim3(NT), 0, (hipStream_t)stream, x, y, rows, HW);
  VG_CHECK_LAUNCH();
  return 0;
}
