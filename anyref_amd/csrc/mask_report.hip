// Mask reports (the rule: anyref_amd/maskreport.py): area, box, stability counts and the bit-packed mask of
// f32 mask logits in one integer pass.
#include "mask_report.h"

#include <algorithm>
#include <cmath>

#include "common.h"

namespace {
constexpr int MR_THREADS = 512;    // 8 waves
constexpr int MR_UNROLL = 4;       // 64-pixel units a wave has in flight per step
constexpr int MR_MAX_BLOCKS = 256; // per mask: the records take one atomic pair per workgroup

// A unit is 64 consecutive pixels of one row (the last unit of a row may be short); a wave takes MR_UNROLL consecutive units per
// step and strides over the mask by the grid.  The ballot of x > 0 over a unit is its two packed words, and the source of the
// count and of the box edges; everything a wave accumulates is wave-uniform.  While the kernel runs the box is held as
// {W - x0, H - y0, x1 + 1, y1 + 1}, so that a record of zeros updated by add and max only is right in any order of arrival;
// mask_report_finish_kernel turns it into x0, y0, x1, y1.
__global__ __launch_bounds__(MR_THREADS) void mask_report_kernel(const float* __restrict__ logits, int H, int W, float d,
                                                                 int32_t* __restrict__ records,
                                                                 uint32_t* __restrict__ packed) {
  const int m = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned Cw = ((unsigned)W + 63u) >> 6, Wp = ((unsigned)W + 31u) >> 5;
  const unsigned units = (unsigned)H * Cw;  // <= H * W <= INT32_MAX
  const float* x = logits + (int64_t)m * H * W;
  uint32_t* pk = packed ? packed + (int64_t)m * H * Wp : nullptr;
  const float nd = -d;
  unsigned area = 0, hi = 0, lo = 0, nf = 0;
  int bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
  const unsigned stride = gridDim.x * (MR_THREADS / 64) * MR_UNROLL;
  for (unsigned u0 = (blockIdx.x * (MR_THREADS / 64) + wave) * MR_UNROLL; u0 < units; u0 += stride) {
    float v[MR_UNROLL];
    bool ok[MR_UNROLL];
    unsigned row[MR_UNROLL], col[MR_UNROLL];
#pragma unroll
    for (int k = 0; k < MR_UNROLL; ++k) {
      const unsigned u = u0 + k;
      row[k] = u / Cw;
      col[k] = (u - row[k] * Cw) * 64u;
      const unsigned px = col[k] + lane;
      ok[k] = u < units && px < (unsigned)W;  // tail lanes and tail units contribute nothing
      v[k] = ok[k] ? x[(int64_t)row[k] * W + px] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < MR_UNROLL; ++k) {
      const bool fin = (__float_as_uint(v[k]) & 0x7f800000u) != 0x7f800000u;
      const unsigned long long b = __ballot(ok[k] && v[k] > 0.f);
      hi += __popcll(__ballot(ok[k] && v[k] > d));
      lo += __popcll(__ballot(ok[k] && v[k] > nd));
      nf += __popcll(__ballot(ok[k] && !fin));
      area += __popcll(b);
      if (b) {
        const int first = (int)col[k] + __ffsll(b) - 1, last = (int)col[k] + 63 - __clzll(b);
        bx0 = max(bx0, W - first);
        bx1 = max(bx1, last + 1);
        by0 = max(by0, H - (int)row[k]);
        by1 = max(by1, (int)row[k] + 1);
      }
      if (pk && u0 + k < units && lane < 2) {  // two 4-byte stores: the word pitch may be odd
        const unsigned w = (col[k] >> 5) + lane;
        if (w < Wp) pk[(int64_t)row[k] * Wp + w] = lane == 0 ? (uint32_t)b : (uint32_t)(b >> 32);
      }
    }
  }
  __shared__ int red[MR_THREADS / 64][8];
  if (lane == 0) {
    red[wave][0] = (int)area; red[wave][1] = (int)hi; red[wave][2] = (int)lo; red[wave][3] = (int)nf;
    red[wave][4] = bx0; red[wave][5] = by0; red[wave][6] = bx1; red[wave][7] = by1;
  }
  __syncthreads();
  if (threadIdx.x < 8) {  // integer add and max: the result does not depend on the order of arrival
    const int t = threadIdx.x;
    int r = red[0][t];
#pragma unroll
    for (int w = 1; w < MR_THREADS / 64; ++w) r = t < 4 ? r + red[w][t] : max(r, red[w][t]);
    if (r) {
      if (t < 4) atomicAdd(&records[m * 8 + t], r);
      else atomicMax(&records[m * 8 + t], r);
    }
  }
}

__global__ void mask_report_finish_kernel(int n, int H, int W, int32_t* __restrict__ records) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 2) return;
  int32_t* r = records + (i >> 1) * 8;
  if (r[0] == 0) return;  // empty: the box stays 0, 0, 0, 0
  if (i & 1) {
    r[6] -= 1;
    r[7] -= 1;
  } else {
    r[4] = W - r[4];
    r[5] = H - r[5];
  }
}
}  // namespace

void launch_mask_report(const float* logits, int n, int H, int W, float offset, int32_t* records, uint32_t* packed,
                        hipStream_t s) {
  if (n <= 0) return;
  if (!logits || !records) throw std::runtime_error("mask_report: null logits / records");
  if (H < 1 || W < 1 || (int64_t)H * W > INT32_MAX) throw std::runtime_error("mask_report: H, W >= 1 and H * W <= INT32_MAX");
  if (n > 65535) throw std::runtime_error("mask_report: at most 65535 masks per launch");
  if (!(offset >= 0.f) || !std::isfinite(offset)) throw std::runtime_error("mask_report: the offset must be finite and >= 0");
  HIP_TRY(hipMemsetAsync(records, 0, (size_t)n * 8 * sizeof(int32_t), s));
  const int64_t units = (int64_t)H * (((int64_t)W + 63) / 64), per_block = (MR_THREADS / 64) * MR_UNROLL;
  const int64_t blocks = std::min<int64_t>((units + per_block - 1) / per_block, MR_MAX_BLOCKS);
  hipLaunchKernelGGL(mask_report_kernel, dim3((unsigned)blocks, n), dim3(MR_THREADS), 0, s, logits, H, W, offset, records,
                     packed);
  hipLaunchKernelGGL(mask_report_finish_kernel, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, s, n, H, W, records);
}
