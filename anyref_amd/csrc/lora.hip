// Adapter hot-swap (anyref_adapter_apply): the LoRA merge W' = W + scaling * B A written straight into a packed
// weight buffer, from the f32 base a reserving handle kept.  The rule (anyref_amd/lora.py states it in torch; the tests hold
// the bits against it), per element:
//   acc = 0 (f64);  j = 0 .. r-1 in order: acc = fma(f64(B[n,j]), f64(A[j,k]), acc)   -- the product of two f32 is exact in f64,
//                                                                                        so fma and mul-then-add agree
//   m = f32(acc * f64(scaling) + f64(w))     one f64 multiply, one f64 add (NOT contracted), one RNE
//   m = f32(d_in(m))                         the dtype the base was handed to anyref_set_weight in
//   stored = W(m)                            RNE, exactly what convert_kernel stores at finalize
// r = 0 stores W(w): the base as finalize converted it (a -0 stays -0).
//
// A thread owns 8 consecutive k of a row (16-byte loads of the base and of A, one 16-byte store of 8 16-bit weights or two of
// f32) and walks rows with them.  r <= 8: its 8 columns of A stay in registers across the rows (16 would take all 256 VGPRs: 1 wave per SIMD).  r <= 64: the block's
// columns of A are staged in LDS once (r x 128 f32 = 32 KB at r = 64).  Pad columns [K, ld) of the destination are never
// written; row_stride 2 writes every second row (the gate / up interleave).  Vector stores only.
#include <algorithm>
#include <string>

#include "../../include/anyref_hip.h"
#include "common.h"
#include "kernels.h"

namespace anyref {

namespace {

constexpr int kLoraRegRank = 8;    // largest rank whose A columns are kept in registers
constexpr int kLoraLdsCols = 128;  // columns of A a block of the LDS form stages

__device__ inline float lora_finish(double acc, double s, float w, int d_in) {
#pragma clang fp contract(off)
  const double p = acc * s;
  float m = (float)(p + (double)w);
  if (d_in == ANYREF_BF16) m = bf2f(f2bf(m));
  else if (d_in == ANYREF_F16) m = h2f(f2h(m));
  return m;
}

template <typename W>
__device__ inline void lora_store8(W* p, const float* m) {
  if constexpr (sizeof(W) == 4) {
    float4v* o = reinterpret_cast<float4v*>(p);
    o[0] = float4v{m[0], m[1], m[2], m[3]};
    o[1] = float4v{m[4], m[5], m[6], m[7]};
  } else {
    *reinterpret_cast<uint4v*>(p) = uint4v{pack2_from_f32<W>(m[0], m[1]), pack2_from_f32<W>(m[2], m[3]),
                                           pack2_from_f32<W>(m[4], m[5]), pack2_from_f32<W>(m[6], m[7])};
  }
}

}  // namespace

// counts (optional): [0] += elements with float(W(m)) != m, [1] += finite m stored as inf (f16 past +-65504)
template <typename W, bool LDS>
__global__ __launch_bounds__(256) void lora_merge_rows_kernel(const float* __restrict__ base, int d_in, int N, int K,
                                                              const float* __restrict__ A, const float* __restrict__ B, int r,
                                                              float scaling, W* __restrict__ dst, int64_t row_pitch, int vec,
                                                              unsigned long long* __restrict__ counts) {
  constexpr int CX = LDS ? kLoraLdsCols / 8 : 64;  // threads along k (8 columns each)
  constexpr int RY = 256 / CX;                     // rows a block works on at once
  const int tx = threadIdx.x % CX, ty = threadIdx.x / CX;
  const int k0 = (blockIdx.x * CX + tx) * 8;       // first column of this thread
  const int nk = k0 < K ? (K - k0 < 8 ? K - k0 : 8) : 0;
  const bool full = vec && nk == 8;

  extern __shared__ float sA[];  // LDS form: [r][kLoraLdsCols]
  float a[LDS ? 1 : kLoraRegRank][8];
  if constexpr (LDS) {
    const int c0 = blockIdx.x * kLoraLdsCols;
    for (int i = threadIdx.x; i < r * kLoraLdsCols; i += 256) {
      const int j = i / kLoraLdsCols, c = i % kLoraLdsCols;
      sA[i] = c0 + c < K ? A[(int64_t)j * K + c0 + c] : 0.f;
    }
    __syncthreads();
  } else {
#pragma unroll
    for (int j = 0; j < kLoraRegRank; ++j) {
      if (j < r) {
        const float* ap = A + (int64_t)j * K + k0;
        if (full) {
          const float4v lo = *reinterpret_cast<const float4v*>(ap), hi = *reinterpret_cast<const float4v*>(ap + 4);
          a[j][0] = lo[0]; a[j][1] = lo[1]; a[j][2] = lo[2]; a[j][3] = lo[3];
          a[j][4] = hi[0]; a[j][5] = hi[1]; a[j][6] = hi[2]; a[j][7] = hi[3];
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) a[j][e] = e < nk ? ap[e] : 0.f;
        }
      }
    }
  }

  const double s = (double)scaling;
  unsigned inexact = 0, overflow = 0;
  for (int n = blockIdx.y * RY + ty; n < N && nk > 0; n += gridDim.y * RY) {
    const float* wp = base + (int64_t)n * K + k0;
    float w[8];
    if (full) {
      const float4v lo = *reinterpret_cast<const float4v*>(wp), hi = *reinterpret_cast<const float4v*>(wp + 4);
      w[0] = lo[0]; w[1] = lo[1]; w[2] = lo[2]; w[3] = lo[3];
      w[4] = hi[0]; w[5] = hi[1]; w[6] = hi[2]; w[7] = hi[3];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = e < nk ? wp[e] : 0.f;
    }
    float m[8];
    if (r == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = w[e];
    } else {
      double acc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = 0.0;
      const float* bp = B + (int64_t)n * r;
      if constexpr (LDS) {
        for (int j = 0; j < r; ++j) {
          const double b = (double)bp[j];
          const float4v lo = *reinterpret_cast<const float4v*>(sA + j * kLoraLdsCols + tx * 8);
          const float4v hi = *reinterpret_cast<const float4v*>(sA + j * kLoraLdsCols + tx * 8 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[e] = __builtin_fma(b, (double)lo[e], acc[e]);
            acc[e + 4] = __builtin_fma(b, (double)hi[e], acc[e + 4]);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < kLoraRegRank; ++j) {
          if (j < r) {
            const double b = (double)bp[j];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = __builtin_fma(b, (double)a[j][e], acc[e]);
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = lora_finish(acc[e], s, w[e], d_in);
    }
    W* op = dst + (int64_t)n * row_pitch + k0;
    if (full) {
      lora_store8<W>(op, m);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < nk) op[e] = from_f32<W>(m[e]);
    }
    if constexpr (sizeof(W) == 2) {
      if (counts) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (e < nk) {
            const float y = to_f32<W>(from_f32<W>(m[e]));
            inexact += (y != m[e] && !(__builtin_isnan(m[e]) && __builtin_isnan(y))) ? 1u : 0u;
            overflow += (__builtin_isfinite(m[e]) && !__builtin_isfinite(y)) ? 1u : 0u;
          }
        }
      }
    }
  }
  if constexpr (sizeof(W) == 2) {
    if (!counts) return;
    const float fi = wave_sum((float)inexact), fo = wave_sum((float)overflow);  // <= 64 * 8 * rows per lane: exact in f32
    if ((threadIdx.x & 63) == 0) {
      if (fi > 0.f) atomicAdd(&counts[0], (unsigned long long)fi);
      if (fo > 0.f) atomicAdd(&counts[1], (unsigned long long)fo);
    }
  }
}

template <typename W>
void launch_lora_merge(const float* base, int d_in, int N, int K, const float* A, const float* B, int r, float scaling,
                       void* dst, int64_t ld, int row_stride, unsigned long long* counts, hipStream_t s, const char* name) {
  const std::string who = name && *name ? name : "lora_merge";
  if (r < 0 || r > 64) throw std::runtime_error(who + ": LoRA rank " + std::to_string(r) + " is outside 1 .. 64");
  if (N <= 0 || K <= 0) return;
  if (!base || !dst || (r > 0 && (!A || !B))) throw std::runtime_error(who + ": null tensor");
  if (ld < K) throw std::runtime_error(who + ": destination rows are shorter than K");
  if (row_stride != 1 && row_stride != 2) throw std::runtime_error(who + ": destination row stride must be 1 or 2");
  if (d_in != ANYREF_F32 && d_in != ANYREF_BF16 && d_in != ANYREF_F16) throw std::runtime_error(who + ": bad base dtype");
  if (!(scaling == scaling) || scaling - scaling != 0.f) throw std::runtime_error(who + ": scaling is not finite");
  const int64_t pitch = ld * row_stride;
  const uintptr_t al = (uintptr_t)base | (uintptr_t)dst | (uintptr_t)(r > 0 ? A : base);
  const int vec = K % 8 == 0 && (al & 15) == 0 && (pitch * (int64_t)sizeof(W)) % 16 == 0;
  const bool lds = r > kLoraRegRank;
  const int cols = lds ? kLoraLdsCols : 512, rows = lds ? 256 / (kLoraLdsCols / 8) : 4;
  const int gx = cdiv(K, cols);
  const int gy = std::max(1, std::min(cdiv(N, rows), 1024 / gx));
  W* d = reinterpret_cast<W*>(dst);
  if (lds)
    hipLaunchKernelGGL((lora_merge_rows_kernel<W, true>), dim3(gx, gy), dim3(256), (size_t)r * kLoraLdsCols * sizeof(float), s,
                       base, d_in, N, K, A, B, r, scaling, d, pitch, vec, counts);
  else
    hipLaunchKernelGGL((lora_merge_rows_kernel<W, false>), dim3(gx, gy), dim3(256), 0, s, base, d_in, N, K, A, B, r, scaling,
                       d, pitch, vec, counts);
}
template void launch_lora_merge<float>(const float*, int, int, int, const float*, const float*, int, float, void*, int64_t, int,
                                       unsigned long long*, hipStream_t, const char*);
template void launch_lora_merge<bf16>(const float*, int, int, int, const float*, const float*, int, float, void*, int64_t, int,
                                      unsigned long long*, hipStream_t, const char*);
template void launch_lora_merge<f16>(const float*, int, int, int, const float*, const float*, int, float, void*, int64_t, int,
                                     unsigned long long*, hipStream_t, const char*);

}  // namespace anyref
