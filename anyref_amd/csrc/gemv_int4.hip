// int4 group-quantised weights (ANYREF_MODE_PERF_INT4W): the finalize quantiser, the bf16 image for the prefill GEMM
// and the decode GEMV.  A translation unit of its own, so that it compiles (and is iterated on) beside gemv.hip.
//
// Format (anyref_amd/quant.py is the authority): per output row, groups of 128 consecutive k (the last may be short and is
// padded with zeros in storage); s = max|w| / 7 rounded UP to 5 significant bits (a bf16 with three zero low mantissa bits;
// 1 for a group below 2^-100), q = clamp(rne(w / s), -7, 7).  |q| <= 7 has 3 significant bits, so q * s is EXACTLY a bf16:
// the GEMV's sum_g s_g sum_k q_k x_k, the prefill GEMM on the bf16 image and an oracle run on q * s all see one set of weights.
//
// Storage: nibbles [N, ceil(K / 128) * 64 bytes (+ row pad)], scales bf16 [N, ceil(K / 128)].  A nibble holds q + 8 (1 .. 15).
// A 16-byte block is 32 consecutive weights of ONE group, as four dwords of 8; inside dword d, nibble i (i < 4) is weight
// 8 d + 2 i and nibble 4 + i is weight 8 d + 2 i + 1, so that ((dword >> 4 i) & 0x000F000F) | 0x43004300 is the packed bf16
// pair (136 + q[8 d + 2 i], 136 + q[8 d + 2 i + 1]) in one instruction (0x4300 = 128.0, whose ulp is 1), ready for
// v_dot2c_f32_bf16 against the packed pair x[8 d + 2 i], x[8 d + 2 i + 1].
#include <cstdlib>
#include <stdexcept>
#include <type_traits>

#include "gemv_common.h"

namespace anyref {

constexpr int I4_GROUP = 128;   // weights per scale
constexpr int I4_BLOCK = 32;    // weights per 16-byte block (one lane's load)
constexpr float I4_BIAS = 136.f;  // 128 (the bf16 exponent that makes a nibble a mantissa) + 8 (the nibble's own offset)

// ---------------------------------------------------------------------------------------------
// Quantiser: one workgroup per row, 16 threads per group (8 weights = one dword each).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quant_int4_rows_kernel(const float* __restrict__ src, int lds, int K,
                                                              uint8_t* __restrict__ q, int ldq, bf16* __restrict__ scale,
                                                              int lds_scale, unsigned long long* __restrict__ inexact) {
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* row = src + (int64_t)n * lds;
  uint32_t* out = reinterpret_cast<uint32_t*>(q + (int64_t)n * ldq);
  const int G = cdiv(K, I4_GROUP);
  unsigned changed = 0;  // elements whose held value q * s differs from the source
  for (int g0 = 0; g0 < G; g0 += 16) {  // (every thread walks every round: the shuffles below take whole waves)
    const int g = g0 + (tid >> 4), k0 = g * I4_GROUP + (tid & 15) * 8;
    float w[8];
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      w[e] = (g < G && k0 + e < K) ? row[k0 + e] : 0.f;
      amax = fmaxf(amax, fabsf(w[e]));
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const bool zero = !(amax >= 0x1p-100f);
    float s = 1.f;
    if (!zero) {
      uint32_t u = __builtin_bit_cast(uint32_t, amax / 7.f);
      const uint32_t low = u & 0x7FFFFu;
      u = (u - low) + (low ? 0x80000u : 0u);  // up to 5 significant bits (a carry runs into the exponent)
      s = __builtin_bit_cast(float, u);
    }
    if (g >= G) continue;
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float r = zero ? 0.f : rintf(w[e] / s);  // f32 division, ties to even
      r = fminf(fmaxf(r, -7.f), 7.f);
      const uint32_t nib = (uint32_t)((int)r + 8);
      word |= nib << (4 * ((e >> 1) + 4 * (e & 1)));
      if (k0 + e < K && r * s != w[e]) ++changed;
    }
    out[g * 16 + (tid & 15)] = word;
    if ((tid & 15) == 0) {
      bf16 sb;
      sb.x = (uint16_t)(__builtin_bit_cast(uint32_t, s) >> 16);  // exact: the low 19 bits are zero
      scale[(int64_t)n * lds_scale + g] = sb;
    }
  }
  if (inexact) {
    const float c = wave_sum((float)changed);  // <= 64 * K / 32: exact in f32
    if ((tid & 63) == 0 && c > 0.f) atomicAdd(inexact, (unsigned long long)c);
  }
}
void launch_quant_int4_rows(const float* src, int lds, int N, int K, uint8_t* q, int ldq, void* scale_bf16, int ld_scale,
                            hipStream_t s, unsigned long long* inexact) {
  if (N <= 0) return;
  if (K % 16 || ldq % 16 || ldq < cdiv(K, I4_GROUP) * 64 || ((uintptr_t)q & 15))
    throw std::runtime_error("quant_int4: K must be a multiple of 16, rows 16-byte aligned and whole groups long");
  hipLaunchKernelGGL(quant_int4_rows_kernel, dim3(N), dim3(256), 0, s, src, lds, K, q, ldq, reinterpret_cast<bf16*>(scale_bf16),
                     ld_scale, inexact);
}

// nibbles + scales -> bf16 [N, K]: a dword (8 weights) per thread step, one 16-byte store.  q * s is exact in f32 and in bf16.
__global__ __launch_bounds__(256) void dequant_int4_rows_kernel(const uint8_t* __restrict__ q, int ldq,
                                                                const bf16* __restrict__ scale, int ld_scale, int N, int K,
                                                                bf16* __restrict__ out, int ldo) {
  const int64_t per_row = K / 8;
  const int64_t total = (int64_t)N * per_row;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / per_row), c = (int)(i % per_row);
    const uint32_t word = *reinterpret_cast<const uint32_t*>(q + (int64_t)n * ldq + c * 4);
    const float s = bf2f(scale[(int64_t)n * ld_scale + c / 16]);
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float lo = (float)((int)((word >> (4 * j)) & 15u) - 8) * s, hi = (float)((int)((word >> (4 * j + 16)) & 15u) - 8) * s;
      w[j] = (uint32_t)f2bf(lo).x | ((uint32_t)f2bf(hi).x << 16);
    }
    *reinterpret_cast<uint4v*>(out + (int64_t)n * ldo + c * 8) = uint4v{w[0], w[1], w[2], w[3]};
  }
}
void launch_dequant_int4_rows(const uint8_t* q, int ldq, const void* scale_bf16, int ld_scale, int N, int K, void* out_bf16,
                              int ldo, hipStream_t s) {
  if (N <= 0) return;
  if (K % 16 || ldq % 16 || ldo % 8 || ((uintptr_t)out_bf16 & 15))
    throw std::runtime_error("dequant_int4: K must be a multiple of 16");
  int64_t blocks = cdiv64((int64_t)N * (K / 8), 256);
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(dequant_int4_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, q, ldq,
                     reinterpret_cast<const bf16*>(scale_bf16), ld_scale, N, K, reinterpret_cast<bf16*>(out_bf16), ldo);
}

// ---------------------------------------------------------------------------------------------
// Decode GEMV on int4 weights.  What it shares with gemv_kernel (gemv.hip) is gemv_common.h's code, not a copy: the work list
// with the wave-pair split, the RMSNorm input stage (x first, the first weight chunk right behind it; xn_out), the row-group
// finish (DUAL gate / up SwiGLU form, bias / act / resid), the stamps, and on the host the grid / wave-pair rules, the K ladder
// and the passes of 1 - 4 batch rows.  Its own: x as bf16 planes + block sums in LDS, and the multiply.  Weights by 16-byte
// non-temporal loads straight to VGPRs, software-pipelined one chunk deep.
//
// A lane's 16 bytes are one BLOCK: 32 weights of one group.  A row of K = 4096 is two wave-loads, K = 11008 is 5.4, so a
// chunk is UNR = 1 .. 4 wave-loads (by K) instead of gemv_kernel's four loads of 512 weights.
// The x stage is laid out for that: plane d (d = 0 .. 3) holds the 16-byte piece d (x[32 blk + 8 d .. + 8) as bf16) of every
// block, so the 64 lanes of a read are 1 KB contiguous; and the stage also keeps xsum[blk] = the f32 sum of the block's 32
// ROUNDED x.  Per load and batch row:  t = -136 xsum;  t += dot2(pair(136 + q), pair(x)) sixteen times;  acc += s t
// -- the nibble pairs are unpacked once per load (16 VALU) and shared by the batch rows.
// Rounding: the products (136 + q) x are exact in f32; the chain is f32 in a fixed order (no atomics): deterministic.
// Positions past K inside the last block meet x = 0 (the stage pads with zeros), whatever the nibbles hold.
// ---------------------------------------------------------------------------------------------
template <int NB, bool DUAL, int XPT, bool PAIR>  // XPT: x elements per thread in the staging, K <= 512 * XPT
__global__ __launch_bounds__(512) void gemv_int4_kernel(GemvArgs a, int b0, int nb) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
  constexpr int R = DUAL ? 1 : 2;  // output rows per wave per pass
  constexpr int RW = 2;            // weight rows streamed per pass (DUAL: gate row + up row)
  // wave-loads (64 blocks = 2048 weights of a row) per chunk: K <= 4096 is one chunk (one per wave of a pair), K <= 12288 two
  // chunks of three, K <= 16384 two chunks of four
  constexpr int UNR = XPT == 8 ? (PAIR ? 1 : 2) : XPT == 24 ? 3 : 4;
  constexpr int CHB = 64 * UNR;  // blocks one wave sweeps per chunk
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float red[NB][8];
  __shared__ float red2[2][4][2][NB];  // PAIR: partial sums of the odd waves, double-buffered over the groups
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, KB = cdiv(K, I4_BLOCK);
  const int row_bytes = KB * 64;               // one batch row's bf16 stage (four planes of KB * 16 bytes)
  float* xsum = reinterpret_cast<float*>(smem + (size_t)NB * row_bytes);  // [NB][KB]
  __shared__ unsigned long long st_t[2];
  __shared__ unsigned st_cnt;
  const unsigned long long t_begin = gemv_stamp_begin(a.stamp, st_t, st_cnt, tid);

  const uint8_t* __restrict__ W = reinterpret_cast<const uint8_t*>(a.W);
  const uint8_t* __restrict__ W2 = reinterpret_cast<const uint8_t*>(a.W2);
  const uint16_t* __restrict__ S = reinterpret_cast<const uint16_t*>(a.gscale);
  const uint16_t* __restrict__ S2 = reinterpret_cast<const uint16_t*>(a.gscale2);
  const int ldw = a.ldw, lgs = a.ld_gscale;  // bytes between nibble rows, scales between scale rows
  const GemvWork<R, PAIR> wk(gridDim.x, blockIdx.x, wave, a.N, cdiv(KB, CHB));
  const int items = wk.items;
  uint4v wcur[UNR][RW], wnxt[UNR][RW];
  uint32_t scur[UNR][RW], snxt[UNR][RW];  // the block's group scale (bf16 bits), loaded beside it
  auto load_item = [&](int t, uint4v (&w)[UNR][RW], uint32_t (&sc)[UNR][RW]) {
    const auto it = wk.item(t);
    const int n0 = it.g * R;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int blk = it.live ? it.c * CHB + u * 64 + lane : KB;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int n = n0 + r < a.N ? n0 + r : a.N - 1;
        w[u][r] = blk < KB ? __builtin_nontemporal_load(reinterpret_cast<const uint4v*>(W + (int64_t)n * ldw + blk * 16))
                           : uint4v{0, 0, 0, 0};
        sc[u][r] = blk < KB ? (uint32_t)S[(int64_t)n * lgs + (blk >> 2)] : 0u;
      }
      if (DUAL) {
        w[u][RW - 1] = blk < KB ? __builtin_nontemporal_load(reinterpret_cast<const uint4v*>(W2 + (int64_t)n0 * ldw + blk * 16))
                                : uint4v{0, 0, 0, 0};
        sc[u][RW - 1] = blk < KB ? (uint32_t)S2[(int64_t)n0 * lgs + (blk >> 2)] : 0u;
      }
    }
  };
  // ---- x stage: x goes FIRST into the (in-order) vector-memory queue, the first weight chunk right behind it ----
  {
    constexpr int XV = (XPT + 3) / 4;  // float4 per thread and row
    GemvNormStage<NB, XV> st;
    if (a.gain) st.load_gain(a, tid);
    st.load_x(a, b0, nb, tid);
    if (items > 0) load_item(0, wcur, scur);
    float scale[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) scale[b] = 1.f;
    if (a.gain) st.scales(a, red, lane, wave, scale);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int i = 0; i < XV; ++i) {
        const int k = (tid + i * 512) * 4;  // eight consecutive lanes hold one block
        const float4v v = a.gain ? st.xr[b][i] * scale[b] * st.gr[i] : st.xr[b][i];  // zeros past K and for rows >= nb
        const bf16 h0 = f2bf(v[0]), h1 = f2bf(v[1]), h2 = f2bf(v[2]), h3 = f2bf(v[3]);
        float sum = (bf2f(h0) + bf2f(h1)) + (bf2f(h2) + bf2f(h3));
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        sum += __shfl_xor(sum, 4, 64);
        const int blk = k >> 5, in = k & 31;
        if (b < nb && blk < KB) {
          char* p = smem + (size_t)b * row_bytes + (size_t)(in >> 3) * (KB * 16) + blk * 16 + (in & 7) * 2;
          *reinterpret_cast<uint2v*>(p) = uint2v{(uint32_t)h0.x | ((uint32_t)h1.x << 16), (uint32_t)h2.x | ((uint32_t)h3.x << 16)};
          if ((tid & 7) == 0) xsum[b * KB + blk] = sum;
          if (a.gain) gemv_store_xn(a, b0 + b, k, v, k < K);
        }
      }
    }
  }
  __syncthreads();

  float acc[RW][NB];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
  for (int t = 0; t < items; ++t) {
    if (t + 1 < items) load_item(t + 1, wnxt, snxt);
    const auto it = wk.item(t);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int blk = it.live ? it.c * CHB + u * 64 + lane : KB;
      if (blk < KB) {
        uint32_t pr[RW][16];  // packed bf16 pairs (136 + q, 136 + q)
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const uint32_t wd = wcur[u][r][d];
#pragma unroll
            for (int j = 0; j < 4; ++j) pr[r][d * 4 + j] = ((wd >> (4 * j)) & 0x000F000Fu) | 0x43004300u;
          }
        float sf[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) sf[r] = __builtin_bit_cast(float, scur[u][r] << 16);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (b >= nb) continue;
          const char* xb = smem + (size_t)b * row_bytes + blk * 16;
          uint4v xv[4];
#pragma unroll
          for (int d = 0; d < 4; ++d) xv[d] = *reinterpret_cast<const uint4v*>(xb + (size_t)d * (KB * 16));
          const float t0 = -I4_BIAS * xsum[b * KB + blk];
#pragma unroll
          for (int r = 0; r < RW; ++r) {
            float tt = t0;
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const uint32_t xj = xv[d][j], pj = pr[r][d * 4 + j];
                tt = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, pj), __builtin_bit_cast(bf16x2, xj), tt, false);
              }
            acc[r][b] = fmaf(sf[r], tt, acc[r][b]);
          }
        }
      }
    }
    if (it.last) gemv_finish_group<NB, R, DUAL, false, PAIR>(a, acc, red2, it.g, it.pass, wk.half, lane, wave, b0, nb);
    if (t + 1 < items) {
#pragma unroll
      for (int u = 0; u < UNR; ++u)
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          wcur[u][r] = wnxt[u][r];
          scur[u][r] = snxt[u][r];
        }
    }
  }
  gemv_stamp_end(a.stamp, st_t, st_cnt, t_begin, lane);
}

template <int NB>
static void gemv_int4_dispatch(const GemvArgs& a, int b0, int nb, hipStream_t s) {
  const int KB = cdiv(a.K, I4_BLOCK), G = cdiv(a.K, I4_GROUP);
  const size_t lds = (size_t)NB * KB * (64 + 4);
  // algorithmic bytes: every nibble and every scale once (+ the tiny activation / output vectors)
  const double wbytes = (double)a.N * ((double)a.K * 0.5 + G * 2.0) * (a.W2 ? 2 : 1) + (double)nb * (a.K + a.N) * 4;
  gemv_dispatch_pass("gemv_int4", "int4w", a, lds, wbytes, nb, s, [&](auto xpt_t, auto dual_t, auto pair_t, const GemvArgs& g, int grid) {
    gemv_launch<&gemv_int4_kernel<NB, decltype(dual_t)::value, decltype(xpt_t)::value, decltype(pair_t)::value>>(grid, lds, s, g, b0, nb);
  });
}

void launch_gemv_int4(const GemvArgs& a, hipStream_t s) {
  const int G = cdiv(a.K, I4_GROUP);
  if (a.K % 16 || ((uintptr_t)a.W & 15) || ((uintptr_t)a.W2 & 15) || a.ldw % 16 || a.ldw < G * 64)
    throw std::runtime_error("gemv_int4: K must be a multiple of 16 and nibble rows 16-byte aligned, whole groups long");
  if (!a.gscale || (a.W2 && !a.gscale2) || a.ld_gscale < G) throw std::runtime_error("gemv_int4: group scales missing");
  if (((uintptr_t)a.x & 15) || a.ldx % 4 || (a.gain && ((uintptr_t)a.gain & 15)) ||
      (a.xn_out && (((uintptr_t)a.xn_out & 15) || a.xn_ld % 4)))
    throw std::runtime_error("gemv_int4: x / gain / xn_out rows must be 16-byte aligned");
  // up to four batch rows per pass (5 - 8 rows: two passes)
  gemv_passes<4>(0, a.B, [&](auto nb_t, int b0, int nb) { gemv_int4_dispatch<decltype(nb_t)::value>(a, b0, nb, s); });
}

}  // namespace anyref
