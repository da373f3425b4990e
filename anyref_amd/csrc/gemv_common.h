// What the decode GEMV kernels (gemv.hip: gemv_kernel, gemv_rows8_kernel; gemv_int4.hip: gemv_int4_kernel) and their launchers
// have in common.  Device side: the (row group, K chunk) work list with the wave-pair split, the RMSNorm input stage, the
// row-group finish with its scalar epilogue, the kernel-side stamps.  Host side: the measurement knobs, the grid and wave-pair
// rules, the XPT-by-K ladder, the launch and the passes loop.  Everything here is inlined: no run-time indirection.
#pragma once
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "kernels.h"

namespace anyref {

// ---------------------------------------------------------------------------------------------
// Device
// ---------------------------------------------------------------------------------------------
// Flattened (row group, K chunk) work list of one wave, walked software-pipelined one chunk deep by the kernels.
// PAIR: waves 2i and 2i + 1 of a workgroup share their row groups, each sweeping every second K chunk, and every wave walks the
// same number of groups (they all meet at the hand-off barrier of gemv_finish_group); items past the end are not live.
template <int R, bool PAIR>  // R: output rows per row group
struct GemvWork {
  int ngroups, nch, unit, nunits, half, nchp, items;
  __device__ __forceinline__ GemvWork(unsigned grid, unsigned block, int wave, int N, int nch_) {
    const int nwaves = grid * 8, gw = block * 8 + wave;
    ngroups = cdiv(N, R);
    nch = nch_;
    unit = PAIR ? gw >> 1 : gw;
    nunits = PAIR ? nwaves >> 1 : nwaves;
    half = PAIR ? (gw & 1) : 0;
    nchp = PAIR ? (nch + 1) >> 1 : nch;  // chunk slots per wave and group
    const int my_groups = PAIR ? cdiv(ngroups, nunits) : (gw < ngroups ? (ngroups - gw + nwaves - 1) / nwaves : 0);
    items = my_groups * nchp;
  }
  struct Item {
    int pass, g, c;   // which of the wave's groups, the row group, the K chunk
    bool live, last;  // last: the group's last chunk slot of this wave
  };
  __device__ __forceinline__ Item item(int t) const {
    const int pass = t / nchp, ci = t % nchp;
    const int g = unit + pass * nunits, c = PAIR ? 2 * ci + half : ci;
    return {pass, g, c, !PAIR || (g < ngroups && c < nch), ci == nchp - 1};
  }
};

// RMSNorm input stage in two halves: load() issues the 16-byte loads of the gain and of the NB x rows into registers (XV
// float4 per thread and row; the launchers check the alignment), scales() does the sums of squares of ALL rows behind ONE
// barrier (a barrier per row: NB dependent LDS round trips per launch).  The caller issues its first weight prefetch BETWEEN
// the two: x goes first into the (in-order) vector-memory queue, so that its wait leaves the weight chunk issued right behind
// it in flight.  Issued the other way round, the x wait also waited for the first weight chunk (measured: x staged 4 - 9 us
// into a 10 - 22 us kernel).  Writing the normalised rows into LDS stays with each kernel (the layouts differ).
template <int NB, int XV>
struct GemvNormStage {
  float4v xr[NB][XV], gr[XV];
  __device__ __forceinline__ void load_gain(const GemvArgs& a, int tid) {
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int k = (tid + i * 512) * 4;
      gr[i] = k < a.K ? *reinterpret_cast<const float4v*>(a.gain + k) : float4v{1.f, 1.f, 1.f, 1.f};
    }
  }
  __device__ __forceinline__ void load_x(const GemvArgs& a, int b0, int nb, int tid) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float* x = a.x + (int64_t)(b0 + (b < nb ? b : 0)) * a.ldx;
#pragma unroll
      for (int i = 0; i < XV; ++i) {
        const int k = (tid + i * 512) * 4;
        xr[b][i] = (b < nb && k < a.K) ? *reinterpret_cast<const float4v*>(x + k) : float4v{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  __device__ __forceinline__ void load(const GemvArgs& a, int b0, int nb, int tid) {
    load_gain(a, tid);
    load_x(a, b0, nb, tid);
  }
  __device__ __forceinline__ void scales(const GemvArgs& a, float (&red)[NB][8], int lane, int wave, float (&scale)[NB]) const {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < XV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) ss += xr[b][i][e] * xr[b][i][e];
      ss = wave_sum(ss);
      if (lane == 0) red[b][wave] = ss;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) tot += red[b][w];
      scale[b] = rsqrtf(tot / (float)a.K + a.eps);
    }
  }
};
// the normalised row itself is an output of the step (last-layer hidden state before lm_head): workgroup 0 stores it
// (also: what else the caller's layout asks of this piece)
__device__ __forceinline__ void gemv_store_xn(const GemvArgs& a, int row, int k, float4v v, bool also = true) {
  if (a.xn_out && blockIdx.x == 0 && also)
    *reinterpret_cast<float4v*>(a.xn_out + (int64_t)(a.xn_row_map ? a.xn_row_map[row] : row) * a.xn_ld + k) = v;
}

// One finished output: optional per-row weight scale (fp8), bias, SwiGLU or act, residual, store.
template <bool DUAL, bool W8>
__device__ __forceinline__ void gemv_epilogue(const GemvArgs& a, float v, float v2, int n, int row) {
  if constexpr (W8) {
    v *= a.wscale[(int64_t)n * a.ws_stride];
    if (DUAL) v2 *= a.wscale2[(int64_t)n * a.ws_stride];
  }
  if (a.bias) v += a.bias[n];
  if (DUAL)
    v = apply_act(v, ACT_SILU) * v2;
  else
    v = apply_act(v, a.act);
  const int64_t o = (int64_t)row * a.ldy + n;
  if (a.resid) v += a.resid[o];
  a.y[o] = v;
}

// Row group g finished: reduce across the wave, (PAIR) the odd wave hands its partial sums to the even one through red2 (one
// barrier per group, double-buffered over the wave's groups, fixed order: deterministic), store, and clear the sums.
// Every lane holds every reduced sum (xor butterfly): lane i < R * NB finishes output (r, b) = (i / NB, i % NB) -- scale /
// bias / activation / residual load / store side by side.  One lane walking the R * NB outputs is a chain of dependent
// residual load -> store round trips (y may alias the residual, so the compiler keeps their order): 8 per row group at 4 batch
// rows, on the wave's critical path at the end of the launch.
template <int NB, int R, bool DUAL, bool W8, bool PAIR>
__device__ __forceinline__ void gemv_finish_group(const GemvArgs& a, float (&acc)[2][NB], float (&red2)[2][4][2][NB], int g,
                                                  int pass, int half, int lane, int wave, int b0, int nb) {
  constexpr int RW = 2;
  const int n0 = g * R;
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = wave_sum(acc[r][b]);
  if constexpr (PAIR) {
    const int buf = pass & 1;
    if (half == 1 && lane == 0) {
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int b = 0; b < NB; ++b) red2[buf][wave >> 1][r][b] = acc[r][b];
    }
    __syncthreads();
    if (half == 0) {
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[r][b] += red2[buf][wave >> 1][r][b];
    }
  }
  if (lane < R * NB && half == 0) {
    const int r = lane / NB, b = lane % NB, n = n0 + r;
    float v = 0.f, v2 = 0.f;
#pragma unroll
    for (int rr = 0; rr < R; ++rr)
#pragma unroll
      for (int bb = 0; bb < NB; ++bb)
        if (lane == rr * NB + bb) {
          v = acc[rr][bb];
          v2 = DUAL ? acc[RW - 1][bb] : 0.f;
        }
    if (n < a.N && b < nb) gemv_epilogue<DUAL, W8>(a, v, v2, n, b0 + b);
  }
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
}

// Kernel-side timestamps (kernels.h: StampArgs): off in production (one uniform branch).  st_t / st_cnt are the kernel's own
// __shared__ words; a barrier (the one after the x stage) must lie between begin and end.
__device__ __forceinline__ unsigned long long gemv_stamp_begin(const StampArgs& st, unsigned long long (&st_t)[2],
                                                               unsigned& st_cnt, int tid) {
  unsigned long long t_begin = 0;
  if (st.base) {
    t_begin = wall_clock64();
    if (tid == 0) {
      st_t[0] = ~0ull;
      st_t[1] = 0;
      st_cnt = 0;
    }
  }
  return t_begin;
}
__device__ __forceinline__ void gemv_stamp_end(const StampArgs& st, unsigned long long (&st_t)[2], unsigned& st_cnt,
                                               unsigned long long t_begin, int lane) {
  if (st.base && lane == 0) {
    // every wave folds its span into the workgroup's (LDS atomics; the init is ordered by the barrier after the x
    // stage); the wave whose count comes back last has seen all of them and writes the workgroup's slot
    atomicMin(&st_t[0], t_begin);
    atomicMax(&st_t[1], (unsigned long long)wall_clock64());
    if (atomicAdd(&st_cnt, 1u) == 7u) {
      const int e = *st.epoch;
      if (e < st.max_epoch) {
        unsigned long long* p = st.base + (size_t)e * st.stride + (size_t)blockIdx.x * 2;
        p[0] = st_t[0];
        p[1] = st_t[1];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Host
// ---------------------------------------------------------------------------------------------
// ANYREF_GEMV_GRID=n: decode GEMV workgroups (measurement knob, read once; never set in production)
// ANYREF_GEMV_PAIR=0: one wave per row group (the round-2 work split) instead of wave pairs sharing a group's K chunks
inline bool gemv_pair_knob() {
  static const bool p = !(getenv("ANYREF_GEMV_PAIR") && atoi(getenv("ANYREF_GEMV_PAIR")) == 0);
  return p;
}
inline int gemv_grid_knob() {
  static const int g = getenv("ANYREF_GEMV_GRID") ? atoi(getenv("ANYREF_GEMV_GRID")) : 0;
  return g;
}

struct GemvPlan {
  int grid;
  bool pair;
};
// lds: bytes of the activation stage of one workgroup
inline GemvPlan gemv_plan(const GemvArgs& a, size_t lds) {
  // one or two 8-wave workgroups per CU depending on the LDS the activation stage needs
  // (512 workgroups measured best for N*K of 34-262 MB; 256 / 1024 / 2048 were 3-30 % slower)
  const int grid_rule = 256 * (lds > 76 * 1024 ? 1 : 2);
  int grid = grid_rule;
  if (a.grid > 0 && a.grid < grid) grid = a.grid;
  if (gemv_grid_knob() > 0) grid = gemv_grid_knob();
  // wave pairs where single waves would leave half of the grid without a row group (N = 4096 at 7B: o_proj 8.5 ->
  // 8.05 us, down_proj 17.45 -> 16.7 us); with more groups than waves the plain split is faster (qkv 17.9 vs 18.8 us,
  // gate/up 30.9 vs 31.6: the hand-off barrier per group costs more than the better balance returns).  Decided by the
  // rule's grid, not the capped one: the same sums whatever grid is asked for
  const bool pair = gemv_pair_knob() && cdiv(a.N, a.W2 ? 1 : 2) * 2 <= (gemv_grid_knob() > 0 ? grid : grid_rule) * 8;
  return {grid, pair};
}

// set the dynamic-LDS limit once per kernel instantiation (and device), then launch
template <auto KERN, int LDS_MAX = 150 * 1024, typename... Args>
inline void gemv_launch(int grid, size_t lds, hipStream_t s, Args... args) {
  static KernelAttrOnce once;
  ensure_dyn_lds(once, reinterpret_cast<const void*>(KERN), LDS_MAX);
  hipLaunchKernelGGL(KERN, dim3(grid), dim3(512), lds, s, args...);
}

// One pass of a decode GEMV: plan, tag ("gemv_<kind>[_swiglu]_x<XPT>": one per kernel instantiation, so a tag's average can
// be checked against rocprofv3's per-kernel one), profile / stamp bracket, and launch(xpt, dual, pair, args, grid) with the
// three as integral_constant tags.  XPT: x elements per thread in the staging, K <= 512 * XPT.
// wbytes: algorithmic bytes, every weight element once (+ the tiny activation / output vectors)
template <typename Launch>
inline void gemv_dispatch_pass(const char* name, const char* kind, const GemvArgs& a_in, size_t lds, double wbytes, int nb,
                               hipStream_t s, Launch&& launch) {
  GemvArgs a = a_in;
  if (lds > 150 * 1024) throw std::runtime_error(std::string(name) + ": K too large for the LDS activation stage");
  const GemvPlan p = gemv_plan(a, lds);
  auto go = [&](auto xpt_t) {
    char tag[40];
    snprintf(tag, sizeof(tag), "gemv_%s%s_x%d", kind, a.W2 ? "_swiglu" : "", decltype(xpt_t)::value);
    ProfScope prof(tag, 2.0 * nb * a.N * (double)a.K * (a.W2 ? 2 : 1), wbytes, s);
    if (g_stamp && g_stamp->on) a.stamp = g_stamp->slot(tag, wbytes, p.grid);
    using TT = std::true_type;
    using FF = std::false_type;
    if (a.W2) {
      if (p.pair) launch(xpt_t, TT(), TT(), a, p.grid);
      else launch(xpt_t, TT(), FF(), a, p.grid);
    } else {
      if (p.pair) launch(xpt_t, FF(), TT(), a, p.grid);
      else launch(xpt_t, FF(), FF(), a, p.grid);
    }
  };
  if (a.K <= 512 * 8)
    go(std::integral_constant<int, 8>());
  else if (a.K <= 512 * 24)
    go(std::integral_constant<int, 24>());
  else if (a.K <= 512 * 32)
    go(std::integral_constant<int, 32>());
  else
    throw std::runtime_error(std::string(name) + ": K > 16384 not supported");
}

// rows [b0, B) in passes of up to NBMAX rows: pass(nb_tag, b0, nb) with the kernel's NB (1, 2 or NBMAX) as the tag
template <int NBMAX, typename Pass>
inline void gemv_passes(int b0, int B, Pass&& pass) {
  while (b0 < B) {
    const int left = B - b0, nb = left < NBMAX ? left : NBMAX;
    if (nb == 1)
      pass(std::integral_constant<int, 1>(), b0, nb);
    else if (nb == 2)
      pass(std::integral_constant<int, 2>(), b0, nb);
    else
      pass(std::integral_constant<int, NBMAX>(), b0, nb);
    b0 += nb;
  }
}

}  // namespace anyref
