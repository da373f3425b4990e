// SAM's spatial prompts (prompt_encoder.py:78-186): the decoder's token matrix with point / box / text rows behind the output
// tokens, and the fused mask_downscaling that writes the decoder's keys.  Both f32, no atomics: reruns are bit-identical.
#include "prompt_encode.h"

#include "kernels.h"

namespace anyref {

constexpr int kPromptGridCap = 2048;  // workgroups per launch; the grid-stride loops take the rest

// tokens [n, NQ, C], NQ = n_out + P + pad + 2 * box + text with pad = (P > 0 and no boxes):
//   rows [0, n_out)  out_tokens
//   then P points    PE(p) + emb5[label] for label 0 / 1, emb5[4] alone for label -1, PE(p) alone for any other label
//   then the pad     emb5[4] (a not-a-point at coordinate 0)
//   then two corners PE(x0, y0) + emb5[2], PE(x1, y1) + emb5[3]
//   then text[i]
// PE(p): c = (p + 0.5) / S, v = 2 pi ((2 c_x - 1) G0 + (2 c_y - 1) G1), sin v | cos v -- the argument arithmetic of
// dense_pe_kernel (ops.hip), full-precision sinf / cosf.  One thread per four channels, one 16-byte store each.
__global__ __launch_bounds__(256) void prompt_tokens_kernel(const float* __restrict__ out_tokens, int n_out,
                                                            const float* __restrict__ points,
                                                            const int32_t* __restrict__ labels, int P,
                                                            const float* __restrict__ boxes, const float* __restrict__ text,
                                                            const float* __restrict__ gauss, const float* __restrict__ emb5,
                                                            int n, int C, int S, float* __restrict__ tokens) {
  const int C4 = C / 4, F = C / 2;
  const int pad = (P > 0 && !boxes) ? 1 : 0, nb = boxes ? 2 : 0;
  const int NQ = n_out + P + pad + nb + (text ? 1 : 0);
  const int64_t total = (int64_t)n * NQ * C4;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(idx % C4) * 4;
    const int t = (int)((idx / C4) % NQ), i = (int)(idx / ((int64_t)C4 * NQ));
    int s = t - n_out;
    const float* copy = nullptr;  // rows that are a plain copy
    const float* add = nullptr;   // embedding added to the PE
    float px = 0.f, py = 0.f;
    bool pe = false;
    if (s < 0) {
      copy = out_tokens + (int64_t)t * C;
    } else if (s < P) {
      const int lab = labels[(int64_t)i * P + s];
      if (lab == -1) {
        copy = emb5 + 4 * (int64_t)C;
      } else {
        pe = true;
        px = points[((int64_t)i * P + s) * 2];
        py = points[((int64_t)i * P + s) * 2 + 1];
        if (lab == 0 || lab == 1) add = emb5 + (int64_t)lab * C;
      }
    } else if ((s -= P) < pad) {
      copy = emb5 + 4 * (int64_t)C;
    } else if ((s -= pad) < nb) {
      pe = true;
      px = boxes[(int64_t)i * 4 + 2 * s];
      py = boxes[(int64_t)i * 4 + 2 * s + 1];
      add = emb5 + (int64_t)(2 + s) * C;
    } else {
      copy = text + (int64_t)i * C;
    }
    float4 o;
    if (!pe) {
      o = *reinterpret_cast<const float4*>(copy + d);
    } else {
      const float cx = 2.f * ((px + 0.5f) / (float)S) - 1.f, cy = 2.f * ((py + 0.5f) / (float)S) - 1.f;
      const bool is_cos = d >= F;  // F % 4 == 0: the four channels lie on one side
      const int f = is_cos ? d - F : d;
      const float4 g0 = *reinterpret_cast<const float4*>(gauss + f);
      const float4 g1 = *reinterpret_cast<const float4*>(gauss + F + f);
      const float v0 = 6.283185307179586f * (cx * g0.x + cy * g1.x), v1 = 6.283185307179586f * (cx * g0.y + cy * g1.y);
      const float v2 = 6.283185307179586f * (cx * g0.z + cy * g1.z), v3 = 6.283185307179586f * (cx * g0.w + cy * g1.w);
      if (is_cos) o = make_float4(cosf(v0), cosf(v1), cosf(v2), cosf(v3));
      else o = make_float4(sinf(v0), sinf(v1), sinf(v2), sinf(v3));
      if (add) {
        const float4 a = *reinterpret_cast<const float4*>(add + d);
        o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
      }
    }
    *reinterpret_cast<float4*>(tokens + ((int64_t)i * NQ + t) * C + d) = o;
  }
}

int prompt_token_rows(int n_out, int P, bool boxes, bool text) {
  return n_out + P + ((P > 0 && !boxes) ? 1 : 0) + (boxes ? 2 : 0) + (text ? 1 : 0);
}

void launch_prompt_tokens(const float* out_tokens, int n_out, const float* points, const int32_t* labels, int P,
                          const float* boxes, const float* text, const float* gauss, const float* emb5, int n, int C, int S,
                          float* tokens, hipStream_t s, int max_wg) {
  if (n < 1 || n_out < 1 || P < 0 || S < 1) throw std::runtime_error("prompt_tokens: n >= 1, n_out >= 1, P >= 0, S >= 1");
  if (C < 8 || C % 8) throw std::runtime_error("prompt_tokens: C must be a multiple of 8 (four channels per thread on one side of sin | cos)");
  if (P > 0 && (!points || !labels)) throw std::runtime_error("prompt_tokens: points given without labels (or labels without points)");
  if (!out_tokens || !gauss || !emb5 || !tokens) throw std::runtime_error("prompt_tokens: null argument");
  if (((uintptr_t)out_tokens | (uintptr_t)gauss | (uintptr_t)emb5 | (uintptr_t)tokens | (uintptr_t)text) & 15)
    throw std::runtime_error("prompt_tokens: out_tokens / gauss / emb5 / text / tokens must be 16-byte aligned");
  const int64_t total = (int64_t)n * prompt_token_rows(n_out, P, boxes != nullptr, text != nullptr) * (C / 4);
  const int cap = max_wg > 0 ? max_wg : kPromptGridCap;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv64(total, 256), cap));
  hipLaunchKernelGGL(prompt_tokens_kernel, dim3(grid), dim3(256), 0, s, out_tokens, n_out, points, labels, P, boxes, text, gauss,
                     emb5, n, C, S, tokens);
}

// keys[i, y*g + x, :] = image_emb[y*g + x, :] + mask_downscaling(mask_input[i])[:, y, x]   (prompt_encoder.py:55-64,111-114)
// mask_downscaling = conv k2s2 (1 -> c1), LayerNorm2d, GELU, conv k2s2 (c1 -> c2), LayerNorm2d, GELU, conv 1x1 (c2 -> C).
// One output pixel reads a 4x4 patch.  A workgroup takes kMpePix pixels per pass:
//   A  a thread per (pixel, 2x2 position): the c1 values of conv 1, their norm and GELU        -> LDS s1
//   B  a thread per (pixel, c2 channel): the 4 c1-term dot of conv 2 -> LDS raw; then the norm over the pixel's c2 raw
//      values (each thread sums them itself, in channel order) and GELU                          -> LDS s2
//   C  a thread per (pixel, four output channels): the c2-term dot with its conv-3 rows in registers (loaded once per
//      workgroup: the thread's channel group does not change between passes), + bias first, + image embedding last,
//      one 16-byte store, coalesced over C
constexpr int kMpePix = 16, kMpeC1 = 8, kMpeC2 = 32;

__global__ __launch_bounds__(256) void mask_prompt_embed_kernel(
    const float* __restrict__ mask, const float* __restrict__ image_emb, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ g1, const float* __restrict__ be1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ g2, const float* __restrict__ be2, const float* __restrict__ w3,
    const float* __restrict__ b3, int n, int g, int C, int c1, int c2, float eps, float* __restrict__ keys) {
  __shared__ float s1[kMpePix][4][kMpeC1];
  __shared__ float raw2[kMpePix][kMpeC2];
  __shared__ float s2[kMpePix][kMpeC2];
  const int tid = threadIdx.x, C4 = C / 4, L = 4 * g;
  const int64_t npix = (int64_t)n * g * g;
  const int64_t tiles = (npix + kMpePix - 1) / kMpePix;
  // phase C's fixed role and weights
  const int cg = tid % C4, lane_pix = tid / C4, PP = 256 / C4;  // C4 <= 256 (launcher)
  float w[4][kMpeC2];
  float4 bias3 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (lane_pix < PP) {
    bias3 = *reinterpret_cast<const float4*>(b3 + 4 * cg);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < kMpeC2; ++j) w[k][j] = j < c2 ? w3[(int64_t)(4 * cg + k) * c2 + j] : 0.f;
  }
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t p0 = tile * kMpePix;
    // ---- A ----
    if (tid < kMpePix * 4) {
      const int pl = tid >> 2, pos = tid & 3;
      const int64_t p = p0 + pl;
      if (p < npix) {
        const int i = (int)(p / ((int64_t)g * g)), yx = (int)(p % ((int64_t)g * g)), y = yx / g, x = yx % g;
        const float* m = mask + ((int64_t)i * L + 4 * y + 2 * (pos >> 1)) * L + 4 * x + 2 * (pos & 1);
        const float2 r0 = *reinterpret_cast<const float2*>(m), r1 = *reinterpret_cast<const float2*>(m + L);
        float a[kMpeC1];
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < kMpeC1; ++c) {
          a[c] = 0.f;
          if (c < c1) {
            float acc = b1[c];
            acc = fmaf(w1[c * 4 + 0], r0.x, acc);
            acc = fmaf(w1[c * 4 + 1], r0.y, acc);
            acc = fmaf(w1[c * 4 + 2], r1.x, acc);
            acc = fmaf(w1[c * 4 + 3], r1.y, acc);
            a[c] = acc;
            sum += acc;
          }
        }
        const float mean = sum / (float)c1;
        float var = 0.f;
#pragma unroll
        for (int c = 0; c < kMpeC1; ++c)
          if (c < c1) {
            a[c] -= mean;
            var = fmaf(a[c], a[c], var);
          }
        const float rs = 1.f / sqrtf(var / (float)c1 + eps);
#pragma unroll
        for (int c = 0; c < kMpeC1; ++c)
          if (c < c1) s1[pl][pos][c] = apply_act(g1[c] * (a[c] * rs) + be1[c], ACT_GELU);
      }
    }
    __syncthreads();
    // ---- B ----
    for (int e = tid; e < kMpePix * c2; e += 256) {
      const int pl = e / c2, co = e % c2;
      if (p0 + pl < npix) {
        float acc = b2[co];
        for (int c = 0; c < c1; ++c)
#pragma unroll
          for (int pos = 0; pos < 4; ++pos) acc = fmaf(w2[((int64_t)co * c1 + c) * 4 + pos], s1[pl][pos][c], acc);
        raw2[pl][co] = acc;
      }
    }
    __syncthreads();
    for (int e = tid; e < kMpePix * c2; e += 256) {
      const int pl = e / c2, co = e % c2;
      if (p0 + pl < npix) {
        float sum = 0.f;
        for (int j = 0; j < c2; ++j) sum += raw2[pl][j];
        const float mean = sum / (float)c2;
        float var = 0.f;
        for (int j = 0; j < c2; ++j) {
          const float dj = raw2[pl][j] - mean;
          var = fmaf(dj, dj, var);
        }
        const float rs = 1.f / sqrtf(var / (float)c2 + eps);
        s2[pl][co] = apply_act(g2[co] * ((raw2[pl][co] - mean) * rs) + be2[co], ACT_GELU);
      }
    }
    __syncthreads();
    // ---- C ----
    if (lane_pix < PP)
      for (int pl = lane_pix; pl < kMpePix; pl += PP) {
        const int64_t p = p0 + pl;
        if (p >= npix) break;
        float acc[4] = {bias3.x, bias3.y, bias3.z, bias3.w};
#pragma unroll
        for (int j = 0; j < kMpeC2; ++j)
          if (j < c2) {
            const float v = s2[pl][j];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fmaf(w[k][j], v, acc[k]);
          }
        const float4 e = *reinterpret_cast<const float4*>(image_emb + (p % ((int64_t)g * g)) * C + 4 * cg);
        *reinterpret_cast<float4*>(keys + p * C + 4 * cg) = make_float4(acc[0] + e.x, acc[1] + e.y, acc[2] + e.z, acc[3] + e.w);
      }
    __syncthreads();  // the next pass rewrites s1 / raw2 / s2
  }
}

void launch_mask_prompt_embed(const float* mask, const float* image_emb, const MaskDownW& W, int n, int g, int C, float* keys,
                              hipStream_t s, int max_wg) {
  if (n < 1 || g < 1) throw std::runtime_error("mask_prompt_embed: n >= 1, g >= 1");
  if (W.c1 < 1 || W.c1 > kMpeC1 || W.c2 < 1 || W.c2 > kMpeC2)
    throw std::runtime_error("mask_prompt_embed: c1 in [1, 8] and c2 in [1, 32]");
  if (C < 4 || C % 4 || C > 1024) throw std::runtime_error("mask_prompt_embed: C must be a multiple of 4, at most 1024");
  if (!mask || !image_emb || !keys || !W.w1 || !W.b1 || !W.g1 || !W.be1 || !W.w2 || !W.b2 || !W.g2 || !W.be2 || !W.w3 || !W.b3)
    throw std::runtime_error("mask_prompt_embed: null argument");
  if (((uintptr_t)mask & 7) || (((uintptr_t)image_emb | (uintptr_t)keys | (uintptr_t)W.b3) & 15))
    throw std::runtime_error("mask_prompt_embed: mask_input must be 8-byte, image_emb / keys / conv-3 bias 16-byte aligned");
  const int64_t tiles = cdiv64((int64_t)n * g * g, kMpePix);
  const int cap = max_wg > 0 ? max_wg : kPromptGridCap;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, cap));
  hipLaunchKernelGGL(mask_prompt_embed_kernel, dim3(grid), dim3(256), 0, s, mask, image_emb, W.w1, W.b1, W.g1, W.be1, W.w2, W.b2,
                     W.g2, W.be2, W.w3, W.b3, n, g, C, W.c1, W.c2, 1e-6f, keys);
}

}  // namespace anyref
