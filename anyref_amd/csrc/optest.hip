// Kernel-level C entry points for the parity tests (include/anyref_hip_ops.h).
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/anyref_hip_ops.h"
#include "kernels.h"
#include "mask_report.h"
#include "prompt_encode.h"

using namespace anyref;

static thread_local std::string g_op_err;
static thread_local std::string g_op_tags;

#define OP_GUARD(...)                                    \
  try {                                                  \
    __VA_ARGS__;                                         \
    hipError_t _e = hipGetLastError();                   \
    if (_e != hipSuccess) {                              \
      g_op_err = std::string("HIP error: ") + hipGetErrorString(_e); \
      return 3;                                          \
    }                                                    \
    return 0;                                            \
  } catch (const std::exception& e) {                    \
    g_op_err = e.what();                                 \
    return 2;                                            \
  }

namespace {
// t = 3 (split pairs, ANYREF_MODE_PARITY16): the entry points keep their f32 interface -- an f32 operand that the mode
// carries as a bf16 pair is split into a temporary here, a pair-typed result is read back as hi + lo
// t = 4 (ANYREF_MODE_PARITY16_F16): the same with f16 pairs and f16 weights
struct TmpBuf {
  void* p = nullptr;
  explicit TmpBuf(size_t bytes) { HIP_TRY(hipMalloc(&p, bytes ? bytes : 16)); HIP_TRY(hipMemset(p, 0, bytes ? bytes : 16)); }
  ~TmpBuf() { (void)hipDeviceSynchronize(); (void)hipFree(p); }
};
inline int pad64(int k) { return (k + 63) / 64 * 64; }
// books the launch tags of one *_ex call: a Profiler on g_prof for the duration of the call
struct TagScope {
  Profiler prof;
  Profiler* prev;
  hipStream_t st;
  explicit TagScope(hipStream_t s) : prev(g_prof), st(s) {
    g_op_tags.clear();
    prof.on = true;
    g_prof = &prof;
  }
  ~TagScope() {
    g_prof = prev;
    (void)hipStreamSynchronize(st);  // the bracket events are destroyed with the Profiler
    for (auto& kv : prof.stats()) g_op_tags += (g_op_tags.empty() ? "" : ",") + kv.first;
  }
};
template <typename F>
void by_type(int t, F&& f) {  // f(T()) for the storage type t = 0 .. 4
  if (t == 0) f(float());
  else if (t == 1) f(bf16());
  else if (t == 2) f(f16());
  else if (t == 3) f(sp16());
  else if (t == 4) f(sp16h());
  else throw std::runtime_error("op: t = 0 .. 4");
}
// t = 3 / 4 of the im2col entries: the kernel writes pair rows [rows, cols] (cols % 64 == 0) into a temporary whose every 16-bit
// word starts as a NaN pattern (an element the kernel leaves out comes back as NaN, not as a zero that a pad column should be),
// out f32 [rows, cols] = hi + lo
template <typename F>
void im2col_pairs(int t, int rows, int cols, float* out, hipStream_t st, F&& run) {
  if (cols % 64) throw std::runtime_error("op_im2col t=3/4: the row length must be a multiple of 64");
  TmpBuf Ps((size_t)rows * cols * 4);
  HIP_TRY(hipMemset(Ps.p, 0xFF, (size_t)rows * cols * 4));
  run(Ps.p);
  launch_unsplit(Ps.p, cols, out, cols, rows, cols, st, t == 4);
}
}  // namespace

extern "C" {

const char* anyref_op_last_error(void) { return g_op_err.c_str(); }
const char* anyref_op_last_tags(void) { return g_op_tags.c_str(); }

int anyref_op_gemm_ex(int t, void* stream, anyref_gemm_ex* e) {
  OP_GUARD({
    hipStream_t st = (hipStream_t)stream;
    e->norm_done = 0;
    bool fused = false;
    GemmArgs a;
    a.A = e->A; a.W = e->W; a.bias = e->bias; a.C = e->C; a.resid = e->resid; a.row_map = e->row_map;
    a.a_row_map = e->a_row_map; a.M = e->M; a.N = e->N; a.K = e->K; a.lda = e->lda; a.ldw = e->ldw; a.ldc = e->ldc;
    a.ldr = e->ldr; a.act = e->act; a.c_f32 = e->c_f32; a.alpha = e->alpha; a.swiglu_pairs = e->swiglu_pairs;
    a.max_wg = e->max_wg; a.norm_gain = e->norm_gain; a.norm_out = e->norm_out; a.norm_ld = e->norm_ld;
    a.norm_eps = e->norm_eps; a.norm_bias = e->norm_bias; a.slabs_out = e->slabs_out; a.slabs = e->slabs;
    a.norm_done = &fused; a.batch = e->batch; a.sA = e->sA; a.sW = e->sW; a.sC = e->sC; a.sR = e->sR; a.sBias = e->sBias;
    TagScope tags(st);
    if (t == 3 || t == 4) {  // A f32 -> pairs; a pair-typed C / norm_out is read back as hi + lo into the f32 array given
      const bool h16 = t == 4;
      if (e->batch != 1 || e->a_row_map || e->row_map || e->K % 64)
        throw std::runtime_error("op_gemm_ex t=3/4: batch 1, no row maps, K % 64 == 0");
      const int nc = e->swiglu_pairs ? e->N / 2 : e->N;
      TmpBuf As((size_t)e->M * e->K * 4), Cs(e->c_f32 ? 0 : (size_t)e->M * pad64(nc) * 4),
          Ns(e->norm_out ? (size_t)e->M * pad64(e->N) * 4 : 0);
      if (h16) launch_convert<sp16h>(reinterpret_cast<const float*>(e->A), e->lda, As.p, e->K, e->M, e->K, st);
      else launch_convert<sp16>(reinterpret_cast<const float*>(e->A), e->lda, As.p, e->K, e->M, e->K, st);
      a.A = As.p; a.lda = e->K;
      if (!e->c_f32 && !e->slabs_out) { a.C = Cs.p; a.ldc = pad64(nc); }
      if (e->norm_out) { a.norm_out = Ns.p; a.norm_ld = pad64(e->N); }
      if (h16) launch_gemm<sp16h>(a, st);
      else launch_gemm<sp16>(a, st);
      if (!e->c_f32 && !e->slabs_out) launch_unsplit(Cs.p, pad64(nc), reinterpret_cast<float*>(e->C), e->ldc, e->M, nc, st, h16);
      if (e->norm_out && fused)
        launch_unsplit(Ns.p, pad64(e->N), reinterpret_cast<float*>(e->norm_out), e->norm_ld, e->M, e->N, st, h16);
    } else {
      by_type(t, [&](auto T0) {
        using T = decltype(T0);
        if constexpr (!is_split<T>::value) launch_gemm<T>(a, st);
      });
    }
    e->norm_done = fused ? 1 : 0;
  });
}

int anyref_op_norm_ex(int t, void* stream, anyref_norm_ex* e) {
  OP_GUARD({
    hipStream_t st = (hipStream_t)stream;
    e->fill_done = 0;
    bool filled = false;
    NormArgs a;
    a.x = e->x; a.ldx = e->ldx; a.gain = e->gain; a.bias = e->bias; a.y = e->y; a.ldy = e->ldy; a.row_map = e->row_map;
    a.M = e->M; a.D = e->D; a.eps = e->eps; a.rms = e->rms; a.y_f32 = e->y_f32; a.act = e->act;
    a.fill_dst = e->fill_dst; a.fill_ld = e->fill_ld; a.fill_n = e->fill_n; a.fill_N = e->fill_N;
    a.fill_rows = e->fill_rows; a.fill_bias = e->fill_bias; a.fill_done = &filled;
    TagScope tags(st);
    if (t == 3 || t == 4) {  // the norm writes pairs: y's rows go through a pair-typed temporary and come back as hi + lo
      const bool h16 = t == 4;
      if (e->y_f32) throw std::runtime_error("op_norm_ex t=3/4: the pair-typed output only");
      int rows = e->M;
      if (e->row_map) {
        std::vector<int> h(e->M);
        HIP_TRY(hipMemcpy(h.data(), e->row_map, (size_t)e->M * 4, hipMemcpyDeviceToHost));
        for (int v : h) rows = std::max(rows, v + 1);
      }
      const int ld = pad64(e->D);
      TmpBuf Ys((size_t)rows * ld * 4);
      // (rows the map drops keep what y held: carried through the temporary)
      if (h16) launch_convert<sp16h>(reinterpret_cast<const float*>(e->y), e->ldy, Ys.p, ld, rows, e->D, st);
      else launch_convert<sp16>(reinterpret_cast<const float*>(e->y), e->ldy, Ys.p, ld, rows, e->D, st);
      a.y = Ys.p; a.ldy = ld;
      if (h16) launch_norm<sp16h>(a, st);
      else launch_norm<sp16>(a, st);
      launch_unsplit(Ys.p, ld, reinterpret_cast<float*>(e->y), e->ldy, rows, e->D, st, h16);
      if (!filled && e->fill_fallback && e->fill_n > 0)
        launch_fill_rows_bias<float>(e->fill_dst, e->fill_ld, e->fill_rows, e->fill_n, e->fill_bias, e->fill_N, st);
    } else {
      by_type(t, [&](auto T0) {
        using T = decltype(T0);
        if constexpr (!is_split<T>::value) {
          launch_norm<T>(a, st);
          if (!filled && e->fill_fallback && e->fill_n > 0)
            launch_fill_rows_bias<T>(e->fill_dst, e->fill_ld, e->fill_rows, e->fill_n, e->fill_bias, e->fill_N, st);
        }
      });
    }
    e->fill_done = filled ? 1 : 0;
  });
}

int anyref_op_attention_ex(int t, void* stream, anyref_attn_ex* e) {
  OP_GUARD({
    hipStream_t st = (hipStream_t)stream;
    AttnArgs a;
    a.Q = e->q; a.K = e->k; a.V = e->v; a.O = e->o;
    a.q_bs = e->q_bs; a.q_rs = e->q_rs; a.q_hs = e->q_hs; a.k_bs = e->k_bs; a.k_rs = e->k_rs; a.k_hs = e->k_hs;
    a.v_bs = e->v_bs; a.v_rs = e->v_rs; a.v_hs = e->v_hs; a.o_bs = e->o_bs; a.o_rs = e->o_rs; a.o_hs = e->o_hs;
    a.B = e->B; a.H = e->H; a.Sq = e->Sq; a.Sk = e->Sk; a.hd = e->hd; a.scale = e->scale; a.causal = e->causal;
    a.q_pos0 = e->q_pos0; a.kv_len = e->kv_len; a.q_len = e->q_len; a.rel_h = e->rel_h; a.rel_w = e->rel_w;
    a.kh = e->kh; a.kw = e->kw; a.rel_p = e->rel_p; a.rel_hs = e->rel_hs; a.rel_ld = e->rel_ld;
    a.rel_tab_h = e->rel_tab_h; a.rel_tab_w = e->rel_tab_w; a.rel_tab_ld = e->rel_tab_ld; a.max_wg = e->max_wg;
    TagScope tags(st);
    if (t == 3) {  // split-pair attention: f32 operands, pair-typed output rows; o gets hi + lo
      if (e->o_rs % 64 || e->o_bs != (int64_t)e->Sq * e->o_rs || e->H * e->hd > e->o_rs)
        throw std::runtime_error("op_attention_ex t=3: o rows are whole pair rows (o_rs % 64 == 0, o_bs == Sq * o_rs)");
      const int rows = e->B * e->Sq, cols = e->H * e->hd;
      TmpBuf Os((size_t)rows * e->o_rs * 4);
      // (rows past q_len keep what o held: carried through the temporary)
      launch_convert<sp16>(reinterpret_cast<const float*>(e->o), e->o_rs, Os.p, e->o_rs, rows, cols, st);
      a.O = Os.p; a.o_split = 1; a.sp16 = 1;
      launch_attention<float>(a, st);
      launch_unsplit(Os.p, e->o_rs, reinterpret_cast<float*>(e->o), e->o_rs, rows, cols, st, 0);
    } else if (t == 0) launch_attention<float>(a, st);
    else if (t == 2) launch_attention<f16>(a, st);
    else if (t == 1) launch_attention<bf16>(a, st);
    else throw std::runtime_error("op_attention_ex: t = 0 .. 3");
  });
}

int anyref_op_gemm(int t, void* stream, const void* A, const void* W, const float* bias, void* C,
                   const float* resid, const int32_t* row_map, int M, int N, int K, int act, int c_f32) {
  OP_GUARD({
    GemmArgs a;
    a.A = A; a.lda = K; a.W = W; a.ldw = K; a.bias = bias; a.C = C; a.ldc = N; a.resid = resid; a.ldr = N;
    a.row_map = row_map; a.M = M; a.N = N; a.K = K; a.act = act; a.c_f32 = c_f32;
    if (const char* e = getenv("ANYREF_OPTEST_LDW_PAD")) a.ldw = K + atoi(e);  // probe: padded weight rows
    if (t == 3 || t == 4) {  // A f32 [M,K] -> pairs; W bf16 / f16 [N,K] (K % 64 == 0); C f32 [*, N] either way (read back from pairs if !c_f32)
      hipStream_t st = (hipStream_t)stream;
      const bool h16 = t == 4;
      if (K % 64) throw std::runtime_error("op_gemm t=3/4: K % 64 != 0");
      TmpBuf As((size_t)M * K * 4);
      if (h16) launch_convert<sp16h>(reinterpret_cast<const float*>(A), K, As.p, K, M, K, st);
      else launch_convert<sp16>(reinterpret_cast<const float*>(A), K, As.p, K, M, K, st);
      a.A = As.p;
      if (c_f32) {
        if (h16) launch_gemm<sp16h>(a, st);
        else launch_gemm<sp16>(a, st);
      } else {
        int rows = M;
        if (row_map) {
          std::vector<int> h(M);
          HIP_TRY(hipMemcpy(h.data(), row_map, M * 4, hipMemcpyDeviceToHost));
          for (int v : h) rows = std::max(rows, v + 1);
        }
        TmpBuf Cs((size_t)rows * pad64(N) * 4);
        a.C = Cs.p; a.ldc = pad64(N);
        if (h16) launch_gemm<sp16h>(a, st);
        else launch_gemm<sp16>(a, st);
        launch_unsplit(Cs.p, pad64(N), reinterpret_cast<float*>(C), N, rows, N, st, h16);
      }
    }
    else if (t == 0) launch_gemm<float>(a, (hipStream_t)stream);
    else if (t == 2) launch_gemm<f16>(a, (hipStream_t)stream);
    else launch_gemm<bf16>(a, (hipStream_t)stream);
  });
}

int anyref_op_gemv(int t, void* stream, const float* x, const float* gain, float eps, const void* W,
                   const void* W2, const float* bias, float* y, const float* resid, int B, int N, int K, int act) {
  OP_GUARD({
    GemvArgs a;
    a.x = x; a.ldx = K; a.gain = gain; a.eps = eps; a.W = W; a.W2 = W2; a.bias = bias; a.y = y; a.resid = resid;
    a.ldy = N; a.B = B; a.N = N; a.K = K; a.act = act;
    if (const char* e = getenv("ANYREF_OPTEST_LDW_PAD")) a.ldw = K + atoi(e);  // probe: padded weight rows
    if (t == 3) launch_gemv<sp16>(a, (hipStream_t)stream);  // W bf16, x f32 staged as f32
    else if (t == 4) launch_gemv<sp16h>(a, (hipStream_t)stream);  // W f16
    else if (t == 0) launch_gemv<float>(a, (hipStream_t)stream);
    else if (t == 2) launch_gemv<f16>(a, (hipStream_t)stream);
    else launch_gemv<bf16>(a, (hipStream_t)stream);
  });
}

int anyref_op_gemv_xn(int t, void* stream, const float* x, const float* gain, float eps, const void* W, const void* W2,
                      const float* bias, float* y, const float* resid, int B, int N, int K, int act, float* xn_out,
                      const int32_t* xn_row_map, int xn_ld) {
  OP_GUARD({
    GemvArgs a;
    a.x = x; a.ldx = K; a.gain = gain; a.eps = eps; a.W = W; a.W2 = W2; a.bias = bias; a.y = y; a.resid = resid;
    a.ldy = N; a.B = B; a.N = N; a.K = K; a.act = act;
    a.xn_out = xn_out; a.xn_row_map = xn_row_map; a.xn_ld = xn_ld;
    if (t == 0) launch_gemv<float>(a, (hipStream_t)stream);
    else if (t == 1) launch_gemv<bf16>(a, (hipStream_t)stream);
    else if (t == 2) launch_gemv<f16>(a, (hipStream_t)stream);
    else if (t == 3) launch_gemv<sp16>(a, (hipStream_t)stream);
    else if (t == 4) launch_gemv<sp16h>(a, (hipStream_t)stream);
    else throw std::runtime_error("op_gemv_xn: t = 0 .. 4");
  });
}

int anyref_op_split_roundtrip(int t, void* stream, const float* in, float* out, void* hi_out, int rows, int cols) {
  OP_GUARD({
    if (t != 3 && t != 4) throw std::runtime_error("op_split_roundtrip: t = 3 / 4");
    hipStream_t st = (hipStream_t)stream;
    TmpBuf Ps((size_t)rows * pad64(cols) * 4);
    if (t == 4) launch_convert<sp16h>(in, cols, Ps.p, pad64(cols), rows, cols, st);
    else launch_convert<sp16>(in, cols, Ps.p, pad64(cols), rows, cols, st);
    launch_unsplit(Ps.p, pad64(cols), out, cols, rows, cols, st, t == 4);
    if (hi_out) {  // the hi term alone: widen the 16-bit words at sp_col(c) on the host side of the test
      std::vector<uint16_t> h((size_t)rows * pad64(cols) * 2);
      HIP_TRY(hipStreamSynchronize(st));
      HIP_TRY(hipMemcpy(h.data(), Ps.p, h.size() * 2, hipMemcpyDeviceToHost));
      std::vector<uint16_t> hi((size_t)rows * cols);
      for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) hi[(size_t)r * cols + c] = h[(size_t)r * pad64(cols) * 2 + sp_col(c)];
      HIP_TRY(hipMemcpy(hi_out, hi.data(), hi.size() * 2, hipMemcpyHostToDevice));
    }
  });
}

int anyref_op_rope_table(int S, int hd, float theta, float* out_host) { OP_GUARD(rope_table(S, hd, theta, out_host)); }

int anyref_op_decode_attn(int t, void* stream, const float* qkv, int B, int H, int hd, const int32_t* pos,
                          const float* cs_tab, void* kc, void* vc, int maxS, float scale, float* out, void* q_keep,
                          int force_fallback) {
  OP_GUARD({
    if (t != 0 && t != 1 && t != 2) throw std::runtime_error("op_decode_attn: t = 0 / 1 / 2");
    hipStream_t st = (hipStream_t)stream;
    // kv_len[b] = pos[b] + 1 (the model's kvlen_dev_, written by the argmax of the step before)
    std::vector<int> h(B);
    HIP_TRY(hipMemcpy(h.data(), pos, (size_t)B * 4, hipMemcpyDeviceToHost));
    for (int& v : h) v += 1;
    TmpBuf kv_len((size_t)B * 4);
    TmpBuf q_tmp((size_t)B * H * hd * 4);
    HIP_TRY(hipMemcpy(kv_len.p, h.data(), (size_t)B * 4, hipMemcpyHostToDevice));
    if (t == 0)
      launch_decode_step_attn<float>(qkv, B, H, hd, pos, (const int*)kv_len.p, cs_tab, q_tmp.p, kc, vc, maxS, scale, out,
                                     q_keep, st, force_fallback != 0);
    else if (t == 2)
      launch_decode_step_attn<f16>(qkv, B, H, hd, pos, (const int*)kv_len.p, cs_tab, q_tmp.p, kc, vc, maxS, scale, out,
                                   q_keep, st, force_fallback != 0);
    else
      launch_decode_step_attn<bf16>(qkv, B, H, hd, pos, (const int*)kv_len.p, cs_tab, q_tmp.p, kc, vc, maxS, scale, out,
                                    q_keep, st, force_fallback != 0);
  });
}

int anyref_op_seg_rephrase(int t, void* stream, const void* q_keep, const void* kc, int maxS, int H, int hd, const float* hidden,
                           const int32_t* items, int n_items, int max_span, int span_cap, float* scratch, float scale,
                           float weight, float* y, int32_t* launched) {
  OP_GUARD({
    if (t != 0 && t != 1 && t != 2) throw std::runtime_error("op_seg_rephrase: t = 0 / 1 / 2");
    if (!q_keep || !kc || !hidden || !items || !scratch || !y || !launched) throw std::runtime_error("op_seg_rephrase: null argument");
    if (n_items < 0 || maxS < 1 || H < 1 || hd < 1) throw std::runtime_error("op_seg_rephrase: bad shape");
    hipStream_t st = (hipStream_t)stream;
    bool ok;
    if (t == 0)
      ok = launch_seg_rephrase<float>(q_keep, kc, maxS, H, hd, hidden, items, n_items, max_span, span_cap, scratch, scale, weight, y, st);
    else if (t == 2)
      ok = launch_seg_rephrase<f16>(q_keep, kc, maxS, H, hd, hidden, items, n_items, max_span, span_cap, scratch, scale, weight, y, st);
    else
      ok = launch_seg_rephrase<bf16>(q_keep, kc, maxS, H, hd, hidden, items, n_items, max_span, span_cap, scratch, scale, weight, y, st);
    *launched = ok ? 1 : 0;
  });
}

int anyref_op_rephrase_chain(int t, void* stream, const void* q_keep, const void* kc, int maxS, int H, int hd,
                             const float* hidden, int b, int e0, int s0, const int32_t* kv_len, float* attn_row, float scale,
                             float weight, float* y) {
  OP_GUARD({
    if (t != 0 && t != 1 && t != 2) throw std::runtime_error("op_rephrase_chain: t = 0 / 1 / 2");
    if (!q_keep || !kc || !hidden || !kv_len || !attn_row || !y) throw std::runtime_error("op_rephrase_chain: null argument");
    if (b < 0 || s0 < 0 || e0 <= s0 || e0 >= maxS) throw std::runtime_error("op_rephrase_chain: bad item");
    hipStream_t st = (hipStream_t)stream;
    const int D = H * hd;
    const size_t es = t == 0 ? 4 : 2;
    const char* q = (const char*)q_keep + ((size_t)b * maxS + e0) * D * es;
    const char* k = (const char*)kc + (size_t)b * maxS * D * es;
    if (t == 0) launch_attn_row_mean<float>(q, 0, hd, k, 0, D, hd, kv_len, 1, H, hd, scale, attn_row, maxS, st);
    else if (t == 2) launch_attn_row_mean<f16>(q, 0, hd, k, 0, D, hd, kv_len, 1, H, hd, scale, attn_row, maxS, st);
    else launch_attn_row_mean<bf16>(q, 0, hd, k, 0, D, hd, kv_len, 1, H, hd, scale, attn_row, maxS, st);
    launch_rephrase(hidden + (size_t)b * maxS * D, D, attn_row, s0, e0, weight, y, st);
  });
}

int anyref_op_rope_cache(int t, void* stream, const void* qkv, const float* slab0, const float* slab1, int B, int S, int H,
                         int hd, const int32_t* pos0, const int32_t* lens, const float* cs_tab, void* q_out, void* kc,
                         void* vc, int maxS, void* q_keep) {
  OP_GUARD({
    hipStream_t st = (hipStream_t)stream;
    if (t != 0 && t != 1 && t != 2) throw std::runtime_error("op_rope_cache: t = 0 / 1 / 2");
    if (slab0) {
      if (t == 0) launch_rope_cache_slabs<float>(slab0, slab1, B, S, H, hd, pos0, lens, cs_tab, q_out, kc, vc, maxS, q_keep, st);
      else if (t == 2) launch_rope_cache_slabs<f16>(slab0, slab1, B, S, H, hd, pos0, lens, cs_tab, q_out, kc, vc, maxS, q_keep, st);
      else launch_rope_cache_slabs<bf16>(slab0, slab1, B, S, H, hd, pos0, lens, cs_tab, q_out, kc, vc, maxS, q_keep, st);
    } else if (t == 0)
      launch_rope_cache<float>(qkv, B, S, H, hd, pos0, lens, cs_tab, q_out, kc, vc, maxS, q_keep, st);
    else if (t == 2)
      launch_rope_cache<f16>(qkv, B, S, H, hd, pos0, lens, cs_tab, q_out, kc, vc, maxS, q_keep, st);
    else
      launch_rope_cache<bf16>(qkv, B, S, H, hd, pos0, lens, cs_tab, q_out, kc, vc, maxS, q_keep, st);
  });
}

int anyref_op_argmax(void* stream, const float* x, int M, int N, int ldx, int64_t* out, int32_t* pos, const void* table,
                     int is_bf16, int D, int maxS, float* x_next, int32_t* row_map, int32_t* kvlen) {
  OP_GUARD({
    if (table && (is_bf16 < 0 || is_bf16 > 2)) throw std::runtime_error("op_argmax: table dtype 0 / 1 / 2");
    if (table)
      launch_argmax_next(x, M, N, ldx, out, pos, table, is_bf16, D, maxS, x_next, row_map, kvlen, (hipStream_t)stream);
    else
      launch_argmax(x, M, N, ldx, out, (hipStream_t)stream, pos);
  });
}

int anyref_op_token_scores(void* stream, const float* logits, int M, int N, int ldx, const int32_t* dst, float* logprob,
                           float* gap, int64_t* id) {
  OP_GUARD({
    if (!logits || !logprob || !gap) throw std::runtime_error("op_token_scores: null argument");
    if (M < 1) throw std::runtime_error("op_token_scores: M >= 1 rows");
    if (N < 2) throw std::runtime_error("op_token_scores: a row needs N >= 2 entries (the gap is to the second one)");
    if (ldx < N) throw std::runtime_error("op_token_scores: ldx < N");
    launch_token_scores(logits, M, N, ldx, dst, logprob, gap, id, (hipStream_t)stream);
  });
}

int anyref_op_mask_report(void* stream, const float* logits, int n, int H, int W, float offset, int32_t* records,
                          uint32_t* packed) {
  OP_GUARD(launch_mask_report(logits, n, H, W, offset, records, packed, (hipStream_t)stream));
}

int anyref_op_draft_accept(void* stream, const float* logits, int B, int k, int N, int ldx, int64_t* p, const int64_t* draft,
                           const int32_t* draft_lens, int64_t* next, int32_t* pos, int64_t* tokens, int32_t* accepted,
                           const void* table, int dtype, int D, int maxS, float* x_next, int32_t* row_map, int32_t* kvlen) {
  OP_GUARD({
    if (dtype < 0 || dtype > 2) throw std::runtime_error("op_draft_accept: table dtype 0 / 1 / 2");
    if (!logits || !p || !draft || !draft_lens || !next || !pos || !tokens || !accepted || !table || !x_next || !row_map || !kvlen)
      throw std::runtime_error("op_draft_accept: null argument");
    launch_draft_accept(logits, B, k, N, ldx, p, draft, draft_lens, next, pos, tokens, accepted, table, dtype, D, maxS, x_next,
                        row_map, kvlen, (hipStream_t)stream);
  });
}

int anyref_op_kv_broadcast(void* stream, void* kc, void* vc, int layers, int rows, int maxS, int row_elems, int elem_size,
                           int P, int r0, int r1) {
  OP_GUARD({
    if (!kc) throw std::runtime_error("op_kv_broadcast: null argument");
    if (elem_size != 2 && elem_size != 4) throw std::runtime_error("op_kv_broadcast: elem_size 2 / 4");
    if (layers < 1 || rows < 1 || maxS < 1 || row_elems < 1) throw std::runtime_error("op_kv_broadcast: bad shape");
    const int64_t row_bytes = (int64_t)row_elems * elem_size;
    launch_kv_broadcast(kc, layers, vc, vc ? layers : 0, (int64_t)rows * maxS * row_bytes, rows, maxS, row_bytes, P, r0, r1,
                        (hipStream_t)stream);
  });
}

int anyref_op_kv_gather(void* stream, void* kc, void* vc, int layers, int rows, int maxS, void* pool, int n_slots, int maxP,
                        int row_elems, int elem_size, const int32_t* table, int n, int pack) {
  OP_GUARD({
    if (!kc || !pool || (n > 0 && !table)) throw std::runtime_error("op_kv_gather: null argument");
    if (elem_size != 2 && elem_size != 4) throw std::runtime_error("op_kv_gather: elem_size 2 / 4");
    if (layers < 1 || rows < 1 || maxS < 1 || row_elems < 1 || n_slots < 1 || maxP < 1 || n < 0)
      throw std::runtime_error("op_kv_gather: bad shape");
    const int64_t row_bytes = (int64_t)row_elems * elem_size;
    std::vector<KvGatherItem> items(n);
    for (int i = 0; i < n; ++i) items[i] = KvGatherItem{table[4 * i], table[4 * i + 1], table[4 * i + 2], table[4 * i + 3]};
    launch_kv_gather(kc, layers, vc, vc ? layers : 0, (int64_t)rows * maxS * row_bytes, rows, maxS, pool, n_slots, maxP, row_bytes,
                     items.data(), n, pack != 0, (hipStream_t)stream);
  });
}

int anyref_op_norm(int t, void* stream, const float* x, const float* gain, const float* bias, float* y, int M,
                   int D, float eps, int rms) {
  OP_GUARD({
    NormArgs a;
    a.x = x; a.ldx = D; a.gain = gain; a.bias = bias; a.y = y; a.ldy = D; a.M = M; a.D = D; a.eps = eps;
    a.rms = rms; a.y_f32 = 1;
    if (t == 3 || t == 4) {  // the norm writes pairs; y gets hi + lo
      TmpBuf Ys((size_t)M * pad64(D) * 4);
      a.y = Ys.p; a.ldy = pad64(D); a.y_f32 = 0;
      if (t == 4) launch_norm<sp16h>(a, (hipStream_t)stream);
      else launch_norm<sp16>(a, (hipStream_t)stream);
      launch_unsplit(Ys.p, pad64(D), y, D, M, D, (hipStream_t)stream, t == 4);
    } else
    if (t == 0) launch_norm<float>(a, (hipStream_t)stream);
    else if (t == 2) launch_norm<f16>(a, (hipStream_t)stream);
    else launch_norm<bf16>(a, (hipStream_t)stream);
  });
}

int anyref_op_attention(int t, void* stream, const void* q, const void* k, const void* v, void* o, int B, int H,
                        int Sq, int Sk, int hd, float scale, int causal, const int32_t* kv_len,
                        const float* rel_h, const float* rel_w, int kh, int kw) {
  OP_GUARD({
    AttnArgs a;
    a.Q = q; a.K = k; a.V = v; a.O = o;
    a.q_bs = (int64_t)Sq * H * hd; a.q_rs = H * hd; a.q_hs = hd;
    a.k_bs = a.v_bs = (int64_t)Sk * H * hd; a.k_rs = a.v_rs = H * hd; a.k_hs = a.v_hs = hd;
    a.o_bs = (int64_t)Sq * H * hd; a.o_rs = H * hd; a.o_hs = hd;
    a.B = B; a.H = H; a.Sq = Sq; a.Sk = Sk; a.hd = hd; a.scale = scale; a.causal = causal; a.kv_len = kv_len;
    a.rel_h = rel_h; a.rel_w = rel_w; a.kh = kh; a.kw = kw;
    if (t == 3 || t == 4) {  // f32 operands, pair-typed output rows [B*Sq, H*hd] (H*hd % 64 == 0; t = 4: f16 terms); o gets hi + lo
      if ((H * hd) % 64) throw std::runtime_error("op_attention t=3/4: H * hd % 64 != 0");
      TmpBuf Os((size_t)B * Sq * H * hd * 4);
      a.O = Os.p; a.o_split = t == 4 ? 2 : 1; a.sp16 = 1;
      launch_attention<float>(a, (hipStream_t)stream);
      launch_unsplit(Os.p, H * hd, reinterpret_cast<float*>(o), H * hd, B * Sq, H * hd, (hipStream_t)stream, t == 4);
    } else
    if (t == 0) launch_attention<float>(a, (hipStream_t)stream);
    else if (t == 2) launch_attention<f16>(a, (hipStream_t)stream);
    else launch_attention<bf16>(a, (hipStream_t)stream);
  });
}

int anyref_op_attention_tab(int t, void* stream, const void* q, const void* k, const void* v, void* o, int B, int H, int S,
                            int hd, float scale, const void* tab_h, const void* tab_w, int tab_ld, int kh, int kw) {
  OP_GUARD({
    AttnArgs a;
    a.Q = q; a.K = k; a.V = v; a.O = o;
    a.q_bs = a.k_bs = a.v_bs = a.o_bs = (int64_t)S * H * hd;
    a.q_rs = a.k_rs = a.v_rs = a.o_rs = H * hd; a.q_hs = a.k_hs = a.v_hs = a.o_hs = hd;
    a.B = B; a.H = H; a.Sq = S; a.Sk = S; a.hd = hd; a.scale = scale;
    a.rel_tab_h = tab_h; a.rel_tab_w = tab_w; a.rel_tab_ld = tab_ld; a.kh = kh; a.kw = kw;
    if (t == 3 || t == 4) {  // split-pair attention: f32 operands and f32 tables, pair-typed output rows; o gets hi + lo
      if ((H * hd) % 64) throw std::runtime_error("op_attention_tab t=3/4: H * hd % 64 != 0");
      if (!attention_takes_rel_tables(4, hd, S, S, kh, kw, true)) throw std::runtime_error("op_attention_tab t=3/4: not a window shape");
      TmpBuf Os((size_t)B * S * H * hd * 4);
      a.O = Os.p; a.o_split = t == 4 ? 2 : 1; a.sp16 = 1;
      launch_attention<float>(a, (hipStream_t)stream);
      launch_unsplit(Os.p, H * hd, reinterpret_cast<float*>(o), H * hd, B * S, H * hd, (hipStream_t)stream, t == 4);
    } else
    if (t == 2) launch_attention<f16>(a, (hipStream_t)stream);
    else launch_attention<bf16>(a, (hipStream_t)stream);
  });
}

int anyref_op_gemm_gather(int t, void* stream, const void* A, const int32_t* a_row_map, const void* W, const float* bias,
                          void* C, const float* resid, int M, int N, int K, int c_f32) {
  OP_GUARD({
    GemmArgs a;
    a.A = A; a.lda = K; a.W = W; a.ldw = K; a.bias = bias; a.C = C; a.ldc = N; a.resid = resid; a.ldr = N;
    a.a_row_map = a_row_map; a.M = M; a.N = N; a.K = K; a.c_f32 = c_f32;
    if (t == 2) launch_gemm<f16>(a, (hipStream_t)stream);
    else if (t == 1) launch_gemm<bf16>(a, (hipStream_t)stream);
    else throw std::runtime_error("gemm_gather: 16-bit types only");
  });
}

int anyref_op_attention_relp(int t, void* stream, const void* q, const void* k, const void* v, void* o, int B, int H, int S,
                             int hd, float scale, const float* rel_p, int rel_ld, int kh, int kw) {
  OP_GUARD({
    AttnArgs a;
    a.Q = q; a.K = k; a.V = v; a.O = o;
    a.q_bs = a.k_bs = a.v_bs = a.o_bs = (int64_t)S * H * hd;
    a.q_rs = a.k_rs = a.v_rs = a.o_rs = H * hd; a.q_hs = a.k_hs = a.v_hs = a.o_hs = hd;
    a.B = B; a.H = H; a.Sq = S; a.Sk = S; a.hd = hd; a.scale = scale;
    a.rel_p = rel_p; a.rel_ld = rel_ld; a.rel_hs = (int64_t)B * S * rel_ld; a.kh = kh; a.kw = kw;
    if (t == 3 || t == 4) {  // split-pair attention: f32 operands, pair-typed output rows; o gets hi + lo
      if ((H * hd) % 64) throw std::runtime_error("op_attention_relp t=3/4: H * hd % 64 != 0");
      TmpBuf Os((size_t)B * S * H * hd * 4);
      a.O = Os.p; a.o_split = t == 4 ? 2 : 1; a.sp16 = 1;
      launch_attention<float>(a, (hipStream_t)stream);
      launch_unsplit(Os.p, H * hd, reinterpret_cast<float*>(o), H * hd, B * S, H * hd, (hipStream_t)stream, t == 4);
    } else
    if (t == 0) launch_attention<float>(a, (hipStream_t)stream);
    else if (t == 2) launch_attention<f16>(a, (hipStream_t)stream);
    else launch_attention<bf16>(a, (hipStream_t)stream);
  });
}

int anyref_op_rel_pos(int t, void* stream, const void* q, const float* tab_h, const float* tab_w, int B, int H,
                      int size, int hd, float* rel_h, float* rel_w) {
  OP_GUARD({
    const int64_t S = (int64_t)size * size;
    if (t == 0)
      launch_rel_pos<float>(q, S * H * hd, H * hd, hd, tab_h, tab_w, B, H, size, hd, rel_h, rel_w, (hipStream_t)stream);
    else
      launch_rel_pos<bf16>(q, S * H * hd, H * hd, hd, tab_h, tab_w, B, H, size, hd, rel_h, rel_w, (hipStream_t)stream);
  });
}

int anyref_op_postprocess(void* stream, const float* low, int n, int lh, int lw, int S, int rh, int rw, int H, int W,
                          float* out) {
  OP_GUARD(launch_postprocess(low, (int64_t)lh * lw, n, lh, lw, S, rh, rw, H, W, out, (hipStream_t)stream));
}

int anyref_op_gemm_fp8(void* stream, const void* A, const uint8_t* W8, const float* scale, const float* bias, void* C,
                       const float* resid, int M, int N, int K, int act, int c_f32) {
  OP_GUARD({
    GemmArgs a;
    a.A = A; a.lda = K; a.W = W8; a.ldw = K; a.w_fp8 = 1; a.col_scale = scale; a.bias = bias; a.C = C; a.ldc = N;
    a.resid = resid; a.ldr = N; a.M = M; a.N = N; a.K = K; a.act = act; a.c_f32 = c_f32;
    launch_gemm<bf16>(a, (hipStream_t)stream);
  });
}

int anyref_op_quant_fp8(void* stream, const float* src, int N, int K, uint8_t* q, float* scale) {
  OP_GUARD(launch_quant_fp8_rows(src, K, N, K, q, K, scale, (hipStream_t)stream));
}

int anyref_op_gemv_fp8(void* stream, const float* x, const float* gain, float eps, const uint8_t* W,
                       const uint8_t* W2, const float* scale, const float* scale2, float* y, const float* resid,
                       int B, int N, int K) {
  OP_GUARD({
    GemvArgs a;
    a.x = x; a.ldx = K; a.gain = gain; a.eps = eps; a.W = W; a.W2 = W2; a.wscale = scale; a.wscale2 = scale2;
    a.w_fp8 = 1; a.y = y; a.resid = resid; a.ldy = N; a.B = B; a.N = N; a.K = K;
    launch_gemv<bf16>(a, (hipStream_t)stream);
  });
}

int anyref_op_quant_int4(void* stream, const float* src, int N, int K, uint8_t* q, void* scale_bf16) {
  OP_GUARD(launch_quant_int4_rows(src, K, N, K, q, (K + 127) / 128 * 64, scale_bf16, (K + 127) / 128, (hipStream_t)stream));
}

int anyref_op_lora_merge(int t, void* stream, const float* base_f32, int d_in, int N, int K, const float* A, const float* B, int r,
                         float scaling, void* dst, int ld, int row_stride, uint64_t* counts) {
  OP_GUARD({
    if (r < 1) throw std::runtime_error("anyref_op_lora_merge: LoRA rank " + std::to_string(r) + " is outside 1 .. 64");
    auto* c = reinterpret_cast<unsigned long long*>(counts);
    if (t == 0) launch_lora_merge<float>(base_f32, d_in, N, K, A, B, r, scaling, dst, ld, row_stride, c, (hipStream_t)stream, "anyref_op_lora_merge");
    else if (t == 1) launch_lora_merge<bf16>(base_f32, d_in, N, K, A, B, r, scaling, dst, ld, row_stride, c, (hipStream_t)stream, "anyref_op_lora_merge");
    else if (t == 2) launch_lora_merge<f16>(base_f32, d_in, N, K, A, B, r, scaling, dst, ld, row_stride, c, (hipStream_t)stream, "anyref_op_lora_merge");
    else throw std::runtime_error("anyref_op_lora_merge: t = 0 (f32), 1 (bf16) or 2 (f16)");
  });
}

int anyref_op_dequant_int4(void* stream, const uint8_t* q, const void* scale_bf16, int N, int K, void* out_bf16) {
  OP_GUARD(launch_dequant_int4_rows(q, (K + 127) / 128 * 64, scale_bf16, (K + 127) / 128, N, K, out_bf16, K, (hipStream_t)stream));
}

int anyref_op_gemm_int4(void* stream, const void* A, const uint8_t* W4, const void* scale_bf16, const float* bias, void* C,
                        const float* resid, int M, int N, int K, int act, int c_f32, int swiglu) {
  OP_GUARD({
    TagScope tags((hipStream_t)stream);
    GemmArgs a;
    a.A = A; a.lda = K; a.W = W4; a.ldw = (K + 127) / 128 * 64; a.w_int4 = 1; a.gscale = scale_bf16; a.ld_gscale = (K + 127) / 128;
    a.bias = bias; a.C = C; a.ldc = swiglu ? N / 2 : N; a.resid = resid; a.ldr = N; a.M = M; a.N = N; a.K = K; a.act = act;
    a.c_f32 = c_f32; a.swiglu_pairs = swiglu ? 1 : 0;
    launch_gemm<bf16>(a, (hipStream_t)stream);
  });
}

int anyref_op_gemv_int4(void* stream, const float* x, const float* gain, float eps, const uint8_t* W, const uint8_t* W2,
                        const void* scale_bf16, const void* scale2_bf16, float* y, const float* resid, int B, int N, int K) {
  OP_GUARD({
    GemvArgs a;
    a.x = x; a.ldx = K; a.gain = gain; a.eps = eps; a.W = W; a.W2 = W2; a.gscale = scale_bf16; a.gscale2 = scale2_bf16;
    a.w_int4 = 1; a.ldw = (K + 127) / 128 * 64; a.ld_gscale = (K + 127) / 128; a.y = y; a.resid = resid; a.ldy = N; a.B = B;
    a.N = N; a.K = K;
    launch_gemv<bf16>(a, (hipStream_t)stream);
  });
}

int anyref_op_iou_counts(void* stream, const float* logits, const uint8_t* target, int n, int64_t hw,
                         int64_t* counts) {
  OP_GUARD(launch_iou_counts(logits, target, n, hw, counts, (hipStream_t)stream));
}

int anyref_op_avs_counts(void* stream, const float* logits, const uint8_t* target, int n, int64_t hw,
                         const float* cuts, int nth, float cut_pred, int64_t* conf, int64_t* hist) {
  OP_GUARD(launch_avs_counts(logits, target, n, hw, cuts, nth, cut_pred, conf, hist, (hipStream_t)stream));
}

int anyref_op_sam_preprocess(void* stream, const uint8_t* img, int h, int w, int S, const float* mean3,
                             const float* std3, float* out) {
  OP_GUARD(launch_sam_preprocess(img, h, w, S, mean3, std3, out, (hipStream_t)stream));
}

int anyref_op_pil_resample_u8(void* stream, const uint8_t* in, int H, int W, int C, uint8_t* tmp, uint8_t* out, int ow,
                              int oh, const int32_t* xbounds, const int32_t* xk, int kx, const int32_t* ybounds,
                              const int32_t* yk, int ky) {
  OP_GUARD(launch_pil_resample_u8(in, H, W, C, tmp, out, ow, oh, xbounds, xk, kx, ybounds, yk, ky, (hipStream_t)stream));
}

int anyref_op_pool_ref_tokens(void* stream, const float* feats, int n, int L, int H, int n_out, float* out) {
  OP_GUARD(launch_pool_ref_tokens(feats, n, L, H, n_out, out, (hipStream_t)stream));
}

int anyref_op_kaldi_fbank(void* stream, const float* wave, int C, int T, int win, int shift, int padded, float preemph,
                          const float* banks, int n_mel, const double* tw, double* scratch, int target_len, float mean,
                          float stdv, float* out) {
  OP_GUARD(launch_kaldi_fbank(wave, C, T, win, shift, padded, preemph, banks, n_mel, tw, scratch, target_len, mean, stdv, out,
                              (hipStream_t)stream));
}
int anyref_op_clip_finish(void* stream, const uint8_t* img, int ih, int iw, int y0, int x0, int h, int w, int S,
                          const float* mean3, const float* std3, float* out) {
  OP_GUARD(launch_clip_finish(img, ih, iw, y0, x0, h, w, S, mean3, std3, out, (hipStream_t)stream));
}

// ---- glue kernels and the skinny f32 GEMV (tests/test_gpu_glue_ops.py) -------------------------------------------------
int anyref_op_gemv_skinny(void* stream, const float* x, int ldx, const float* W, const float* bias, float* y, int ldy,
                          const float* resid, int B, int N, int K, int act) {
  OP_GUARD({
    if (!x || !W || !y) throw std::runtime_error("op_gemv_skinny: null argument");
    if (N < 1 || K < 4 || ldx < K || ldy < N) throw std::runtime_error("op_gemv_skinny: N >= 1, K >= 4, ldx >= K, ldy >= N");
    GemvArgs a;
    a.x = x; a.ldx = ldx; a.W = W; a.bias = bias; a.y = y; a.ldy = ldy; a.resid = resid; a.B = B; a.N = N; a.K = K; a.act = act;
    launch_gemv_skinny_f32(a, (hipStream_t)stream);
  });
}

int anyref_op_upscale1(int t, void* stream, const float* tmp, int n, int g, int C, const float* ln_g, const float* ln_b, float eps,
                       void* out) {
  OP_GUARD({
    if (t != 0) throw std::runtime_error("op_upscale1: t = 0 (the f32 output is the only form the model runs)");
    if (n < 1 || g < 1 || C < 1) throw std::runtime_error("op_upscale1: bad shape");
    launch_upscale1<float>(tmp, n, g, C, ln_g, ln_b, eps, out, (hipStream_t)stream);
  });
}

int anyref_op_upscale2_masks(void* stream, const float* tmp, const float* hyper, int n, int ntok, int g2, int C, float* masks) {
  OP_GUARD({
    if (n < 1 || ntok < 1 || g2 < 1 || C < 1) throw std::runtime_error("op_upscale2_masks: bad shape");
    launch_upscale2_masks(tmp, hyper, n, ntok, g2, C, masks, (hipStream_t)stream);
  });
}

int anyref_op_dense_pe(void* stream, const float* gauss, int g, int F, float* out) {
  OP_GUARD({
    if (g < 1 || F < 1) throw std::runtime_error("op_dense_pe: bad shape");
    launch_dense_pe(gauss, g, F, out, (hipStream_t)stream);
  });
}

int anyref_op_build_tokens(void* stream, const float* out_tokens, int n_out, const float* pred, int n, int C, float* tokens) {
  OP_GUARD(launch_build_tokens(out_tokens, n_out, pred, n, C, tokens, (hipStream_t)stream));
}

int anyref_op_prompt_tokens(void* stream, const float* out_tokens, int n_out, const float* points, const int32_t* labels, int P,
                            const float* boxes, const float* text, const float* gauss, const float* emb5, int n, int C, int S,
                            float* tokens, int max_wg) {
  OP_GUARD(launch_prompt_tokens(out_tokens, n_out, points, labels, P, boxes, text, gauss, emb5, n, C, S, tokens,
                                (hipStream_t)stream, max_wg));
}

int anyref_op_mask_prompt_embed(void* stream, const float* mask, const float* image_emb, const float* w1, const float* b1,
                                const float* ln1_g, const float* ln1_b, const float* w2, const float* b2, const float* ln2_g,
                                const float* ln2_b, const float* w3, const float* b3, int n, int g, int C, int c1, int c2,
                                float* keys, int max_wg) {
  OP_GUARD({
    MaskDownW W;
    W.w1 = w1; W.b1 = b1; W.g1 = ln1_g; W.be1 = ln1_b; W.w2 = w2; W.b2 = b2; W.g2 = ln2_g; W.be2 = ln2_b; W.w3 = w3; W.b3 = b3;
    W.c1 = c1; W.c2 = c2;
    launch_mask_prompt_embed(mask, image_emb, W, n, g, C, keys, (hipStream_t)stream, max_wg);
  });
}

int anyref_op_add_rows(void* stream, const float* a, const float* b, int bmod, float* out, int M, int D) {
  OP_GUARD({
    if (bmod < 1) throw std::runtime_error("op_add_rows: bmod >= 1");
    launch_add_rows(a, b, bmod, out, M, D, (hipStream_t)stream);
  });
}

int anyref_op_add_vec(void* stream, const float* a, const float* v, float* out, int M, int D) {
  OP_GUARD(launch_add_vec(a, v, out, M, D, (hipStream_t)stream));
}

int anyref_op_embed_splice(void* stream, const int64_t* ids, const int32_t* lens, int B, int Lmax, const void* table, int dtype,
                           int vocab, const float* img_feat, int n_img, float* x, int Smax, int D, int32_t* out_len) {
  OP_GUARD({
    if (dtype < 0 || dtype > 2) throw std::runtime_error("op_embed_splice: table dtype 0 / 1 / 2");
    if (B < 1 || Lmax < 1 || n_img < 1 || Smax < 1 || D < 1) throw std::runtime_error("op_embed_splice: bad shape");
    launch_embed_splice(ids, lens, B, Lmax, table, dtype, vocab, img_feat, n_img, x, Smax, D, out_len, (hipStream_t)stream);
  });
}

int anyref_op_scatter_rows(void* stream, const float* rows, const int32_t* dst_b, const int32_t* dst_pos, int n, float* x, int Smax,
                           int D) {
  OP_GUARD(launch_scatter_rows(rows, dst_b, dst_pos, n, x, Smax, D, (hipStream_t)stream));
}

int anyref_op_gather_rows(void* stream, const float* x, int Smax, int D, const int32_t* b, const int32_t* pos, int n, float* out) {
  OP_GUARD(launch_gather_rows(x, Smax, D, b, pos, n, out, (hipStream_t)stream));
}

int anyref_op_embed_rows(void* stream, const int64_t* ids, int B, const void* table, int dtype, int D, float* x) {
  OP_GUARD({
    if (dtype < 0 || dtype > 2) throw std::runtime_error("op_embed_rows: table dtype 0 / 1 / 2");
    if (B < 1) throw std::runtime_error("op_embed_rows: B >= 1");
    launch_embed_rows(ids, B, table, dtype, D, x, (hipStream_t)stream);
  });
}

int anyref_op_im2col_patch(int t, void* stream, const float* img, int B, int S, int p, void* out, int Kp) {
  OP_GUARD({
    hipStream_t st = (hipStream_t)stream;
    if (B < 1 || p < 1 || S < p || S % p || Kp < 3 * p * p) throw std::runtime_error("op_im2col_patch: S % p == 0, Kp >= 3 p^2");
    const int rows = B * (S / p) * (S / p);
    if (t == 3 || t == 4)
      im2col_pairs(t, rows, Kp, reinterpret_cast<float*>(out), st, [&](void* ps) {
        if (t == 4) launch_im2col_patch<sp16h>(img, B, S, p, ps, Kp, st);
        else launch_im2col_patch<sp16>(img, B, S, p, ps, Kp, st);
      });
    else
      by_type(t, [&](auto T0) {
        using T = decltype(T0);
        if constexpr (!is_split<T>::value) launch_im2col_patch<T>(img, B, S, p, out, Kp, st);
      });
  });
}

int anyref_op_im2col_3x3(int t, void* stream, const void* in, int B, int g, int C, void* out) {
  OP_GUARD({
    hipStream_t st = (hipStream_t)stream;
    if (B < 1 || g < 1 || C < 1) throw std::runtime_error("op_im2col_3x3: bad shape");
    const int rows = B * g * g;
    if (t == 3 || t == 4) {  // the kernel reads pairs too: in f32 [rows, C] -> pairs
      if (C % 64) throw std::runtime_error("op_im2col_3x3 t=3/4: C % 64 != 0");
      TmpBuf Is((size_t)rows * C * 4);
      if (t == 4) launch_convert<sp16h>(reinterpret_cast<const float*>(in), C, Is.p, C, rows, C, st);
      else launch_convert<sp16>(reinterpret_cast<const float*>(in), C, Is.p, C, rows, C, st);
      im2col_pairs(t, rows, 9 * C, reinterpret_cast<float*>(out), st, [&](void* ps) {
        if (t == 4) launch_im2col_3x3<sp16h>(Is.p, B, g, C, ps, st);
        else launch_im2col_3x3<sp16>(Is.p, B, g, C, ps, st);
      });
    } else
      by_type(t, [&](auto T0) {
        using T = decltype(T0);
        if constexpr (!is_split<T>::value) launch_im2col_3x3<T>(in, B, g, C, out, st);
      });
  });
}

int anyref_op_im2col_conv1(int t, void* stream, const float* img, int n, int Hh, int Ww, int k, int st_, void* out) {
  OP_GUARD({
    hipStream_t st = (hipStream_t)stream;
    if (n < 1 || k < 1 || st_ < 1 || Hh < k || Ww < k) throw std::runtime_error("op_im2col_conv1: bad shape");
    const int rows = n * ((Hh - k) / st_ + 1) * ((Ww - k) / st_ + 1);
    if (t == 3 || t == 4)
      im2col_pairs(t, rows, k * k, reinterpret_cast<float*>(out), st, [&](void* ps) {
        if (t == 4) launch_im2col_conv1<sp16h>(img, n, Hh, Ww, k, st_, ps, st);
        else launch_im2col_conv1<sp16>(img, n, Hh, Ww, k, st_, ps, st);
      });
    else
      by_type(t, [&](auto T0) {
        using T = decltype(T0);
        if constexpr (!is_split<T>::value) launch_im2col_conv1<T>(img, n, Hh, Ww, k, st_, out, st);
      });
  });
}

int anyref_op_clip_assemble(void* stream, const float* patch, const float* cls, const float* pos, float* x, int B, int n, int D,
                            int rows) {
  OP_GUARD({
    if (B < 1 || n < 1 || D < 1 || (rows > 0 && rows < n + 1)) throw std::runtime_error("op_clip_assemble: rows = 0 or >= n + 1");
    launch_clip_assemble(patch, cls, pos, x, B, n, D, (hipStream_t)stream, rows);
  });
}

int anyref_op_l2norm_scale(void* stream, const float* x, int rows, int D, float scale, float* y) {
  OP_GUARD(launch_l2norm_scale(x, rows, D, scale, y, (hipStream_t)stream));
}

int anyref_op_to_f32(void* stream, const void* in, int dtype, float* out, int64_t n) {
  OP_GUARD({
    if (dtype < 0 || dtype > 2) throw std::runtime_error("op_to_f32: dtype 0 / 1 / 2");
    launch_to_f32(in, dtype, out, n, (hipStream_t)stream);
  });
}

int anyref_op_dequant_fp8(void* stream, const uint8_t* q, int ldq, const float* scale, int N, int K, void* out_bf16, int ldo) {
  OP_GUARD({
    if (ldq < K || ldo < K) throw std::runtime_error("op_dequant_fp8: ldq >= K, ldo >= K");
    launch_dequant_fp8_rows(q, ldq, scale, N, K, out_bf16, ldo, (hipStream_t)stream);
  });
}
}
