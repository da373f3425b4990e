/*
 * anyref_hip_ops.h — kernel-level entry points of libanyref_hip.so used by the op tests (tests/test_gpu_*ops*.py,
 * tests/test_gpu_gemm_forms.py and the kernel-level parts of the mode suites; tests/test_cpu_glue_ops_ref.py keeps the
 * ledger of which test file reaches which launcher) to check every hand-written kernel against a float64 / torch
 * reference in isolation.  Not part of the drop-in boundary (that is anyref_hip.h).
 * `t` selects the storage type: 0 = f32 (MFMA 16x16x4 f32), 1 = bf16 (MFMA 16x16x32 bf16), 3 = split pairs (ANYREF_MODE_PARITY16: f32
 * operands at the interface, carried as two bf16 terms inside; weights bf16; gemm / gemv / norm / attention entries), 2 = f16 (MFMA 16x16x32
 * f16: the SAM image encoder of the perf build and every tower of ANYREF_MODE_PERF_F16; GEMM, GEMV, norm, attention, decode
 * attention and RoPE entries), 4 = split pairs with f16 terms (ANYREF_MODE_PARITY16_F16: as 3 with f16 weights; the attention
 * entries multiply as 3 does and write their output rows as f16 pairs).
 * All pointers are device pointers; `stream` is a hipStream_t.
 */
#ifndef ANYREF_HIP_OPS_H
#define ANYREF_HIP_OPS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* C[row_map[m]] = act(A W^T + bias) + resid; A,W in type t; C f32 if c_f32 else t */
int anyref_op_gemm(int t, void* stream, const void* A, const void* W, const float* bias, void* C,
                   const float* resid, const int32_t* row_map, int M, int N, int K, int act, int c_f32);
/* y = act(rmsnorm?(x) W^T) [* (x W2^T)] + resid;  x,y f32; W in type t */
int anyref_op_gemv(int t, void* stream, const float* x, const float* gain, float eps, const void* W,
                   const void* W2, const float* bias, float* y, const float* resid, int B, int N, int K, int act);
/* anyref_op_gemv (t = 0 .. 4) plus the f32 copy of the RMS-normalised rows the lm_head GEMV writes (needs gain):
 * xn_out[(xn_row_map ? xn_row_map[b] : b) * xn_ld + k], xn_out 16-byte aligned, xn_ld % 4 == 0 */
int anyref_op_gemv_xn(int t, void* stream, const float* x, const float* gain, float eps, const void* W, const void* W2,
                      const float* bias, float* y, const float* resid, int B, int N, int K, int act, float* xn_out,
                      const int32_t* xn_row_map, int xn_ld);
/* f32 [rows, cols] -> pair-typed rows (t = 3: bf16 terms, t = 4: f16 terms; launch_convert) -> out f32 = hi + lo
 * (launch_unsplit); hi_out (optional, device, rows * cols 16-bit words): the raw hi terms */
int anyref_op_split_roundtrip(int t, void* stream, const float* in, float* out, void* hi_out, int rows, int cols);
/* the model's RoPE table: out_host f32 [S][2][hd/2] = cos | sin of pos * theta^(-2d/hd) (HOST pointer) */
int anyref_op_rope_table(int S, int hd, float theta, float* out_host);
/* the decode step's attention as the model runs it (t = 0 f32 / 1 bf16 / 2 f16 cache): qkv f32 [B, 3*H*hd], pos i32 [B], cs_tab
 * f32 [maxS][2][hd/2]; rotates q, k at pos[b], appends k, v to kc / vc T [B, maxS, H, hd] (and q to q_keep, same
 * layout, if given), out f32 [B, H*hd] = attention over keys [0, pos[b]].  force_fallback = 0: the fused kernel, or
 * the fallback where it refuses; 1: the fallback (RoPE + append, then the generic attention with Sq = 1) */
int anyref_op_decode_attn(int t, void* stream, const float* qkv, int B, int H, int hd, const int32_t* pos,
                          const float* cs_tab, void* kc, void* vc, int maxS, float scale, float* out, void* q_keep,
                          int force_fallback);
/* the rephrase branch as one launch pair (t = 0 f32 / 1 bf16 / 2 f16 cache).  items i32 dev [n_items][4] =
 * (b, e0, s0, out_row) with 0 <= s0 < e0 < maxS; q_keep / kc T [B, maxS, H, hd] (rotated queries, keys of the last layer),
 * hidden f32 [B, maxS, H*hd].  Per item: p_h = softmax_j(scale * q[b, e0, h] . k[b, j, h]) over keys j in [0, e0]; w_j = mean_h
 * p_h[j] for j in [s0, e0); y[out_row, :] += weight * sum_j hidden[b, j, :] * (w_j / sum_j w_j).  scratch f32 [n_items, H,
 * span_cap]; max_span = the largest e0 - s0 of the items (the host knows it).  *launched = 1, or 0 where the launcher refuses by
 * shape (hd * sizeof(T) no multiple of 16 or more than 64 such pieces / not a power of two of them, the score row of maxS
 * floats or span_cap floats past 64 KB of LDS, max_span > span_cap, a buffer not 16-byte aligned): then nothing was written */
int anyref_op_seg_rephrase(int t, void* stream, const void* q_keep, const void* kc, int maxS, int H, int hd, const float* hidden,
                           const int32_t* items, int n_items, int max_span, int span_cap, float* scratch, float scale,
                           float weight, float* y, int32_t* launched);
/* the same term for ONE item by the per-image chain (the head-mean attention row of query e0 over kv_len[0] = e0 + 1 keys into
 * attn_row f32 [maxS], then y f32 [H*hd] += weight * sum_j hidden[b, j] * attn_row[j] / sum): what runs with
 * anyref_set_rephrase_paths off, here for timing one against the other (tools/ab_session.py) */
int anyref_op_rephrase_chain(int t, void* stream, const void* q_keep, const void* kc, int maxS, int H, int hd,
                             const float* hidden, int b, int e0, int s0, const int32_t* kv_len, float* attn_row, float scale,
                             float weight, float* y);
/* prefill RoPE + KV append (t = 0 f32 / 1 bf16 / 2 f16): qkv T [B, S, 3, H, hd], or (slab0 non-NULL) the sum of two f32 slabs
 * of that shape (rounded to T first; t = 0: not rounded); rows s < lens[b] (all if lens is NULL) go to position pos0[b] + s (pos0 NULL: 0); q_out T [B, S, H, hd],
 * kc / vc / q_keep T [B, maxS, H, hd] */
int anyref_op_rope_cache(int t, void* stream, const void* qkv, const float* slab0, const float* slab1, int B, int S, int H,
                         int hd, const int32_t* pos0, const int32_t* lens, const float* cs_tab, void* q_out, void* kc,
                         void* vc, int maxS, void* q_keep);
/* argmax of x f32 rows [M, N] (row stride ldx) -> out i64 [M], first index on ties, NaN greatest; pos (optional) += 1.
 * table non-NULL ([vocab, D]; is_bf16 is its dtype: 0 = f32, 1 = bf16, 2 = f16): also x_next f32 [M, D] = table[out[b]], row_map[b] =
 * b * maxS + pos[b], kvlen[b] = pos[b] + 1 (pos required) */
int anyref_op_argmax(void* stream, const float* x, int M, int N, int ldx, int64_t* out, int32_t* pos, const void* table,
                     int is_bf16, int D, int maxS, float* x_next, int32_t* row_map, int32_t* kvlen);
/* token scores (anyref_set_token_scores) of logits f32 rows [M, N] (row stride ldx): with id = the row's argmax as
 * anyref_op_argmax chooses it, logprob = x[id] - logsumexp(x) and gap = x[id] - max over i != id of x[i] (the top-2 logit gap,
 * 0 on a tie; the f32 subtraction).  Row i writes index dst[i] of logprob f32 / gap f32 / id i64 (id may be NULL); dst NULL:
 * index i; dst[i] < 0: the row is skipped without being read and nothing is written for it.  A row holding a NaN gives
 * logprob = gap = NaN; -inf entries add 0 to the sum.  Error (nothing launched) if M < 1, N < 2 or ldx < N. */
int anyref_op_token_scores(void* stream, const float* logits, int M, int N, int ldx, const int32_t* dst, float* logprob,
                           float* gap, int64_t* id);
/* mask report (anyref_set_mask_reports; the rule: anyref_amd/maskreport.py) of mask logits f32 [n, H, W] (contiguous, any 4-byte
 * alignment) with stability offset d = `offset` >= 0.  records i32 [n, 8] = {area #{x > 0}, area_hi #{x > d}, area_lo #{x > -d},
 * nonfinite #{NaN, +-inf}, x0, y0, x1, y1} -- the inclusive box of the bits x > 0, all 0 for an empty mask.  packed u32
 * [n, H, Wp], Wp = ceil(W / 32), or NULL: bit k (LSB first) of word w of row y is x[y, 32 w + k] > 0, bits past W are 0.  NaN and
 * -0.0 give bit 0.  The records need no clearing by the caller.  Exact: integer counts, bit-identical on a rerun.  Error (nothing
 * queued) if H < 1, W < 1, H * W > INT32_MAX, n > 65535, the offset is negative or not finite, or logits / records is NULL;
 * n <= 0 does nothing. */
int anyref_op_mask_report(void* stream, const float* logits, int n, int H, int W, float offset, int32_t* records,
                          uint32_t* packed);
/* accept step of the draft-verified greedy decode (anyref_set_draft): logits f32 [B * k, N] (row stride ldx) of a verification
 * pass that fed draft i64 [B, k] (draft_lens[b] <= k valid ids per row, 0 = none) behind next[b], the token already chosen.
 * p i64 [B * k] receives the row argmaxes (first index on ties).  Per row, with g[0] = next[b], g[j + 1] = p[j]: accepted[b] = m =
 * number of leading j < draft_lens[b] with g[j] == draft[b, j]; tokens i64 [B, k + 1] receives g[0 .. m]; and, as
 * anyref_op_argmax leaves them: next[b] = g[m], pos[b] += m, x_next f32 [B, D] = table[g[m]] (dtype 0 = f32, 1 = bf16, 2 = f16),
 * row_map[b] = b * maxS + pos[b], kvlen[b] = pos[b] + 1.  1 <= k <= 256. */
int anyref_op_draft_accept(void* stream, const float* logits, int B, int k, int N, int ldx, int64_t* p, const int64_t* draft,
                           const int32_t* draft_lens, int64_t* next, int32_t* pos, int64_t* tokens, int32_t* accepted,
                           const void* table, int dtype, int D, int maxS, float* x_next, int32_t* row_map, int32_t* kvlen);
/* prefix broadcast of an image session (anyref_session_generate): kc and vc (vc may be NULL: one buffer) are KV caches
 * [layers][rows][maxS][row_elems] of elements of elem_size bytes (2 or 4; the kernel moves bytes and never interprets them).
 * In every layer of both, positions [0, P) of row 0 are copied to rows [r0, r1); everything else is left as it was.  One launch
 * for all layers, both buffers and all target rows.  P == 0 or r1 <= r0 (a single query) launches nothing and returns 0.
 * Error if P > maxS, r0 < 1 or r1 > rows. */
int anyref_op_kv_broadcast(void* stream, void* kc, void* vc, int layers, int rows, int maxS, int row_elems, int elem_size,
                           int P, int r0, int r1);
/* per-row gather / pack of a session pool (anyref_session_generate_pooled / anyref_session_store): kc and vc (vc may be NULL: one
 * buffer) are working buffers [layers][rows][maxS][row_elems] as above, pool is [n_slots][planes][maxP][row_elems] with planes =
 * layers, or 2 * layers when vc is given (K planes first).  table i32 [n, 4] host: (slot, P, row, skip) per item.  pack == 0: in
 * every plane, positions [0, P) of pool slot `slot` are copied to row `row`; pack != 0: the other way.  Everything else, on both
 * sides, is left as it was.  One launch for all planes and up to 16 items; items with P == 0 or skip != 0 move nothing.  The
 * kernel moves bytes (16 at a time when row_elems * elem_size is a multiple of 16, else 2) and never interprets them.
 * Error, with nothing launched: slot outside [0, n_slots), row outside [0, rows), P > maxP or P > maxS, two moved items with the
 * same row (gather) or the same slot (pack). */
int anyref_op_kv_gather(void* stream, void* kc, void* vc, int layers, int rows, int maxS, void* pool, int n_slots, int maxP,
                        int row_elems, int elem_size, const int32_t* table, int n, int pack);
/* LayerNorm (rms=0) / RMSNorm (rms=1); x f32, y f32 */
int anyref_op_norm(int t, void* stream, const float* x, const float* gain, const float* bias, float* y, int M,
                   int D, float eps, int rms);
/* q,k,v,o [B,S,H,hd] contiguous in type t; rel_h/rel_w f32 [B,H,Sq,kh|kw] or NULL */
int anyref_op_attention(int t, void* stream, const void* q, const void* k, const void* v, void* o, int B, int H,
                        int Sq, int Sk, int hd, float scale, int causal, const int32_t* kv_len,
                        const float* rel_h, const float* rel_w, int kh, int kw);
/* SAM decomposed rel-pos tables from q [B,S=size*size,H,hd] (type t) */
int anyref_op_rel_pos(int t, void* stream, const void* q, const float* tab_h, const float* tab_w, int B, int H,
                      int size, int hd, float* rel_h, float* rel_w);
/* Row-wise fp8 e4m3 quantisation used by ANYREF_MODE_PERF_FP8W: src f32 [N,K] -> q u8 [N,K], scale f32 [N] */
int anyref_op_quant_fp8(void* stream, const float* src, int N, int K, uint8_t* q, float* scale);
/* bf16 GEMM with an fp8 weight operand: C = act((A W8^T) * scale[n] + bias) (+ resid); A bf16 [M,K], W8 u8 [N,K] */
int anyref_op_gemm_fp8(void* stream, const void* A, const uint8_t* W8, const float* scale, const float* bias, void* C,
                       const float* resid, int M, int N, int K, int act, int c_f32);
/* decode GEMV on fp8 weights: y[b,n] = (sum_k bf16(norm(x))[b,k] * q[n,k]) * scale[n] (SwiGLU pair if W2) */
int anyref_op_gemv_fp8(void* stream, const float* x, const float* gain, float eps, const uint8_t* W,
                       const uint8_t* W2, const float* scale, const float* scale2, float* y, const float* resid,
                       int B, int N, int K);
/* int4 group quantisation used by ANYREF_MODE_PERF_INT4W: src f32 [N,K] (K % 16 == 0) -> nibble rows q u8 [N, ceil(K/128) * 64]
 * (the order of the nibbles inside a 16-byte block is the library's) and scales bf16 [N, ceil(K/128)] */
int anyref_op_quant_int4(void* stream, const float* src, int N, int K, uint8_t* q, void* scale_bf16);
/* The LoRA merge of anyref_adapter_apply (lora_merge_rows_kernel; the rule: include/anyref_hip.h, anyref_amd/lora.py) on caller
 * buffers: base_f32 f32 [N,K] dev (values exactly representable in dtype d_in = ANYREF_F32 / BF16 / F16), A f32 [r,K], B f32 [N,r]
 * dev, r in 1 .. 64 -> dst of type t (0 f32, 1 bf16, 2 f16): row n at dst + n * row_stride * ld elements (ld >= K; row_stride 1 or
 * 2), columns [0, K) only.  counts u64 [2] dev or NULL (16-bit t): [0] += elements stored inexactly, [1] += finite values stored
 * as inf.  t = 0 followed by anyref_op_quant_fp8 / anyref_op_quant_int4 is the quantised modes' path. */
int anyref_op_lora_merge(int t, void* stream, const float* base_f32, int d_in, int N, int K, const float* A, const float* B,
                         int r, float scaling, void* dst, int ld, int row_stride, uint64_t* counts);
/* q, scale as written by anyref_op_quant_int4 -> out bf16 [N,K] = q * scale (exact) */
int anyref_op_dequant_int4(void* stream, const uint8_t* q, const void* scale_bf16, int N, int K, void* out_bf16);
/* bf16 GEMM with an int4 weight operand (q, scale as written by anyref_op_quant_int4; K % 64 == 0, anything else is an error):
 * C = act(A W'^T + bias) (+ resid), W' = q * scale; A bf16 [M,K]; C f32 or bf16 [M,N].  swiglu: the rows of W are interleaved
 * (gate_j, up_j) pairs and C [M, N/2] = silu(c[m, 2j]) * c[m, 2j+1] (no bias / resid / act).  The launch tags are left in
 * anyref_op_last_tags(). */
int anyref_op_gemm_int4(void* stream, const void* A, const uint8_t* W4, const void* scale_bf16, const float* bias, void* C,
                        const float* resid, int M, int N, int K, int act, int c_f32, int swiglu);
/* decode GEMV on int4 weights: y[b,n] = sum_g scale[n,g] * sum_{k in g} bf16(norm(x))[b,k] * q[n,k] (SwiGLU pair if W2) (+ resid) */
int anyref_op_gemv_int4(void* stream, const float* x, const float* gain, float eps, const uint8_t* W, const uint8_t* W2,
                        const void* scale_bf16, const void* scale2_bf16, float* y, const float* resid, int B, int N, int K);
/* SURVEY.md §8 f-2, replaces `(torch.sigmoid(pred) > 0.5).int()` + utils/utils.py:79-91
 * intersectionAndUnionGPU(pred, gt, 2, ignore_index=255) (call site eval_referseg.py:189-208):
 * logits f32 [n, hw] (device), target u8 [n, hw] with values 0 / 1 / 255 (device), counts i64 [n, 6]
 * (device) = {I0, I1, O0, O1, T0, T1}; area_intersection = I, area_union = O + T - I, area_target = T. */
int anyref_op_iou_counts(void* stream, const float* logits, const uint8_t* target, int n, int64_t hw,
                         int64_t* counts);
/* SURVEY.md §8 f-2 (AVS), the per-pixel part of `mask_iou` and `Eval_Fmeasure` / `_eval_pr`
 * (utils/pyutils.py:163-236; caller eval_avs_object.py:168-178) in one pass: logits f32 [n, hw], target u8
 * [n, hw] (0 / non-zero), cuts f32 [nth] ascending (device; cut_i = smallest logit whose sigmoid reaches the
 * i-th P/R threshold), cut_pred = smallest logit with sigmoid > 0.5.  conf i64 [n, 4] = counts by 2 * pred + gt;
 * hist i64 [n, nth + 1, 2] = pixels by (number of thresholds passed, gt). nth <= 255. */
int anyref_op_avs_counts(void* stream, const float* logits, const uint8_t* target, int n, int64_t hw,
                         const float* cuts, int nth, float cut_pred, int64_t* conf, int64_t* hist);
/* SURVEY.md §8 f-1, replaces `sam_preprocess` (utils/refer_seg.py:560-570) after ResizeLongestSide: img u8
 * HWC [h, w, 3] (device) -> out f32 CHW [3, S, S] (device), (x - mean3[c]) / std3[c], zero padded; mean3 /
 * std3 are HOST pointers. */
int anyref_op_sam_preprocess(void* stream, const uint8_t* img, int h, int w, int S, const float* mean3,
                             const float* std3, float* out);
/* SURVEY.md §8 f-1, replaces `ResizeLongestSide.apply_image` (segment_anything/utils/transforms.py:27-34) and the
 * bicubic resize inside `CLIPImageProcessor.preprocess` (utils/refer_seg.py:578-580): Pillow's 8-bit separable
 * fixed-point resampling, bit-exact.  in u8 [H, W, C] dev -> out u8 [oh, ow, C] dev; tmp u8 [H, ow, C] dev scratch
 * (needed when both sizes change).  Coefficient tables (device, int32; built on the host as Pillow's
 * precompute_coeffs + normalize_coeffs_8bpc do): xbounds [ow, 2] = (first input column, tap count), xk [ow, kx]
 * = round(tap * 2^22); ybounds / yk likewise for rows.  A pass whose size does not change is skipped (tables may be
 * NULL), as in Pillow. */
int anyref_op_pil_resample_u8(void* stream, const uint8_t* in, int H, int W, int C, uint8_t* tmp, uint8_t* out,
                              int ow, int oh, const int32_t* xbounds, const int32_t* xk, int kx,
                              const int32_t* ybounds, const int32_t* yk, int ky);
/* SURVEY.md §8 f-3, the token pooling of the `ref_images` branch (model/anyref.py:335-338, :697-700): feats f32
 * [n, L, H] dev (`encode_images` output, L = 256) -> mean over groups of 16 tokens -> (L/16 != n_out) mean over
 * groups of n_out rows -> out f32 [n, n_out, H] dev (n_out = IMG_REF_NUM = 4). */
int anyref_op_pool_ref_tokens(void* stream, const float* feats, int n, int L, int H, int n_out, float* out);
/* SURVEY.md §8 f-1, the rest of the CLIP input path (utils/refer_seg.py:578-587): window [y0, y0+h) x [x0, x0+w) of
 * img u8 [ih, iw, 3] dev -> x * (1/255) (in double, then f32) -> (x - mean3[c]) / std3[c] -> bilinear
 * (align_corners = False) to out f32 CHW [3, S, S] dev.  mean3 / std3 are HOST pointers. */
int anyref_op_clip_finish(void* stream, const uint8_t* img, int ih, int iw, int y0, int x0, int h, int w, int S,
                          const float* mean3, const float* std3, float* out);
/* SURVEY.md §8 f-4, the audio front-end in front of the ImageBind trunk: replaces `waveform2melspec` + `Normalize`
 * (model/ImageBind/data.py:28-64,152-153; torchaudio.compliance.kaldi.fbank with htk_compat, hanning window, 25 ms / 10 ms
 * frames, no dither, 0.97 pre-emphasis, DC removal, power spectrum, log) for ONE clip: wave f32 [C, T] dev (channel 0
 * is analysed, the clip mean is taken over all channels), banks f32 [n_mel, padded / 2 + 1] dev (kaldi mel filters + zero
 * Nyquist column), tw f64 [2 * padded] dev (cos, then sin, of 2 pi i / padded), scratch f64 [1] dev -> out f32
 * [n_mel, target_len] dev = (pad_or_cut(log-mel^T) - mean) / std.  win / padded: 400 / 512 (16 kHz). */
int anyref_op_kaldi_fbank(void* stream, const float* wave, int C, int T, int win, int shift, int padded, float preemph,
                          const float* banks, int n_mel, const double* tw, double* scratch, int target_len, float mean,
                          float stdv, float* out);
/* 16-bit (t = 1 bf16 / 2 f16) window attention with the decomposed rel-pos bias computed inside the kernel from the tables
 * (image_encoder.py:321-392 get_rel_pos / add_decomposed_rel_pos): tab_h [2*kh-1, hd], tab_w [2*kw-1, hd] in type t,
 * rows at stride tab_ld elements; S = kh*kw tokens, [B,S,H,hd] operands.  Only the shapes the resident-key form
 * takes (hd 80, 192 < S <= 208); others are refused. */
int anyref_op_attention_tab(int t, void* stream, const void* q, const void* k, const void* v, void* o, int B, int H, int S,
                            int hd, float scale, const void* tab_h, const void* tab_w, int tab_ld, int kh, int kw);
/* 16-bit GEMM with an A-row gather: C[m, :] = A[a_row_map[m], :] W^T + bias (+ resid[m, :]) -- the SAM window layers'
 * proj over the real tokens of the window-layout attention output (model.hip sam_encoder; image_encoder.py:196-229,
 * window_unpartition).  t = 1 (bf16) / 2 (f16); K % 64 == 0. */
int anyref_op_gemm_gather(int t, void* stream, const void* A, const int32_t* a_row_map, const void* W, const float* bias,
                          void* C, const float* resid, int M, int N, int K, int c_f32);
/* the same attention with the bias taken from the P buffer the model's batched rel-pos GEMM writes (model.hip
 * sam_encoder, image_encoder.py:354-392): P f32 [H][B*S][rel_ld], columns [0, rel_ld/2) = q . rel_pos_h[e],
 * [rel_ld/2, rel_ld) = q . rel_pos_w[e]; the kernel applies the get_rel_pos shift.  S = kh*kw tokens, [B,S,H,hd]
 * operands.  kw == 64 (SAM global attention) takes the two-query-blocks-per-wave kernel. */
int anyref_op_attention_relp(int t, void* stream, const void* q, const void* k, const void* v, void* o, int B, int H, int S,
                             int hd, float scale, const float* rel_p, int rel_ld, int kh, int kw);
/* Sam.postprocess_masks on low [n,lh,lw] f32 */
int anyref_op_postprocess(void* stream, const float* low, int n, int lh, int lw, int S, int rh, int rw, int H,
                          int W, float* out);
const char* anyref_op_last_error(void);

/* ---- the launch forms the model itself uses (tests/test_gpu_gemm_forms.py): one plain struct per launcher, mirroring the
 * fields of GemmArgs / NormArgs / AttnArgs (anyref_amd/csrc/kernels.h) a test needs.  Pointers are device pointers, strides in
 * elements.  Every call records the launch tags booked while it ran (anyref_op_last_tags). ---- */
typedef struct anyref_gemm_ex {
  const void* A;            /* T [batch][M, K] at row stride lda, batch stride sA (t = 3 / 4: f32, batch 1) */
  const void* W;            /* T [N, K] at row stride ldw, batch stride sW (t = 3: bf16, t = 4: f16) */
  const float* bias;        /* [N], batch stride sBias */
  void* C;                  /* f32 (c_f32) or T (t = 3 / 4: f32 either way, read back from pairs if !c_f32) */
  const float* resid;       /* f32 at row stride ldr, batch stride sR; may alias C */
  const int32_t* row_map;
  const int32_t* a_row_map;
  const float* norm_gain;
  const float* norm_bias;   /* set: LayerNorm */
  void* norm_out;           /* T [M, N] at row stride norm_ld (t = 3 / 4: f32, read back from pairs when the norm was fused) */
  float* slabs_out;         /* f32 [slabs][M, N] */
  int64_t sA, sW, sC, sR, sBias;
  int32_t M, N, K, lda, ldw, ldc, ldr, norm_ld;
  int32_t act, c_f32, swiglu_pairs, slabs, max_wg, batch;
  float alpha, norm_eps;
  int32_t norm_done;        /* out: the norm rode on the split-K reduction */
} anyref_gemm_ex;
int anyref_op_gemm_ex(int t, void* stream, anyref_gemm_ex* e);

typedef struct anyref_norm_ex {
  const float* x;           /* f32 [M, D] at row stride ldx */
  const float* gain;
  const float* bias;        /* NULL with rms */
  void* y;                  /* f32 (y_f32) or T at row stride ldy (t = 3 / 4: f32 holding hi + lo of the pairs) */
  const int32_t* row_map;   /* destination row, < 0: dropped */
  void* fill_dst;           /* T (t = 3 / 4: f32) rows at stride fill_ld: fill_dst[fill_rows[i], 0:fill_N) = fill_bias */
  const int32_t* fill_rows;
  const float* fill_bias;
  int32_t M, D, ldx, ldy, rms, y_f32, act;
  int32_t fill_ld, fill_n, fill_N;
  int32_t fill_fallback;    /* 1: launch_fill_rows_bias when the norm kernel did not take the side job (as the model does) */
  float eps;
  int32_t fill_done;        /* out: the wide-row kernel wrote the fill rows */
} anyref_norm_ex;
int anyref_op_norm_ex(int t, void* stream, anyref_norm_ex* e);

typedef struct anyref_attn_ex {
  const void *q, *k, *v;    /* T (t = 0 .. 3; t = 3: f32) at the batch / row / head strides below */
  void* o;                  /* T (t = 3: f32 holding hi + lo; o_bs == Sq * o_rs, o_rs % 64 == 0) */
  const int32_t *q_pos0, *kv_len, *q_len;
  const float *rel_h, *rel_w, *rel_p;
  const void *rel_tab_h, *rel_tab_w;
  int64_t q_bs, q_rs, q_hs, k_bs, k_rs, k_hs, v_bs, v_rs, v_hs, o_bs, o_rs, o_hs, rel_hs;
  int32_t B, H, Sq, Sk, hd, causal, kh, kw, rel_ld, rel_tab_ld, max_wg;
  float scale;
} anyref_attn_ex;
int anyref_op_attention_ex(int t, void* stream, anyref_attn_ex* e);
/* the launch tags (kernels.h ProfScope) booked during the last *_ex call of this thread, comma separated */
const char* anyref_op_last_tags(void);

/* ---- glue kernels and the skinny f32 GEMV (tests/test_gpu_glue_ops.py; references: tests/glue_ops_ref.py) ---- */
/* launch_gemv_skinny_f32 (every mask-decoder token GEMM, both text_hidden_fcs layers): y[b, n] = act(sum_k x[b, k] W[n, k] +
 * bias[n]) + resid[b, n]; x f32 rows at stride ldx, W f32 [N, K] contiguous, y / resid f32 rows at stride ldy (resid may be y
 * or NULL), act as anyref_op_gemm.  The launcher refuses B outside 1 .. 8, K > 4096, K % 4, ldx % 4 and unaligned x / W */
int anyref_op_gemv_skinny(void* stream, const float* x, int ldx, const float* W, const float* bias, float* y, int ldy,
                          const float* resid, int B, int N, int K, int act);
/* first upscaler tail: tmp f32 [n*g*g, 4*C] (col = (dy*2+dx)*C + c) -> out [n, 2g, 2g, C] = gelu(LayerNorm2d over C); t = 0
 * (f32 out) is the only instantiation; C <= 128 */
int anyref_op_upscale1(int t, void* stream, const float* tmp, int n, int g, int C, const float* ln_g, const float* ln_b, float eps,
                       void* out);
/* second tail: masks f32 [n, ntok, 2*g2, 2*g2] = sum_c hyper[i, t, c] * gelu(tmp[i, (Y/2, X/2), (Y%2*2 + X%2)*C + c]);
 * hyper f32 [n, ntok, C], ntok <= 8 */
int anyref_op_upscale2_masks(void* stream, const float* tmp, const float* hyper, int n, int ntok, int g2, int C, float* masks);
/* dense positional encoding: gauss f32 [2, F] -> out f32 [g*g, 2*F] = sin | cos of 2 pi (cx G[0] + cy G[1]), c = 2 (i + .5) / g - 1 */
int anyref_op_dense_pe(void* stream, const float* gauss, int g, int F, float* out);
/* tokens f32 [n, n_out + 1, C]: rows 0 .. n_out-1 = out_tokens [n_out, C], row n_out = pred[i] */
int anyref_op_build_tokens(void* stream, const float* out_tokens, int n_out, const float* pred, int n, int C, float* tokens);
/* SAM spatial prompts (prompt_encode.hip).  tokens f32 [n, NQ, C], NQ = n_out + P + pad + 2 box + text, pad = (P > 0 and no
 * boxes): out_tokens, then the points (PE + emb5[label] for label 0 / 1, emb5[4] alone for -1, the PE alone otherwise), the
 * pad (emb5[4]), the box corners (PE + emb5[2], PE + emb5[3]), text[i].  points f32 [n,P,2] (x, y) in pixels of the S x S
 * input frame, labels i32 [n,P], boxes f32 [n,4] or NULL, text f32 [n,C] or NULL, gauss f32 [2, C/2], emb5 f32 [5,C].
 * C % 8 == 0.  max_wg > 0 caps the grid.  A refused call writes nothing */
int anyref_op_prompt_tokens(void* stream, const float* out_tokens, int n_out, const float* points, const int32_t* labels, int P,
                            const float* boxes, const float* text, const float* gauss, const float* emb5, int n, int C, int S,
                            float* tokens, int max_wg);
/* keys f32 [n, g*g, C] = image_emb [g*g, C] + mask_downscaling(mask f32 [n, 4g, 4g]) as NHWC: conv k2s2 w1 [c1,1,2,2] + b1,
 * LayerNorm2d (ln1_g, ln1_b, eps 1e-6), GELU, conv k2s2 w2 [c2,c1,2,2] + b2, LayerNorm2d (ln2_g, ln2_b), GELU, conv 1x1
 * w3 [C,c2] + b3.  c1 <= 8, c2 <= 32, C % 4 == 0, C <= 1024.  max_wg > 0 caps the grid.  A refused call writes nothing */
int anyref_op_mask_prompt_embed(void* stream, const float* mask, const float* image_emb, const float* w1, const float* b1,
                                const float* ln1_g, const float* ln1_b, const float* w2, const float* b2, const float* ln2_g,
                                const float* ln2_b, const float* w3, const float* b3, int n, int g, int C, int c1, int c2,
                                float* keys, int max_wg);
/* out[m, :] = a[m, :] + b[m % bmod, :] and out[m, :] = a[m, :] + v[:]   (f32 [M, D]) */
int anyref_op_add_rows(void* stream, const float* a, const float* b, int bmod, float* out, int M, int D);
int anyref_op_add_vec(void* stream, const float* a, const float* v, float* out, int M, int D);
/* LLaVA input assembly: ids i64 [B, Lmax], lens i32 [B], table [vocab, D] of dtype 0 f32 / 1 bf16 / 2 f16, img_feat f32
 * [B, n_img, D] -> x f32 [B, Smax, D]: the first -200 of a row expands to the n_img image rows, every other id < 0 or >= vocab
 * gives a zero row, rows >= out_len[b] are left alone; out_len[b] = len (+ n_img - 1 with an image).  At most Smax rows */
int anyref_op_embed_splice(void* stream, const int64_t* ids, const int32_t* lens, int B, int Lmax, const void* table, int dtype,
                           int vocab, const float* img_feat, int n_img, float* x, int Smax, int D, int32_t* out_len);
/* x[dst_b[i], dst_pos[i], :] = rows[i, :];  out[i, :] = x[b[i], pos[i], :];  x[b, :] = table[ids[b], :]   (x f32 [*, Smax, D]) */
int anyref_op_scatter_rows(void* stream, const float* rows, const int32_t* dst_b, const int32_t* dst_pos, int n, float* x, int Smax,
                           int D);
int anyref_op_gather_rows(void* stream, const float* x, int Smax, int D, const int32_t* b, const int32_t* pos, int n, float* out);
int anyref_op_embed_rows(void* stream, const int64_t* ids, int B, const void* table, int dtype, int D, float* x);
/* tower front ends, t = 0 .. 4.  out is T [rows, cols] for t = 0 / 1 / 2; for t = 3 / 4 the kernel runs on pair rows (cols % 64
 * == 0) and out is f32 = hi + lo, as anyref_op_split_roundtrip returns it.
 * patch: img f32 [B, 3, S, S] -> [B*(S/p)^2, Kp], k = c*p*p + ky*p + kx, columns >= 3 p^2 zero
 * 3x3:   in T [B, g, g, C] (t = 3 / 4: f32, converted to pairs here; C % 64 == 0) -> [B*g*g, 9*C], k = (ky*3 + kx)*C + c, pad 1
 * conv1: img f32 [n, Hh, Ww] -> [n*gh*gw, k*k], gh = (Hh - k) / st + 1, patches overlap (st < k) */
int anyref_op_im2col_patch(int t, void* stream, const float* img, int B, int S, int p, void* out, int Kp);
int anyref_op_im2col_3x3(int t, void* stream, const void* in, int B, int g, int C, void* out);
int anyref_op_im2col_conv1(int t, void* stream, const float* img, int n, int Hh, int Ww, int k, int st, void* out);
/* x f32 [B, rows, D]: x[b, 0] = cls + pos[0], x[b, 1 + i] = patch[b, i] + pos[1 + i], rows n + 1 .. rows - 1 zero (rows = 0: n + 1) */
int anyref_op_clip_assemble(void* stream, const float* patch, const float* cls, const float* pos, float* x, int B, int n, int D,
                            int rows);
/* y[r, :] = x[r, :] / max(||x[r]||_2, 1e-12) * scale   (f32 [rows, D]) */
int anyref_op_l2norm_scale(void* stream, const float* x, int rows, int D, float scale, float* y);
/* out f32 [n] = in of dtype 0 f32 / 1 bf16 / 2 f16 */
int anyref_op_to_f32(void* stream, const void* in, int dtype, float* out, int64_t n);
/* out bf16 [N, K] (row stride ldo, % 8) = bf16(f32(e4m3 q[n, k]) * scale[n]); q rows ldq bytes apart (% 16), K % 16 == 0 */
int anyref_op_dequant_fp8(void* stream, const uint8_t* q, int ldq, const float* scale, int N, int K, void* out_bf16, int ldo);

#ifdef __cplusplus
}
#endif
#endif
