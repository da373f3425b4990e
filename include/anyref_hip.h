/*
 * anyref_hip.h — C-ABI of the MI355X-native AnyRef inference backend (libanyref_hip.so).
 *
 * The reference (jwh97nn/AnyRef) is pure Python and has NO FFI / plugin layer
 * (SURVEY.md §8b); its boundary for this path is the Python surface of
 * `AnyRefForCausalLM` (model/anyref.py:182-237, :647-822) plus the state_dict
 * key names.  This library sits one level below a Python class that reproduces
 * that surface (anyref_amd/model.py); every entry point cites the reference
 * interface whose arithmetic it replaces.
 *
 * Conventions
 *   - plain pointers + sizes only; no torch / STL types cross the boundary
 *   - every `dev` pointer is HBM memory on the handle's device, owned by the caller
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it
 *   - return 0 on success, non-zero on error; text via anyref_last_error()
 *   - one handle per GPU per process; calls on one handle are serialised by the caller
 */
#ifndef ANYREF_HIP_H
#define ANYREF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANYREF_ABI_VERSION 2

/* dtype codes for anyref_set_weight */
#define ANYREF_F32 0
#define ANYREF_BF16 1
#define ANYREF_F16 2

/* compute modes */
#define ANYREF_MODE_PARITY 0 /* fp32 activations + fp32-input MFMA (exact fp32 accumulate) */
#define ANYREF_MODE_PERF 1   /* bf16 weights/activations on bf16 MFMA, fp32 accumulate + fp32 residual stream */
/* PERF with the LLaMA linear layers (q/k/v/o, gate/up/down, lm_head) held as fp8 e4m3 bytes + one f32 scale
 * per output row (weight-only, quantised at finalize: scale = max|row| / 448, RNE): half the weight bytes of
 * the HBM-bound decode; activations, the vision towers and SAM stay as in PERF (BASELINE config 5) */
#define ANYREF_MODE_PERF_FP8W 2
/* The tolerance-meeting mode at 16-bit MFMA rate (north_star: mask logits within 1e-3, identical greedy ids): weights stay in
 * their exact bf16 storage (never widened in HBM: a decode step streams the same bytes as PERF); every activation that feeds a
 * matrix product is f32 carried as a PAIR of bf16 terms (hi = bf16(a), lo = bf16(a - hi): |a - hi - lo| <= 2^-18 |a|), one bf16
 * MFMA pass per term into the same f32 accumulator; the decode GEMV multiplies the f32 activation row (kept in LDS as f32)
 * with the bf16 weights; attention operands (q, k, v, the KV cache), residual streams, norms and the mask decoder are f32 as
 * in PARITY.  Inputs must be weights that are exactly representable in bf16 (the synthetic workloads round once; a real
 * fp32 SAM checkpoint is rounded to bf16 at finalize, as the reference's own fp16 evaluation rounds it to fp16). */
#define ANYREF_MODE_PARITY16 3
/* PERF with f16 in place of bf16: the LLaMA, CLIP, audio and SAM encoder weights and GEMM A-operands, the KV cache and the
 * attention operands are IEEE half (11 significant bits against bf16's 8, same MFMA / dot2 rate, same bytes); residual streams,
 * norms, accumulation, the mask decoder and the logits stay f32 as in PERF.  Holds an fp16 checkpoint (the reference's own
 * evaluation dtype) bit for bit; f16 activations saturate past 65504 as in the reference's fp16 run.  finalize fails, naming
 * the tensor, if a weight lies outside the f16 range.  fp8 weights are not offered with it. */
#define ANYREF_MODE_PERF_F16 4
/* PARITY16 with f16 in place of bf16 wherever a weight is stored or multiplied: the tolerance-meeting mode for fp16 checkpoints
 * (the reference's own evaluation dtype).  LLaMA / CLIP / audio / SAM-encoder weights are stored as f16 exactly as handed over
 * (anyref_inexact_weights = 0 for ANYREF_F16 input; f32 / bf16 input is rounded to f16 and counted; finalize fails, naming the
 * tensor, if a weight lies outside +-65504).  Every activation that feeds a matrix product is f32 carried as a PAIR of f16 terms
 * (hi = f16(a), lo = f16(a - hi): |a - hi - lo| <= max(2^-22 |a|, 2^-25)), one f16 MFMA pass per term into the same f32
 * accumulator (f16 x f16 is exact there); the decode GEMV multiplies the f32 activation row with the f16 weights.  Attention
 * products (q, k, v, the KV cache, rel-pos tables: f32 with no stored 16-bit factor) are multiplied as bf16 pairs exactly as in
 * PARITY16; residual streams, norms and the mask decoder are f32.  Range: a GEMM A-operand (norm / attention output, GELU /
 * SwiGLU hidden row, image patch) past +-65504 becomes inf in its hi term and shows as NaN outputs; the reference's fp16 run
 * has the same limit on more tensors. */
#define ANYREF_MODE_PARITY16_F16 5
/* PERF with q/k/v/o and gate/up/down of every LLaMA layer held as 4-bit integers with one bf16 scale per group of 128
 * consecutive k of an output row (weight-only, quantised at finalize; the last group of a row may be short).  Per group:
 * amax = max|w|; amax < 2^-100: s = 1, q = 0; else s = amax / 7 (f32) rounded UP to 5 significant bits (a bf16 with three zero
 * low mantissa bits, amax / 7 <= s <= 1.0625 amax / 7), q = clamp(rne(w / s), -7, 7), held value w' = q * s -- exactly a bf16,
 * so the decode GEMV (sum_g s_g sum_k q_k x_k) and the MFMA GEMM of prefill, the teacher-forced forward, llm_forward and decode
 * steps of more than 8 rows (it reads the nibbles as stored and widens each operand fragment to the bf16 w' in registers; a
 * linear whose K is not a multiple of 64 goes through a bf16 image of w' instead) multiply one set of weights.
 * lm_head, the embeddings, the vision / audio towers, SAM and every activation stay as in PERF.  About 0.52 bytes per LLM
 * linear element instead of 2.  llm_dim and llm_mlp must be multiples of 16 (finalize fails, naming the tensor).
 * A byte / accuracy trade (relative rms weight error 0.12 - 0.15 on Gaussian weights), not a parity mode;
 * anyref_amd/quant.py states the format in torch. */
#define ANYREF_MODE_PERF_INT4W (6)

typedef struct anyref_config {
  int32_t abi_version; /* = ANYREF_ABI_VERSION */
  int32_t mode;        /* ANYREF_MODE_* */
  /* CLIP vision tower (HF CLIPVisionModel under the absent model/llava; anyref.py:190-192) */
  int32_t clip_image, clip_patch, clip_dim, clip_heads, clip_layers_run, clip_mlp;
  float clip_eps;
  /* LLaMA decoder (HF LlamaModel; anyref.py:211-215) */
  int32_t llm_vocab, llm_dim, llm_heads, llm_layers, llm_mlp, llm_max_seq;
  float llm_rms_eps, llm_rope_theta;
  /* SAM (build_sam.py:48-108) */
  int32_t sam_img, sam_patch, sam_dim, sam_depth, sam_heads, sam_mlp_ratio, sam_window;
  int32_t sam_n_global;
  int32_t sam_global_idx[8];
  int32_t sam_out_chans, dec_heads, dec_mlp, dec_depth, num_mask_tokens;
  /* glue (anyref.py:116-127,161,197-209) */
  int32_t out_dim, audio_dim;
  int32_t seg_lo, seg_hi; /* inclusive [SEG] id range */
  float rephrase_weight;
  int32_t max_batch; /* images per call on this GPU */
  int32_t max_seg;   /* [SEG] tokens per image the workspaces are sized for */
  /* ImageBind audio trunk in HIP (imagebind_model.py:175-192,331-338,391-395,425-428).
   * aud_blocks = 0: no trunk in the handle (the PyTorch-ROCm module feeds anyref_project_audio instead). */
  int32_t aud_dim, aud_blocks, aud_heads, aud_mel, aud_len, aud_kernel, aud_stride, aud_clips;
} anyref_config;

typedef struct anyref_handle anyref_handle;

/* Build an empty model on HIP device `device`. */
int anyref_create(const anyref_config* cfg, int device, anyref_handle** out);
void anyref_destroy(anyref_handle* h);
const char* anyref_last_error(anyref_handle* h); /* h may be NULL: error of the last failed create */

/*
 * Hand over one tensor under its reference state_dict name (SURVEY.md §8b "Weight names":
 * `model.visual_model.*`, `model.text_hidden_fcs.0.{0,2}.*`, `model.audio_projector.*`,
 * `model.layers.*`, `lm_head.weight`, `model.vision_tower.vision_tower.vision_model.*`,
 * `model.mm_projector.*`).  Replaces `load_state_dict` (build_sam.py:104-107,
 * eval_referseg.py:70-88).  `ptr` may be host or device memory (`is_device`); the
 * library keeps its own copy.  Unknown names are ignored and counted.
 */
int anyref_set_weight(anyref_handle* h, const char* name, const void* ptr, int is_device,
                      int dtype, const int64_t* shape, int ndim);
/* Pack / fuse / convert the weights for the chosen mode; reports missing tensors. */
int anyref_finalize(anyref_handle* h);

/*
 * AnyRefForCausalLM.generate (model/anyref.py:647-822).
 *   clip_images  f32 [B,3,clip_image,clip_image]  dev
 *   sam_images   f32 [B,3,sam_img,sam_img]        dev
 *   input_ids    i64 [B,Lmax] host; negative ids are placeholders (-200 image: expands 1->n_patches)
 *   lens         i32 [B] host: true prompt length of each row (no padding semantics: every row
 *                is decoded exactly as the reference decodes a batch of one)
 *   extra_embeds f32 [n_extra, llm_dim] dev or NULL: rows that REPLACE token embeddings 1:1
 *                (projected audio / reference-image features, anyref.py:663-702)
 *   extra_slots  i32 [n_extra,2] host: (batch row, position in input_ids) of each extra row
 *   resized_hw / orig_hw  i32 [B,2] host: sam_resized_sizes and (height,width) (anyref.py:814-818)
 *   max_new_tokens, eos_token_id (<0 disables EOS)
 * outputs
 *   out_ids   i64 [B, Lmax+max_new_tokens] host, out_lens i32 [B] host
 *   out_nseg  i32 [B] host: number of [SEG] tokens found per image (anyref.py:723-726)
 *   out_masks f32 dev: mask logits; image b, seg j at offset mask_offsets[b] + j*H_b*W_b,
 *             capacity `out_masks_cap` floats (error if exceeded); mask_offsets i64 [B] host
 *   out_low   f32 dev or NULL: low-res logits [B, max_seg, 4g, 4g] (what a DP driver all-gathers)
 *   out_hidden f32 dev or NULL: [B, llm_max_seq, llm_dim] last-layer post-norm states
 *             (`outputs.hidden_states[-1]`, anyref.py:718)
 */
int anyref_generate(anyref_handle* h, void* stream, const float* clip_images, const float* sam_images,
                    const int64_t* input_ids, const int32_t* lens, int B, int Lmax,
                    const float* extra_embeds, const int32_t* extra_slots, int n_extra,
                    const int32_t* resized_hw, const int32_t* orig_hw, int max_new_tokens,
                    int eos_token_id, int64_t* out_ids, int32_t* out_lens, int32_t* out_nseg,
                    float* out_masks, int64_t out_masks_cap, int64_t* mask_offsets, float* out_low,
                    float* out_hidden);

/*
 * Teacher-forced path of `model_forward_new` (model/anyref.py:239-430): same arithmetic with the
 * ids given, no decode loop.  [SEG] positions are searched in input_ids itself and the hidden
 * state at pos-1+255 is used (anyref.py:273-282).  `out_logits` f32 dev or NULL:
 * [B, Smax, vocab] LM logits for the caller's CE loss (losses stay in Python, anyref.py:19-68).
 */
int anyref_forward_teacher(anyref_handle* h, void* stream, const float* clip_images,
                           const float* sam_images, const int64_t* input_ids, const int32_t* lens,
                           int B, int Lmax, const float* extra_embeds, const int32_t* extra_slots,
                           int n_extra, const int32_t* rephrase_start, const int32_t* resized_hw,
                           const int32_t* orig_hw, int32_t* out_nseg, float* out_masks,
                           int64_t out_masks_cap, int64_t* mask_offsets, float* out_low,
                           float* out_hidden, float* out_logits);

/* ---- stage entry points (each is one reference function; used by the parity tests) ---- */

/* LLaVA encode_images = CLIP hidden_states[-2][:,1:] -> mm_projector (anyref.py:334).
 * out f32 [B, n_patches, llm_dim] dev; clip_feat f32 [B,n_patches,clip_dim] dev or NULL. */
int anyref_encode_images(anyref_handle* h, void* stream, const float* clip_images, int B, float* out,
                         float* clip_feat);
/* ImageEncoderViT.forward (image_encoder.py:110-125). out f32 [B, g*g, out_chans] dev (NHWC tokens;
 * the reference's NCHW [B,256,g,g] is this transposed). */
int anyref_sam_encode(anyref_handle* h, void* stream, const float* sam_images, int B, float* out);
/* prompt_encoder(text) + mask_decoder.predict_masks + postprocess_masks for one image
 * (anyref.py:797-819).  image_emb f32 [g*g, out_chans] dev, pred_emb f32 [n,out_dim] dev.
 * masks4 f32 [n,4,4g,4g] dev or NULL, iou f32 [n,4] dev or NULL,
 * out_masks f32 [n,H,W] dev or NULL (needs resized_hw, orig_hw i32[2] host). */
int anyref_mask_decode(anyref_handle* h, void* stream, const float* image_emb, const float* pred_emb,
                       int n, float* masks4, float* iou, const int32_t* resized_hw,
                       const int32_t* orig_hw, float* out_masks);

/* ---- SAM spatial prompts beside [SEG] (prompt_encoder.py:78-186) ----
 * Points, a box and a low-resolution mask join the [SEG] text embedding in one decoder pass.  Token order: points, one padding
 * point (iff points are given and boxes are not), box corners, text.  The optional weights
 * model.visual_model.prompt_encoder.{point_embeddings.{0..3}, not_a_point_embed, mask_downscaling.{0,1,3,4,6}} must have been
 * handed to anyref_set_weight before anyref_finalize. */
typedef struct anyref_spatial_prompts {
  const float* points;     /* f32 dev [n,P,2] (x,y), SAM input frame; NULL iff n_points = 0 */
  const int32_t* labels;   /* i32 dev [n,P]: 1 foreground, 0 background, -1 not a point */
  int32_t n_points;        /* P, 0 .. max_points */
  const float* boxes;      /* f32 dev [n,4] x0 y0 x1 y1, or NULL */
  const float* mask_input; /* f32 dev [n,4g,4g] low-res logits, or NULL */
  int32_t multimask;       /* 0: mask token 0;  1: tokens 1..3 */
} anyref_spatial_prompts;
/* After anyref_finalize: allocates the prompted path's workspaces for up to max_points points per prompt (counted in
 * anyref_device_bytes).  Fails, naming the first missing tensor, if the spatial weights were not handed over.  0 frees them;
 * the same value again changes nothing. */
int anyref_prompt_reserve(anyref_handle* h, int max_points);
/* anyref_mask_decode with spatial prompts.  pred_emb may be NULL: SamPredictor.predict on the given embedding.  sp NULL or
 * with nothing set: the text prompt alone, bit-identical to anyref_mask_decode.  masks4 f32 [n,4,4g,4g] or NULL, iou f32
 * [n,4] or NULL, out_masks f32 [n,k,H,W] or NULL, k = 1 (multimask 0: token 0) or 3 (tokens 1..3). */
int anyref_mask_decode_prompted(anyref_handle* h, void* stream, const float* image_emb, const float* pred_emb, int n,
                                const anyref_spatial_prompts* sp, float* masks4, float* iou, const int32_t* resized_hw,
                                const int32_t* orig_hw, float* out_masks);
/* Decodes mask `seg` of row `row` of the last anyref_generate / anyref_session_generate / anyref_session_generate_pooled
 * again, with `sp` (n = 1, may be NULL) ADDED to that [SEG]'s own prompt embedding, on that row's image embedding and sizes.
 * out_low f32 [k,4g,4g] dev or NULL, iou f32 [4] dev or NULL, out_masks f32 [k,H,W] dev or NULL.  Reads the working buffers
 * and writes decoder workspaces only: an open session, pool slots and a pending draft stay usable, mask reports are not
 * touched.  Refused with nothing queued when nothing is reserved, row / seg lie outside that call, n_points > max_points,
 * points come without labels, or another entry has overwritten the embeddings since ("refine lost: ended by <entry>";
 * anyref_refine_masks, anyref_mask_decode and anyref_mask_decode_prompted do not end it). */
int anyref_refine_masks(anyref_handle* h, void* stream, int row, int seg, const anyref_spatial_prompts* sp, float* out_low,
                        float* iou, float* out_masks);
/* The prompt embedding of mask `seg` of row `row` of the last generating call, as anyref_refine_masks reads it: out f32
 * [out_dim] dev.  With it, anyref_mask_decode_prompted on anyref_sam_encode's embedding reproduces a refine bit for bit.  Refused
 * like anyref_refine_masks (it needs no reservation). */
int anyref_refine_embedding(anyref_handle* h, void* stream, int row, int seg, float* out);
/* LLaMA stack on given input embeddings (HF LlamaModel; call sites anyref.py:341-354).
 * embeds f32 [B,S,dim] dev, lens i32[B] host.  hidden f32 [B,S,dim] (post final norm),
 * logits f32 [B,S,vocab] or NULL, attn_row f32 [B,S] or NULL = head-mean last-layer attention of
 * query `attn_q[b]` (i32[B] host) over all keys (anyref.py:748-749). */
int anyref_llm_forward(anyref_handle* h, void* stream, const float* embeds, const int32_t* lens, int B,
                       int S, float* hidden, float* logits, const int32_t* attn_q, float* attn_row);
/* n new rows per sequence behind the KV cache left by the previous anyref_llm_forward / anyref_llm_extend on
 * this handle.  embeds f32 [B,n,dim] dev; pos0, lens i32 [B] host (rows already cached; valid rows <= n);
 * hidden f32 [B,n,dim] dev (post final norm; rows >= lens[b] are left as they were); logits f32 [B,n,vocab] dev or NULL
 * (rows >= lens[b] undefined).  Error if pos0[b] + lens[b] > llm_max_seq.  The pass is the prefill code path at a position
 * offset: RoPE / cache append at pos0[b] + i, causal attention over keys [0, pos0[b] + i]. */
int anyref_llm_extend(anyref_handle* h, void* stream, const float* embeds, const int32_t* pos0,
                      const int32_t* lens, int B, int n, float* hidden, float* logits);

/* ImageBindModel.get_audio_feature, second return value (model/ImageBind/models/imagebind_model.py:477-511; call
 * sites anyref.py:313-315, :670-672), for handles created with aud_blocks > 0 and given the
 * `model.audio_encoder.*` weights: mel f32 dev [n, 1, aud_mel, aud_len] (n = clips, <= aud_clips * max_batch)
 * -> conv stem (kernel aud_kernel, stride aud_stride, no bias) + LayerNorm -> [CLS] + pos_embed -> aud_blocks
 * pre-LN blocks (MHA with add_bias_kv, GELU MLP x4) -> LayerNorm -> CLS -> Linear(aud_dim, audio_dim, no bias)
 * -> L2-normalise x min(exp(log_logit_scale), 100) -> emb f32 dev [n, audio_dim]. */
int anyref_audio_encode(anyref_handle* h, void* stream, const float* mel, int n, float* emb);

/* audio_projector = Linear(audio_dim, llm_dim) on ImageBind audio embeddings (anyref.py:161,673).
 * audio_emb f32 [n, audio_dim] dev (the ImageBind trunk itself stays a PyTorch-ROCm step) ->
 * out f32 [n, llm_dim] dev, ready to be passed as `extra_embeds`. */
int anyref_project_audio(anyref_handle* h, void* stream, const float* audio_emb, int n, float* out);

/*
 * The glue alone: everything `generate` does after `super().generate` returns (model/anyref.py:718-822) or
 * `model_forward_new` does around `super().forward` (:273-282, :356-430), on caller-provided LLM outputs --
 * [SEG] search, hidden-row gather with the reference's hard-coded image offset (+255 = n_patches - 1),
 * rephrase, text_hidden_fcs, SAM image encoder, per-image prompt encoder -> mask decoder -> postprocess.
 * This is the entry the parity tests hold against fixtures made by running the reference's own lines on
 * canned LLM outputs (tests/golden/make_golden_glue.py).
 *   ids        i64 host [B, Lmax]: `outputs.sequences` (teacher = 0) or `input_ids` (teacher = 1);
 *              a [SEG] at index p >= 1 takes hidden row p - 1 + 255 (which is `where(ids[:,1:]) + 255`
 *              of :723-726,:758 and `pos - 1 + 255` of :282)
 *   ids_lens   i32 host [B]
 *   ref_pos    i32 host [B] or NULL: rephrase start = ref_pos[b] - 1 + 255 (teacher = 0: the prompt length,
 *              :745; teacher = 1: `where(labels > 0)[0][0]`, :378)
 *   hidden     f32 dev [B, hidden_rows, llm_dim] = `hidden_states[-1]`
 *   attn_mean  f32 dev [B, hidden_rows, hidden_rows] head-mean `attentions[-1]`, needed iff rephrase_weight > 0
 *   outputs as anyref_generate.
 */
int anyref_seg_tail(anyref_handle* h, void* stream, const float* sam_images, const int64_t* ids,
                    const int32_t* ids_lens, const int32_t* ref_pos, int B, int Lmax, int teacher,
                    const float* hidden, int hidden_rows, const float* attn_mean, const int32_t* resized_hw,
                    const int32_t* orig_hw, int32_t* out_nseg, float* out_masks, int64_t out_masks_cap,
                    int64_t* mask_offsets, float* out_low);

/* Change the inclusive [SEG] id range after creation (`seg_token_idx` kwarg, anyref.py:197-200). */
int anyref_set_seg_range(anyref_handle* h, int lo, int hi);

/* Two-stream overlap of the SAM image encoder with the LLM decode (default 1).  0 keeps the whole
 * call on the caller's stream (used by bench.py to time kernels without a co-running stream). */
int anyref_set_overlap(anyref_handle* h, int on);

/* Early [SEG] masks (default 1; effective with overlap on, batch 1, no [SEG] in the prompt, and rephrase_weight 0 or
 * anyref_set_rephrase_paths on):
 * anyref_generate queues the hand-off MLP, mask decoder and postprocess of a generated [SEG] on the side stream the
 * moment the token is read, under the remaining decode steps (the reference runs them after generate() returns,
 * anyref.py:718-822; same arithmetic per prompt, one prompt per mask-decoder call).  0: all masks after the loop.
 * Under rephrasing the first [SEG]'s rephrase term is queued there too, in front of the MLP: it reads the [SEG] row's
 * query, keys [0, e0] and hidden rows [s0, e0), all final when the token is read. */
int anyref_set_early_tail(anyref_handle* h, int on);
/* masks the last anyref_generate / anyref_session_generate decoded early (0 when the path did not run) */
int anyref_early_masks_done(anyref_handle* h);

/* The rephrase branch (rephrase_weight > 0) on the fast paths (default 0).  1: the rephrase term of every
 * image is computed by one launch pair behind a device table of (image, [SEG] row, start row, output row) items
 * (anyref_op_seg_rephrase) instead of one small launch chain per image; early [SEG] masks, anyref_set_draft and
 * anyref_session_generate then serve rephrase_weight > 0 as they serve 0.  Where the pair refuses a shape the per-image
 * chain runs, and early masks stay off under rephrasing.  0: every entry queues what it queued before this switch
 * existed.  No effect with rephrase_weight 0, on anyref_forward_teacher or on anyref_seg_tail. */
int anyref_set_rephrase_paths(anyref_handle* h, int on);

/* extra_embeds produced on ANOTHER stream (e.g. the ImageBind audio trunk + audio_projector, `anyref_audio_encode` /
 * `anyref_project_audio` on a stream of the caller's): the next anyref_generate / anyref_forward_teacher on this handle makes
 * its own stream wait for `event` (a hipEvent_t recorded behind that work) just before the splice -- the first and only
 * place the rows are read -- so the trunk runs beside the CLIP tower instead of in front of the call.  One-shot: cleared
 * by the call that consumes it; NULL cancels.  The event must stay alive until that call has been queued. */
int anyref_set_extra_event(anyref_handle* h, void* event);

/* Draft-verified greedy decode.  The answers of this model are nearly constant, so a caller can propose
 * the expected continuation and have all of it checked in ONE multi-row pass over the weights instead of one pass per token.
 * Proposed continuation for the NEXT anyref_generate on this handle: draft_ids i64 [B,Kmax] host, draft_lens i32 [B]
 * (0 = no draft for that row).  Copied.  One-shot: cleared at the entry of the next anyref_generate /
 * anyref_forward_teacher whether it is used or not, and on error.  NULL cancels.  A draft never changes what is
 * generated, only how many passes it takes.
 * After prefill has chosen the first token t0, row b's draft d is cut at the first id outside [0, vocab), to
 * max_new_tokens - 1, to 64 and, for B > 1, to llm_max_seq - slen[b] - max_new_tokens (slen = spliced prompt length: a row
 * that gets ahead keeps stepping while slower rows finish and must stay inside the cache); a row whose t0 != d[0] offers
 * nothing.  If any row offers k_b >= 1 tokens, one pass runs d[0 .. k_b) at positions slen[b] .. (anyref_llm_extend's path),
 * lm_head on those rows and the accept step (anyref_op_draft_accept): with g[0] = t0, g[j + 1] = argmax(logits[j]), the
 * accepted count m_b is the number of leading j < k_b with g[j] == d[j], and g[0 .. m_b] are appended to the row (EOS and
 * max_new_tokens applied per row).  The one-token loop then continues, graph replay included, until every row has ended.
 * At most one verification pass per call.  With rephrase_weight > 0 the draft is ignored (offered = 0) unless
 * anyref_set_rephrase_paths is on: then the pass keeps the last layer's rotated queries of its rows as a decode step does
 * (rejected rows' queries are overwritten by the steps that follow, like their K and V). */
int anyref_set_draft(anyref_handle* h, const int64_t* draft_ids, const int32_t* draft_lens, int B, int Kmax);
/* After anyref_generate: per row, the draft tokens fed to the verification pass and how many were accepted;
 * decode steps launched by the call; verification passes (0 or 1).  Any pointer may be NULL. */
int anyref_draft_stats(anyref_handle* h, int32_t* offered, int32_t* accepted, int B, int32_t* decode_steps,
                       int32_t* verify_passes);

/* Token scores: how sure the greedy decode was of every token it generated.  Off by default; while off
 * nothing is launched or allocated for it.  On: every generated token of anyref_generate, anyref_session_generate and
 * anyref_session_generate_pooled -- drafted or not, graphs on or off -- carries two f32 numbers computed on the device from the
 * f32 logits row x that decided it (token_scores_kernel; anyref_op_token_scores states the rule):
 *   logprob = x[id] - logsumexp(x)      gap = x[id] - max over i != id of x[i]   (the top-2 logit gap; 0 on a tie)
 * The first switch-on allocates two f32 arrays [max_batch, llm_max_seq], indexed like the hidden states by the position of
 * the row that predicted the token.  The decode step's graph is keyed by the switch: graphs captured under one setting are
 * kept, and never replayed, under the other. */
int anyref_set_token_scores(anyref_handle* h, int on);
/* Of the last generating call, for its rows b < B: n[b] = tokens row b generated (its EOS included), and their scores in
 * generation order at logprob[b * n_cap ..] / gap[b * n_cap ..] (f32 host, [B, n_cap]; entries past n[b] are left alone).
 * Every generating call clears this state on entry; rows the call did not have report n = 0.  Error while the switch is off,
 * and if a row holds more than n_cap tokens. */
int anyref_token_scores(anyref_handle* h, int B, int n_cap, float* logprob, float* gap, int32_t* n);

/* Mask reports: what a caller wants to know about every mask without copying its f32 plane out.  Off by
 * default; while off nothing is launched or allocated for it and every call queues exactly what it queued before.  On: every
 * mask that anyref_generate, anyref_forward_teacher, anyref_seg_tail, anyref_session_generate and
 * anyref_session_generate_pooled write to out_masks is read once more on the device, right behind the kernel that wrote it
 * (mask_report_kernel; anyref_op_mask_report states the rule, anyref_amd/maskreport.py holds it), and leaves an i32 record
 *   {area #{x > 0}, area_hi #{x > offset}, area_lo #{x > -offset}, nonfinite #{NaN, +-inf}, x0, y0, x1, y1}
 * with the inclusive box of the bits x > 0 (0, 0, 0, 0 for an empty mask).  area_hi / area_lo is SAM's stability score.
 * `offset` must be finite and >= 0 (SAM's default is 1.0).  The first switch-on allocates the device records
 * [max_batch, max_seg, 8].  Exact integer arithmetic: the records of a call depend on its out_masks alone.  The decode step's
 * graphs do not depend on the switch: no report is launched inside them. */
int anyref_set_mask_reports(anyref_handle* h, int on, float offset);
/* A caller-owned device buffer of cap_words u32 words for the bit-packed masks of the NEXT mask-producing call (the five
 * above) -- one-shot, like anyref_set_draft: taken and cleared at the entry of that call, used or not, and nothing stays
 * armed after an error; NULL cancels.  Needs the switch above on at that call.  Mask j of row b, H_b x W_b, takes H_b * Wp_b
 * words, Wp_b = ceil(W_b / 32), from word pack_offsets[b] + j * H_b * Wp_b, rows in order (pack_offsets mirrors mask_offsets:
 * anyref_mask_reports returns it): bit k (LSB first) of word w of row y is x[y, 32 w + k] > 0, bits past W_b are 0.  A
 * capacity too small for the call's masks is refused where a too small out_masks_cap is. */
int anyref_set_packed_masks(anyref_handle* h, uint32_t* packed_dev, int64_t cap_words);
/* Of the last mask-producing call, for its rows b < B: n[b] = masks of row b (its out_nseg), their records at
 * rec[(b * seg_cap + j) * 8 ..] (i32 host, [B, seg_cap, 8]; entries past n[b] are left alone) and, if pack_offsets is not
 * NULL, pack_offsets[b] (i64 host [B]; meaningful when that call had a packed buffer armed).  Waits for that call's
 * stream to have produced them.  Every mask-producing call clears this state on entry; rows the call did not have report
 * n = 0.  Error while the switch is off, and if a row holds more than seg_cap masks. */
int anyref_mask_reports(anyref_handle* h, int B, int seg_cap, int32_t* n, int32_t* rec, int64_t* pack_offsets);

/*
 * Image sessions: the callers' loops ask several questions about one image (RefCOCO: ~7 expressions per image,
 * one `generate` each with the same clip_images / sam_images, eval_referseg.py:124-137).  Everything that depends only on the
 * image -- CLIP tower + projector, SAM encoder, the prefill of `system prompt + image tokens` -- is done once by
 * anyref_session_open; anyref_session_generate then prefills only each query's suffix behind that cache (anyref_llm_extend's
 * path) and decodes.  One session per handle; opening again replaces it.
 *
 *   clip_image f32 [1,3,clip_image,clip_image] dev, sam_image f32 [1,3,sam_img,sam_img] dev
 *   prefix_ids i64 [prefix_len] host: the start of every prompt, up to and INCLUDING the image placeholder (-200), which must be
 *              its last id and occur exactly once
 *   resized_hw / orig_hw i32 [2] host, as one row of anyref_generate's
 * Runs the CLIP tower and projector, the SAM encoder (on the side stream unless overlap is off; joined before the call returns
 * its work to `stream`) into image-embedding slot 0, and the ordinary prefill of the P = prefix_len + n_patches - 1 spliced
 * prefix rows into row 0 of the KV cache and of the hidden states.  Error if P + 2 > llm_max_seq.
 */
int anyref_session_open(anyref_handle* h, void* stream, const float* clip_image, const float* sam_image,
                        const int64_t* prefix_ids, int prefix_len, const int32_t* resized_hw, const int32_t* orig_hw);
/*
 * Q queries (1 <= Q <= max_batch) about the session's image in one call: a Q-row answer equals Q anyref_generate calls of one
 * row each on prefix_ids + suffix.
 *   suffix_ids i64 [Q, Lmax] host, lens i32 [Q] host (>= 1): what follows the placeholder in each prompt
 *   extra_embeds / extra_slots as anyref_generate, slot = (query, position in suffix_ids); a suffix id outside [0, vocab)
 *              must have an extra row
 *   out_ids   i64 [Q, prefix_len + Lmax + max_new_tokens] host: prefix_ids + suffix + new tokens; out_lens counts all three
 *   out_nseg, out_masks, out_masks_cap, mask_offsets, out_low, out_hidden: as anyref_generate for a batch of Q (every query
 *              has the session's image and sizes; hidden rows [0, P) of every query are the prefix's)
 * Cache rows 1 .. Q-1 receive the prefix by one copy launch (anyref_op_kv_broadcast; rows that already hold this session's
 * prefix are skipped: queries only ever write positions >= P), the suffix rows run as anyref_llm_extend's pass at pos0 = P, then
 * the greedy loop of anyref_generate (hipGraph step, EOS rules) and its masks, all after the loop: no encoder co-runs, so the
 * CU share and early masks do not apply.  A pending anyref_set_draft is honoured under the rules stated there with
 * slen[b] = P + lens[b], one-shot and consumed by this call whatever happens; anyref_draft_stats reports the call's counters.
 * Refused before anything is queued, the session staying usable: P + lens[b] + max_new_tokens > llm_max_seq, lens[b] < 1, Q
 * outside [1, max_batch], an image placeholder inside a suffix, and rephrase_weight > 0 while anyref_set_rephrase_paths is
 * off.  With it on, rephrasing is served: the term reads the query of the row that predicted the [SEG], which lies behind the
 * prompt (e0 > s0 = P + lens[b] - 1) and so comes from a decode step or a draft's pass, never from the suffix pass.
 * Any other entry that writes row 0 of the KV cache or of the hidden states, the CLIP feature buffer or image-embedding slot 0
 * ends the session: anyref_generate, anyref_forward_teacher, anyref_llm_forward, anyref_llm_extend, anyref_seg_tail,
 * anyref_encode_images, anyref_finalize.  The next anyref_session_generate then fails with "session lost: ended by <entry>".
 */
int anyref_session_generate(anyref_handle* h, void* stream, const int64_t* suffix_ids, const int32_t* lens, int Q, int Lmax,
                            const float* extra_embeds, const int32_t* extra_slots, int n_extra, int max_new_tokens,
                            int eos_token_id, int64_t* out_ids, int32_t* out_lens, int32_t* out_nseg, float* out_masks,
                            int64_t out_masks_cap, int64_t* mask_offsets, float* out_low, float* out_hidden);
/* Forget the session (anyref_destroy does the same).  No error if none is open. */
int anyref_session_close(anyref_handle* h);

/*
 * Session pool: many images resident at once, queries about different images in one call.  A session lives in
 * the working buffers (row 0 of the KV cache and of the hidden states, image-embedding slot 0), so a handle holds one, every
 * image switch pays an open, and any plain call ends it.  A pool keeps what anyref_session_open leaves behind OUTSIDE the working
 * buffers, compactly, in n_slots slots: the K and V prefix rows of every layer [2 * layers][max_prefix_rows][llm_dim] in the cache
 * element type, the hidden prefix rows [max_prefix_rows][llm_dim] f32, the SAM image embedding, and on the host the prefix ids, P,
 * the sizes and a generation counter.  A pooled call brings each row's prefix back from its slot with one gather launch
 * (anyref_op_kv_gather) and then runs as anyref_session_generate does.
 *
 * anyref_session_pool_reserve: after anyref_finalize.  Allocates the pool (counted in anyref_device_bytes; a handle that reserves
 * nothing holds exactly what it held before).  1 <= max_prefix_rows <= llm_max_seq.  Reserving again with the same sizes changes
 * nothing; with other sizes it is allowed only while every slot is empty (never stored, closed or lost); n_slots = 0,
 * max_prefix_rows = 0 frees the pool whatever it holds.  Waits for the device before it frees.
 */
int anyref_session_pool_reserve(anyref_handle* h, int n_slots, int max_prefix_rows);
/*
 * Copy the live session (anyref_session_open) into `slot`: its cache row, its hidden rows and image-embedding slot 0, by the
 * gather kernel in its pack direction (one launch for K and V of every layer, one for the hidden rows, one for the embedding).
 * Replaces whatever the slot held, under a new generation.  The live session stays live and unchanged.
 * Refused with nothing queued: no live session ("session lost: ended by <entry>" / "no session open"), P > max_prefix_rows, slot
 * outside the pool, no pool.
 */
int anyref_session_store(anyref_handle* h, void* stream, int slot);
/*
 * anyref_session_generate for rows about DIFFERENT images: its arguments plus
 *   slots i32 [Q] host: the slot query b is about.  Rows may name one slot several times or different slots; slots may have
 *              different P.
 * Schedule: (1) one gather launch brings every row's K / V prefix, all layers, from its slot into cache row b; two more launches of
 * the same kernel bring the hidden prefix rows into hidden row b and the image embedding into image-embedding slot b.  The host
 * remembers which (slot, generation) every cache row and embedding slot holds and skips the rows that already hold the right
 * prefix (queries only ever write positions >= P); every entry that ends a session, anyref_session_open and
 * anyref_session_generate clear that memory.  (2) anyref_session_generate's steps from the suffix embeddings on, with
 * pos0[b] = P[slots[b]], slen[b] = P[slots[b]] + lens[b], every row's own sizes, and the masks decoded against embedding slot b.
 *   out_ids   i64 [Q, Lout] host, Lout = np + Lmax + max_new_tokens with np the LONGEST prefix_len among the call's slots: row b
 *              is that slot's prefix_ids + suffix + new tokens from column 0 on, zero behind; out_lens counts all three
 *   out_hidden rows [0, P[slots[b]]) of query b are its slot's prefix rows
 * A row's answer does not depend on the other rows: a call about slots [a, b, c] gives row by row what the calls about one slot
 * with the same Q and lens give.  anyref_set_draft, anyref_draft_stats and anyref_set_rephrase_paths as in
 * anyref_session_generate.  The call writes row 0: it ends an unpooled live session ("session lost: ended by
 * anyref_session_generate_pooled").
 * Refused before anything is queued, the pool and a live session staying usable: a slot outside the pool, empty, or lost ("slot N
 * lost: ended by <entry>"); Q outside [1, max_batch]; P[slots[b]] + lens[b] + max_new_tokens > llm_max_seq; and
 * anyref_session_generate's own rules (lens[b] < 1, an image placeholder inside a suffix, an id without an extra row,
 * rephrase_weight > 0 with the paths switch off).
 * What ends a slot is what changes the weights: anyref_adapter_apply, anyref_update_weight, anyref_finalize.  anyref_generate and
 * every other entry that merely uses the working buffers does NOT: the next pooled call gathers again.
 */
int anyref_session_generate_pooled(anyref_handle* h, void* stream, const int32_t* slots, const int64_t* suffix_ids,
                                   const int32_t* lens, int Q, int Lmax, const float* extra_embeds, const int32_t* extra_slots,
                                   int n_extra, int max_new_tokens, int eos_token_id, int64_t* out_ids, int32_t* out_lens,
                                   int32_t* out_nseg, float* out_masks, int64_t out_masks_cap, int64_t* mask_offsets,
                                   float* out_low, float* out_hidden);
/* Empty one slot (also one that was lost).  Error if slot is outside the pool. */
int anyref_session_slot_close(anyref_handle* h, int slot);
/* Any pointer may be NULL.  slots, slots in use, bytes the pool holds on the device; cache rows the last pooled call gathered and
 * skipped; device time of that call's gather launches in ms between two events on its stream (waits for them; -1 when the call
 * launched none). */
int anyref_session_pool_stats(anyref_handle* h, int32_t* slots, int32_t* in_use, int64_t* bytes, int32_t* rows_gathered,
                              int32_t* rows_skipped, double* last_gather_ms);

/*
 * Adapter hot-swap: the reference's evaluations load a LoRA adapter each (`lora_name`), and a training run is
 * evaluated by sweeping its checkpoints (eval_reason.py:188-201).  A handle that RESERVED its LoRA targets before anyref_finalize
 * keeps their unmerged base and can be switched between adapters, and back to the base, any number of times without drift and
 * without a rebuild.  A handle that reserves nothing is unchanged in every respect (bytes, arithmetic, entry points).
 *
 * The merge rule, for a target with base w [N,K] (handed to anyref_set_weight in dtype d_in), A [r,K], B [N,r] and `scaling`
 * (= lora_alpha / r, passed as f32):
 *     acc = 0 (f64);  for j = 0 .. r-1 in this order:  acc = acc + f64(B[n,j]) * f64(A[j,k])    (f32 x f32 is exact in f64)
 *     m   = f32( acc * f64(scaling) + f64(w[n,k]) )     one f64 multiply, one f64 add, one RNE to f32
 *     m   = f32( d_in(m) )                              RNE to the dtype the base came in (identity for f32)
 *     stored = what anyref_finalize makes of an f32 tensor holding m (RNE to the mode's weight type; in PERF_FP8W / PERF_INT4W the
 *              row / group quantiser runs on the f32 rows of m)
 * anyref_amd/lora.py states it in torch; the device reproduces it bit for bit.  A target no pair names holds the base exactly as
 * anyref_finalize converted it.
 */
#define ANYREF_LORA_Q 1u
#define ANYREF_LORA_K 2u
#define ANYREF_LORA_V 4u
#define ANYREF_LORA_O 8u
#define ANYREF_LORA_GATE 16u
#define ANYREF_LORA_UP 32u
#define ANYREF_LORA_DOWN 64u
#define ANYREF_LORA_ALL 127u
/* Before anyref_finalize (an error after it): `targets` is a mask of ANYREF_LORA_* over the seven linears of every LLaMA layer
 * (Q | V is the reference's set, train.py:371-374).  anyref_finalize then keeps the raw f32 tensors of those linears instead of
 * freeing them (no copy; anyref_device_bytes counts them: 4 N K bytes per target, 4.3 GB for Q | V at 7B). */
int anyref_adapter_reserve(anyref_handle* h, uint32_t targets);
typedef struct anyref_lora_pair {
  const char* weight_name; /* the target's state_dict name, e.g. "model.layers.0.self_attn.q_proj.weight" */
  const float* A;          /* f32 [r,K]  (transposed: [r,N]) */
  const float* B;          /* f32 [N,r]  (transposed: [K,r]) */
  int32_t r;               /* 1 .. 64 */
  int32_t is_device;       /* A and B are device (1) or host (0) memory */
  int32_t transposed;      /* fan_in_fan_out adapters: delta = (B A)^T, as merge_lora transposes */
} anyref_lora_pair;
/* After anyref_finalize on a reserving handle.  SETS the reserved targets, it does not accumulate: every reserved target named in
 * `pairs` becomes base + scaling * B A by the rule above, every reserved target not named returns to its base; n_pairs = 0
 * restores the base model.  Everything is validated before anything is written (target reserved, rank 1 .. 64, no name twice,
 * non-null tensors, finite scaling; A and B must have the shapes stated above): a refused call leaves the weights, an open
 * session and a pending draft as they were.  The call then waits for the side stream (no co-running SAM encoder or early mask in
 * flight), writes the packed weight buffers IN PLACE on `stream` (no buffer moves: a captured decode graph replays the new
 * weights), ends an open image session ("session lost: ended by anyref_adapter_apply"), drops a pending anyref_set_draft and
 * returns when the writes have completed.  In the f16 modes a merged element past +-65504 fails the call naming the tensor; the
 * reserved targets are then all back at their base. */
int anyref_adapter_apply(anyref_handle* h, void* stream, const anyref_lora_pair* pairs, int n_pairs, float scaling);
/* After anyref_finalize on a reserving handle: replace one of the tensors an adapter's `modules_to_save` carries
 * (train.py:375-387), repacked into its existing buffer by the code anyref_finalize uses:
 *   model.embed_tokens.weight, lm_head.weight, model.text_hidden_fcs.0.{0,2}.{weight,bias}, model.audio_projector.{weight,bias},
 *   and under model.visual_model.mask_decoder.: mask_tokens.weight, output_upscaling.{0,1,3}.{weight,bias},
 *   output_hypernetworks_mlps.<t>.layers.<j>.{weight,bias}.
 * Arguments as anyref_set_weight.  The shape must equal the built one (a vocabulary that differs is an error naming both sizes);
 * any other name is refused.  Same session / draft consequences as anyref_adapter_apply ("ended by anyref_update_weight"). */
int anyref_update_weight(anyref_handle* h, void* stream, const char* name, const void* ptr, int is_device, int dtype,
                         const int64_t* shape, int ndim);
/* targets_reserved: reserved tensors (targets x layers); pairs_active: targets holding a merged adapter now; inexact: as
 * anyref_inexact_weights for the weights held now; last_apply_ms: device time of the last anyref_adapter_apply's merge launches
 * (a hipEvent pair around them).  Any pointer may be NULL. */
int anyref_adapter_stats(anyref_handle* h, int32_t* targets_reserved, int32_t* pairs_active, int64_t* inexact,
                         double* last_apply_ms);

/* hipGraph replay of the greedy decode step (default 1): one step is ~170 launches with fixed
 * arguments (position / next token live on the device), captured once per batch size.  0 launches
 * them eagerly; the per-kernel profiler below always runs eagerly. */
int anyref_set_graphs(anyref_handle* h, int on);

/* CU share of the side stream (generate, batch 1; default 128 workgroups over 6 steps): while the SAM encoder co-runs
 * with the decode loop, its GEMM / attention launches are capped at `wgs` workgroups (each walks several output
 * tiles), so that the decode GEMVs -- whose throughput is proportional to the CUs they get -- keep CUs of their own
 * instead of queueing behind 256 resident MFMA workgroups; the encoder's blocks are queued ceil(depth / steps) per
 * decode step, and what is left when the loop ends runs uncapped.  wgs = 0: uncapped, queued whole at the fork
 * (the behaviour for more than 4 images per call; 2 - 4 images are fed the same way at a share of their own, 160
 * workgroups over 3 steps, which this call does not change).  steps <= 0 keeps the current value.  Results are
 * bit-identical either way. */
int anyref_set_side_share(anyref_handle* h, int wgs, int steps);

/*
 * Per-kernel timing for the measurement harness (bench.py "roofline"): when enabled, every GEMM /
 * GEMV / attention launch is bracketed by a hipEvent pair on its launch stream.  After the caller
 * has synchronised the stream, anyref_profile_collect() books the elapsed times;
 * anyref_profile_read(idx) returns tag, summed ms, launch count and summed algorithmic FLOPs /
 * bytes (returns -1 past the last tag).
 */
int anyref_profile_enable(anyref_handle* h, int on);
/* Restrict timing to one tag (NULL = all) and to every `sample_every`-th launch of a tag, so the
 * event pairs do not perturb the timed region they measure. */
int anyref_profile_config(anyref_handle* h, const char* only_tag, int sample_every);
int anyref_profile_collect(anyref_handle* h);
/* Measures what an event bracket adds to the kernel inside it on `stream` (tiny-kernel differencing;
 * synchronises the stream) and takes it off every bracket booked afterwards, so a tag's time is the
 * kernel's own duration (checked against rocprofv3 --kernel-trace in profiles/).  *overhead_us
 * receives the value. */
int anyref_profile_calibrate(anyref_handle* h, void* stream, double* overhead_us);
int anyref_profile_read(anyref_handle* h, int idx, char* name, int cap, double* ms, int64_t* count,
                        double* flops, double* bytes);

/*
 * Kernel-side timestamps for the measurement harness (bench.py "roofline", in situ): hipEvent brackets cannot be
 * placed inside a replayed hipGraph and rocprofv3 serialises the call's two streams, so neither sees a decode GEMV
 * as it runs in production.  With stamps enabled every decode-GEMV workgroup writes {earliest wave start, latest
 * wave end} of the 100 MHz wall clock into its own slot (plain stores); a launch's duration is max(end) - min(start)
 * over its workgroups.  Works inside graph replay (the captured step is re-captured with stamp slots addressed by a
 * device-side replay counter) and beside the second stream.  Costs one uniform branch when off.
 * anyref_stamps_collect() (after the caller has synchronised the device) reduces the slots and returns the number of
 * launches recorded since enable / the last collect, in start-time order; anyref_stamps_read(idx) returns one launch:
 * tag (the rocprofv3-visible instantiation, as in anyref_profile_read), start / end in microseconds relative to the
 * first launch, algorithmic bytes, and the replay index of its captured step (-1: eager launch).
 */
int anyref_stamps_enable(anyref_handle* h, int on);
int anyref_stamps_collect(anyref_handle* h, int64_t* count);
/* launches that went UNSTAMPED since enable / the last collect -- a step larger than the per-step record, or graph replays past
 * the epoch capacity (48): read it BEFORE anyref_stamps_collect (which resets it); non-zero means per-step averages built on the
 * collected rows miss launches */
int anyref_stamps_dropped(anyref_handle* h, int64_t* count);
int anyref_stamps_read(anyref_handle* h, int64_t idx, char* name, int cap, double* t0_us, double* t1_us,
                       double* bytes, int* epoch);
/* the same launch's spread over its workgroups: last start - first start (dispatch ramp), last end - first end (tail),
 * and the median workgroup's own start-to-end span */
int anyref_stamps_spread(anyref_handle* h, int64_t idx, double* start_spread_us, double* end_spread_us,
                         double* wg_median_us);

/* Bytes of HBM the handle holds (weights + workspaces), for sizing reports. */
int64_t anyref_device_bytes(anyref_handle* h);
/* Name of the compute mode's arithmetic ("f32" / "bf16" / "f16" ...). */
const char* anyref_mode_name(anyref_handle* h);
/* After anyref_finalize, in every mode: *out = the number of weight elements the handle holds in a value other than the one
 * handed to anyref_set_weight (rounded to the mode's 16-bit type, or quantised to fp8 and back in ANYREF_MODE_PERF_FP8W, or to int4
 * groups and back in ANYREF_MODE_PERF_INT4W).
 * 0 in PARITY; 0 in PERF_F16 for an fp16 checkpoint; in PERF that checkpoint loses 3 mantissa bits in most elements. */
int anyref_inexact_weights(anyref_handle* h, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ANYREF_HIP_H */
