// extern "C" boundary of libanyref_hip.so (include/anyref_hip.h).  Exceptions never cross it:
// every entry point returns a status and stores the text for anyref_last_error().
#include <cstring>
#include <string>

#include "model.h"

using namespace anyref;

struct anyref_handle {
  std::unique_ptr<ModelBase> m;
  std::string err;
  std::vector<StampRow> stamp_rows;  // last anyref_stamps_collect()
};

static thread_local std::string g_create_err;

#define GUARD(h, body)                         \
  if (!(h) || !(h)->m) return 1;               \
  try {                                        \
    struct ProfInstall {                       \
      ProfInstall(Profiler* p, Stamper* t) { g_prof = p; g_stamp = t; } \
      ~ProfInstall() { g_prof = nullptr; g_stamp = nullptr; }            \
    } _pi(&(h)->m->prof, &(h)->m->stamp);      \
    body;                                      \
    hipError_t _e = hipGetLastError();         \
    if (_e != hipSuccess) {                    \
      (h)->err = std::string("HIP error: ") + hipGetErrorString(_e); \
      return 3;                                \
    }                                          \
    return 0;                                  \
  } catch (const std::exception& e) {          \
    (h)->err = e.what();                       \
    return 2;                                  \
  }

extern "C" {

int anyref_create(const anyref_config* cfg, int device, anyref_handle** out) {
  try {
    if (!cfg || !out) throw std::runtime_error("null argument");
    if (cfg->abi_version != ANYREF_ABI_VERSION) throw std::runtime_error("anyref_config ABI version mismatch");
    if (cfg->max_batch < 1 || cfg->max_seg < 1) throw std::runtime_error("max_batch / max_seg must be >= 1");
    if (cfg->llm_dim % cfg->llm_heads || cfg->clip_dim % cfg->clip_heads || cfg->sam_dim % cfg->sam_heads)
      throw std::runtime_error("hidden sizes must be divisible by the head counts");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
      throw std::runtime_error("no HIP device visible: the AnyRef HIP backend needs an MI355X (there is no CPU fallback)");
    if (device < 0 || device >= ndev) throw std::runtime_error("device index out of range");
    auto* h = new anyref_handle();
    h->m = make_model(*cfg, device);
    *out = h;
    return 0;
  } catch (const std::exception& e) {
    g_create_err = e.what();
    return 2;
  }
}

void anyref_destroy(anyref_handle* h) { delete h; }

const char* anyref_last_error(anyref_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int anyref_set_weight(anyref_handle* h, const char* name, const void* ptr, int is_device, int dtype,
                      const int64_t* shape, int ndim) {
  GUARD(h, h->m->set_weight(name, ptr, is_device, dtype, shape, ndim));
}

int anyref_finalize(anyref_handle* h) { GUARD(h, h->m->end_session("anyref_finalize"); h->m->end_slots("anyref_finalize"); h->m->refine_forget("anyref_finalize"); h->m->finalize()); }

int anyref_generate(anyref_handle* h, void* stream, const float* clip_images, const float* sam_images,
                    const int64_t* input_ids, const int32_t* lens, int B, int Lmax, const float* extra_embeds,
                    const int32_t* extra_slots, int n_extra, const int32_t* resized_hw, const int32_t* orig_hw,
                    int max_new_tokens, int eos_token_id, int64_t* out_ids, int32_t* out_lens, int32_t* out_nseg,
                    float* out_masks, int64_t out_masks_cap, int64_t* mask_offsets, float* out_low,
                    float* out_hidden) {
  GUARD(h, h->m->end_session("anyref_generate"); h->m->refine_begin("anyref_generate"); h->m->generate((hipStream_t)stream, clip_images, sam_images, input_ids, lens, B, Lmax, extra_embeds,
                          extra_slots, n_extra, resized_hw, orig_hw, max_new_tokens, eos_token_id, out_ids,
                          out_lens, out_nseg, out_masks, out_masks_cap, mask_offsets, out_low, out_hidden));
}

int anyref_forward_teacher(anyref_handle* h, void* stream, const float* clip_images, const float* sam_images,
                           const int64_t* input_ids, const int32_t* lens, int B, int Lmax,
                           const float* extra_embeds, const int32_t* extra_slots, int n_extra,
                           const int32_t* rephrase_start, const int32_t* resized_hw, const int32_t* orig_hw,
                           int32_t* out_nseg, float* out_masks, int64_t out_masks_cap, int64_t* mask_offsets,
                           float* out_low, float* out_hidden, float* out_logits) {
  GUARD(h, h->m->end_session("anyref_forward_teacher"); h->m->refine_forget("anyref_forward_teacher"); h->m->forward_teacher((hipStream_t)stream, clip_images, sam_images, input_ids, lens, B, Lmax,
                                 extra_embeds, extra_slots, n_extra, rephrase_start, resized_hw, orig_hw, out_nseg,
                                 out_masks, out_masks_cap, mask_offsets, out_low, out_hidden, out_logits));
}

int anyref_encode_images(anyref_handle* h, void* stream, const float* clip_images, int B, float* out,
                         float* clip_feat) {
  GUARD(h, h->m->end_session("anyref_encode_images"); h->m->encode_images((hipStream_t)stream, clip_images, B, out, clip_feat));
}

int anyref_sam_encode(anyref_handle* h, void* stream, const float* sam_images, int B, float* out) {
  GUARD(h, h->m->refine_forget("anyref_sam_encode"); h->m->sam_encode((hipStream_t)stream, sam_images, B, out));
}

int anyref_mask_decode(anyref_handle* h, void* stream, const float* image_emb, const float* pred_emb, int n,
                       float* masks4, float* iou, const int32_t* resized_hw, const int32_t* orig_hw,
                       float* out_masks) {
  GUARD(h, h->m->mask_decode((hipStream_t)stream, image_emb, pred_emb, n, masks4, iou, resized_hw, orig_hw, out_masks));
}

int anyref_prompt_reserve(anyref_handle* h, int max_points) { GUARD(h, h->m->prompt_reserve(max_points)); }

int anyref_mask_decode_prompted(anyref_handle* h, void* stream, const float* image_emb, const float* pred_emb, int n,
                                const anyref_spatial_prompts* sp, float* masks4, float* iou, const int32_t* resized_hw,
                                const int32_t* orig_hw, float* out_masks) {
  GUARD(h, h->m->mask_decode_prompted((hipStream_t)stream, image_emb, pred_emb, n, sp, masks4, iou, resized_hw, orig_hw, out_masks));
}

int anyref_refine_masks(anyref_handle* h, void* stream, int row, int seg, const anyref_spatial_prompts* sp, float* out_low,
                        float* iou, float* out_masks) {
  GUARD(h, h->m->refine_masks((hipStream_t)stream, row, seg, sp, out_low, iou, out_masks));
}

int anyref_refine_embedding(anyref_handle* h, void* stream, int row, int seg, float* out) {
  GUARD(h, h->m->refine_embedding((hipStream_t)stream, row, seg, out));
}

int anyref_llm_forward(anyref_handle* h, void* stream, const float* embeds, const int32_t* lens, int B, int S,
                       float* hidden, float* logits, const int32_t* attn_q, float* attn_row) {
  GUARD(h, h->m->end_session("anyref_llm_forward"); h->m->llm_forward((hipStream_t)stream, embeds, lens, B, S, hidden, logits, attn_q, attn_row));
}

int anyref_llm_extend(anyref_handle* h, void* stream, const float* embeds, const int32_t* pos0, const int32_t* lens, int B,
                      int n, float* hidden, float* logits) {
  GUARD(h, h->m->end_session("anyref_llm_extend"); h->m->llm_extend((hipStream_t)stream, embeds, pos0, lens, B, n, hidden, logits));
}

int anyref_session_open(anyref_handle* h, void* stream, const float* clip_image, const float* sam_image,
                        const int64_t* prefix_ids, int prefix_len, const int32_t* resized_hw, const int32_t* orig_hw) {
  GUARD(h, h->m->refine_forget("anyref_session_open"); h->m->session_open((hipStream_t)stream, clip_image, sam_image, prefix_ids, prefix_len, resized_hw, orig_hw));
}

int anyref_session_generate(anyref_handle* h, void* stream, const int64_t* suffix_ids, const int32_t* lens, int Q, int Lmax,
                            const float* extra_embeds, const int32_t* extra_slots, int n_extra, int max_new_tokens,
                            int eos_token_id, int64_t* out_ids, int32_t* out_lens, int32_t* out_nseg, float* out_masks,
                            int64_t out_masks_cap, int64_t* mask_offsets, float* out_low, float* out_hidden) {
  GUARD(h, h->m->refine_begin("anyref_session_generate"); h->m->session_generate((hipStream_t)stream, suffix_ids, lens, Q, Lmax, extra_embeds, extra_slots, n_extra,
                                  max_new_tokens, eos_token_id, out_ids, out_lens, out_nseg, out_masks, out_masks_cap,
                                  mask_offsets, out_low, out_hidden));
}

int anyref_session_close(anyref_handle* h) { GUARD(h, h->m->session_close()); }

int anyref_session_pool_reserve(anyref_handle* h, int n_slots, int max_prefix_rows) {
  GUARD(h, h->m->session_pool_reserve(n_slots, max_prefix_rows));
}

int anyref_session_store(anyref_handle* h, void* stream, int slot) { GUARD(h, h->m->session_store((hipStream_t)stream, slot)); }

int anyref_session_generate_pooled(anyref_handle* h, void* stream, const int32_t* slots, const int64_t* suffix_ids,
                                   const int32_t* lens, int Q, int Lmax, const float* extra_embeds, const int32_t* extra_slots,
                                   int n_extra, int max_new_tokens, int eos_token_id, int64_t* out_ids, int32_t* out_lens,
                                   int32_t* out_nseg, float* out_masks, int64_t out_masks_cap, int64_t* mask_offsets,
                                   float* out_low, float* out_hidden) {
  GUARD(h, h->m->refine_begin("anyref_session_generate_pooled"); h->m->session_generate_pooled((hipStream_t)stream, slots, suffix_ids, lens, Q, Lmax, extra_embeds, extra_slots, n_extra,
                                         max_new_tokens, eos_token_id, out_ids, out_lens, out_nseg, out_masks, out_masks_cap,
                                         mask_offsets, out_low, out_hidden));
}

int anyref_session_slot_close(anyref_handle* h, int slot) { GUARD(h, h->m->session_slot_close(slot)); }

int anyref_session_pool_stats(anyref_handle* h, int32_t* slots, int32_t* in_use, int64_t* bytes, int32_t* rows_gathered,
                              int32_t* rows_skipped, double* last_gather_ms) {
  GUARD(h, h->m->session_pool_stats(slots, in_use, bytes, rows_gathered, rows_skipped, last_gather_ms));
}

int anyref_set_draft(anyref_handle* h, const int64_t* draft_ids, const int32_t* draft_lens, int B, int Kmax) {
  GUARD(h, h->m->set_draft(draft_ids, draft_lens, B, Kmax));
}

int anyref_draft_stats(anyref_handle* h, int32_t* offered, int32_t* accepted, int B, int32_t* decode_steps,
                       int32_t* verify_passes) {
  GUARD(h, h->m->draft_stats(offered, accepted, B, decode_steps, verify_passes));
}

int anyref_set_token_scores(anyref_handle* h, int on) { GUARD(h, h->m->set_token_scores(on != 0)); }

int anyref_token_scores(anyref_handle* h, int B, int n_cap, float* logprob, float* gap, int32_t* n) {
  GUARD(h, h->m->token_scores(B, n_cap, logprob, gap, n));
}

int anyref_set_mask_reports(anyref_handle* h, int on, float offset) { GUARD(h, h->m->set_mask_reports(on != 0, offset)); }

int anyref_set_packed_masks(anyref_handle* h, uint32_t* packed_dev, int64_t cap_words) {
  GUARD(h, h->m->set_packed_masks(packed_dev, cap_words));
}

int anyref_mask_reports(anyref_handle* h, int B, int seg_cap, int32_t* n, int32_t* rec, int64_t* pack_offsets) {
  GUARD(h, h->m->mask_reports(B, seg_cap, n, rec, pack_offsets));
}

int anyref_adapter_reserve(anyref_handle* h, uint32_t targets) { GUARD(h, h->m->adapter_reserve(targets)); }

int anyref_adapter_apply(anyref_handle* h, void* stream, const anyref_lora_pair* pairs, int n_pairs, float scaling) {
  GUARD(h, h->m->adapter_apply((hipStream_t)stream, pairs, n_pairs, scaling));
}

int anyref_update_weight(anyref_handle* h, void* stream, const char* name, const void* ptr, int is_device, int dtype,
                         const int64_t* shape, int ndim) {
  GUARD(h, h->m->update_weight((hipStream_t)stream, name, ptr, is_device, dtype, shape, ndim));
}

int anyref_adapter_stats(anyref_handle* h, int32_t* targets_reserved, int32_t* pairs_active, int64_t* inexact,
                         double* last_apply_ms) {
  GUARD(h, h->m->adapter_stats(targets_reserved, pairs_active, inexact, last_apply_ms));
}

int anyref_audio_encode(anyref_handle* h, void* stream, const float* mel, int n, float* emb) {
  GUARD(h, h->m->audio_encode((hipStream_t)stream, mel, n, emb));
}

int anyref_project_audio(anyref_handle* h, void* stream, const float* audio_emb, int n, float* out) {
  GUARD(h, h->m->project_audio((hipStream_t)stream, audio_emb, n, out));
}

int anyref_seg_tail(anyref_handle* h, void* stream, const float* sam_images, const int64_t* ids,
                    const int32_t* ids_lens, const int32_t* ref_pos, int B, int Lmax, int teacher, const float* hidden,
                    int hidden_rows, const float* attn_mean, const int32_t* resized_hw, const int32_t* orig_hw,
                    int32_t* out_nseg, float* out_masks, int64_t out_masks_cap, int64_t* mask_offsets, float* out_low) {
  GUARD(h, h->m->end_session("anyref_seg_tail"); h->m->refine_forget("anyref_seg_tail"); h->m->seg_tail((hipStream_t)stream, sam_images, ids, ids_lens, ref_pos, B, Lmax, teacher, hidden,
                          hidden_rows, attn_mean, resized_hw, orig_hw, out_nseg, out_masks, out_masks_cap,
                          mask_offsets, out_low));
}

int anyref_set_seg_range(anyref_handle* h, int lo, int hi) { GUARD(h, h->m->set_seg_range(lo, hi)); }

int anyref_set_overlap(anyref_handle* h, int on) { GUARD(h, h->m->set_overlap(on != 0)); }
int anyref_set_early_tail(anyref_handle* h, int on) { GUARD(h, h->m->set_early_tail(on != 0)); }
int anyref_early_masks_done(anyref_handle* h) { return h && h->m ? h->m->early_masks_done() : 0; }
int anyref_set_rephrase_paths(anyref_handle* h, int on) { GUARD(h, h->m->set_rephrase_paths(on != 0)); }
int anyref_set_extra_event(anyref_handle* h, void* event) { GUARD(h, h->m->set_extra_event(event)); }

int anyref_set_graphs(anyref_handle* h, int on) { GUARD(h, h->m->set_graphs(on != 0)); }
int anyref_set_side_share(anyref_handle* h, int wgs, int steps) { GUARD(h, h->m->set_side_share(wgs, steps)); }

int anyref_profile_enable(anyref_handle* h, int on) {
  GUARD(h, {
    h->m->prof.on = on != 0;
    if (on) h->m->prof.reset();
  });
}

int anyref_profile_config(anyref_handle* h, const char* only_tag, int sample_every) {
  GUARD(h, {
    h->m->prof.filter = only_tag ? only_tag : "";
    h->m->prof.sample_every = sample_every > 1 ? sample_every : 1;
  });
}

int anyref_profile_collect(anyref_handle* h) { GUARD(h, h->m->prof.collect()); }

int anyref_profile_calibrate(anyref_handle* h, void* stream, double* overhead_us) {
  GUARD(h, {
    h->m->prof.calibrate((hipStream_t)stream);
    if (overhead_us) *overhead_us = h->m->prof.null_ms * 1e3;
  });
}

int anyref_profile_read(anyref_handle* h, int idx, char* name, int cap, double* ms, int64_t* count, double* flops,
                        double* bytes) {
  if (!h || !h->m) return -1;
  auto st = h->m->prof.stats();
  if (idx < 0 || idx >= (int)st.size()) return -1;
  snprintf(name, cap, "%s", st[idx].first.c_str());
  *ms = st[idx].second.ms;
  *count = st[idx].second.count;
  *flops = st[idx].second.flops;
  *bytes = st[idx].second.bytes;
  return 0;
}

int anyref_stamps_enable(anyref_handle* h, int on) { GUARD(h, h->m->stamp.enable(on != 0)); }

int anyref_stamps_dropped(anyref_handle* h, int64_t* count) {
  GUARD(h, {
    if (!count) throw std::runtime_error("null argument");
    *count = h->m->stamp.dropped();
  });
}
int anyref_stamps_collect(anyref_handle* h, int64_t* count) {
  GUARD(h, {
    h->stamp_rows = h->m->stamp.collect();
    if (count) *count = (int64_t)h->stamp_rows.size();
  });
}

int anyref_stamps_read(anyref_handle* h, int64_t idx, char* name, int cap, double* t0_us, double* t1_us, double* bytes,
                       int* epoch) {
  if (!h || idx < 0 || idx >= (int64_t)h->stamp_rows.size()) return -1;
  const StampRow& r = h->stamp_rows[(size_t)idx];
  snprintf(name, cap, "%s", r.tag.c_str());
  *t0_us = r.t0_us;
  *t1_us = r.t1_us;
  *bytes = r.bytes;
  if (epoch) *epoch = r.epoch;
  return 0;
}

int anyref_stamps_spread(anyref_handle* h, int64_t idx, double* start_spread_us, double* end_spread_us, double* wg_median_us) {
  if (!h || idx < 0 || idx >= (int64_t)h->stamp_rows.size()) return -1;
  const StampRow& r = h->stamp_rows[(size_t)idx];
  *start_spread_us = r.start_spread_us;
  *end_spread_us = r.end_spread_us;
  *wg_median_us = r.wg_median_us;
  return 0;
}

int64_t anyref_device_bytes(anyref_handle* h) { return h && h->m ? h->m->device_bytes() : 0; }

int anyref_inexact_weights(anyref_handle* h, int64_t* out) {
  GUARD(h, {
    if (!out) throw std::runtime_error("anyref_inexact_weights: out is NULL");
    *out = h->m->inexact_weights();
  });
}

const char* anyref_mode_name(anyref_handle* h) { return h && h->m ? h->m->mode_name() : ""; }

}  // extern "C"
