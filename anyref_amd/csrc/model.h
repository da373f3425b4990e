// Host-side model: weight store, packed weights, workspaces, stage orchestration.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/anyref_hip.h"
#include "kernels.h"
#include "prompt_encode.h"

namespace anyref {

struct RawTensor {
  float* p = nullptr;  // f32 device copy
  int dtype = ANYREF_F32;  // the type it was handed to set_weight in (every such value is exact in the f32 copy)
  std::vector<int64_t> shape;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

// Mode-independent interface behind the C-ABI.
class ModelBase {
 public:
  explicit ModelBase(const anyref_config& c, int device);
  virtual ~ModelBase();

  void set_weight(const char* name, const void* ptr, int is_device, int dtype, const int64_t* shape, int ndim);
  virtual void finalize() = 0;
  virtual const char* mode_name() const = 0;

  virtual void generate(hipStream_t s, const float* clip_images, const float* sam_images, const int64_t* input_ids,
                        const int32_t* lens, int B, int Lmax, const float* extra_embeds,
                        const int32_t* extra_slots, int n_extra, const int32_t* resized_hw, const int32_t* orig_hw,
                        int max_new_tokens, int eos_token_id, int64_t* out_ids, int32_t* out_lens,
                        int32_t* out_nseg, float* out_masks, int64_t out_masks_cap, int64_t* mask_offsets,
                        float* out_low, float* out_hidden) = 0;
  virtual void forward_teacher(hipStream_t s, const float* clip_images, const float* sam_images,
                               const int64_t* input_ids, const int32_t* lens, int B, int Lmax,
                               const float* extra_embeds, const int32_t* extra_slots, int n_extra,
                               const int32_t* rephrase_start, const int32_t* resized_hw, const int32_t* orig_hw,
                               int32_t* out_nseg, float* out_masks, int64_t out_masks_cap, int64_t* mask_offsets,
                               float* out_low, float* out_hidden, float* out_logits) = 0;
  virtual void encode_images(hipStream_t s, const float* clip_images, int B, float* out, float* clip_feat) = 0;
  virtual void sam_encode(hipStream_t s, const float* sam_images, int B, float* out) = 0;
  virtual void mask_decode(hipStream_t s, const float* image_emb, const float* pred_emb, int n, float* masks4,
                           float* iou, const int32_t* resized_hw, const int32_t* orig_hw, float* out_masks) = 0;
  // ---- SAM spatial prompts beside [SEG] (anyref_prompt_reserve / _mask_decode_prompted / _refine_masks) ----
  virtual void prompt_reserve(int max_points) = 0;
  virtual void mask_decode_prompted(hipStream_t s, const float* image_emb, const float* pred_emb, int n,
                                    const anyref_spatial_prompts* sp, float* masks4, float* iou, const int32_t* resized_hw,
                                    const int32_t* orig_hw, float* out_masks) = 0;
  virtual void refine_masks(hipStream_t s, int row, int seg, const anyref_spatial_prompts* sp, float* out_low, float* iou,
                            float* out_masks) = 0;
  virtual void refine_embedding(hipStream_t s, int row, int seg, float* out) = 0;
  // where mask (row, seg) of the last generating call came from: rows [pred_row0, pred_row0 + n) of the prompt embeddings,
  // image-embedding slot emb_slot, and the row's sizes
  struct RefineRow {
    int pred_row0 = 0, n = 0, emb_slot = 0;
    int32_t rhw[2] = {0, 0}, ohw[2] = {0, 0};
  };
  std::vector<RefineRow> refine_rows_;
  const char* refine_lost_by_ = nullptr;  // entry that overwrote what a refine reads (for the error text)
  bool refine_arm_ = false;               // the running call is a generating one: run_tail records its rows
  // every entry that writes the image embeddings or the prompt embeddings calls one of the two first (api.hip)
  void refine_forget(const char* by) {
    if (!refine_rows_.empty()) refine_lost_by_ = by;
    refine_rows_.clear();
    refine_arm_ = false;
  }
  void refine_begin(const char* by) {
    refine_forget(by);
    refine_arm_ = true;
  }
  virtual void llm_forward(hipStream_t s, const float* embeds, const int32_t* lens, int B, int S, float* hidden,
                           float* logits, const int32_t* attn_q, float* attn_row) = 0;
  virtual void llm_extend(hipStream_t s, const float* embeds, const int32_t* pos0, const int32_t* lens, int B, int n,
                          float* hidden, float* logits) = 0;
  // image sessions (anyref_session_*)
  virtual void session_open(hipStream_t s, const float* clip_image, const float* sam_image, const int64_t* prefix_ids,
                            int prefix_len, const int32_t* resized_hw, const int32_t* orig_hw) = 0;
  virtual void session_generate(hipStream_t s, const int64_t* suffix_ids, const int32_t* lens, int Q, int Lmax,
                                const float* extra_embeds, const int32_t* extra_slots, int n_extra, int max_new_tokens,
                                int eos_token_id, int64_t* out_ids, int32_t* out_lens, int32_t* out_nseg, float* out_masks,
                                int64_t out_masks_cap, int64_t* mask_offsets, float* out_low, float* out_hidden) = 0;
  void session_close() {
    sess_live_ = false;
    sess_lost_by_ = nullptr;
  }
  // the entries that write what a session keeps on the device call this first (api.hip): the one flag, and who cleared it
  void end_session(const char* by) {
    if (sess_live_) sess_lost_by_ = by;
    sess_live_ = false;
    forget_rows();
  }
  // ---- session pool (anyref_session_pool_* / _store / _generate_pooled) ----
  virtual void session_pool_reserve(int n_slots, int max_prefix_rows) = 0;
  virtual void session_store(hipStream_t s, int slot) = 0;
  virtual void session_generate_pooled(hipStream_t s, const int32_t* slots, const int64_t* suffix_ids, const int32_t* lens, int Q,
                                       int Lmax, const float* extra_embeds, const int32_t* extra_slots, int n_extra,
                                       int max_new_tokens, int eos_token_id, int64_t* out_ids, int32_t* out_lens,
                                       int32_t* out_nseg, float* out_masks, int64_t out_masks_cap, int64_t* mask_offsets,
                                       float* out_low, float* out_hidden) = 0;
  void session_slot_close(int slot) {
    if (slot < 0 || slot >= (int)pool_.size()) throw std::runtime_error("session_slot_close: slot outside the pool");
    pool_[slot] = PoolSlot();
  }
  void session_pool_stats(int32_t* slots, int32_t* in_use, int64_t* bytes, int32_t* gathered, int32_t* skipped, double* gather_ms);
  // what one slot holds on the host; the device part sits at the slot's index in pool_kv_ / pool_hid_ / pool_emb_
  struct PoolSlot {
    bool used = false;
    const char* lost_by = nullptr;  // entry that ended it (for the error text); a store or a close clears it
    int P = 0;
    int64_t gen = 0;                // stamped by every store: a cache row holds a slot's prefix only under the same generation
    std::vector<int64_t> prefix;
    int32_t rhw[2] = {0, 0}, ohw[2] = {0, 0};
  };
  // the entries that change the weights (anyref_adapter_apply, anyref_update_weight, anyref_finalize) end every slot
  void end_slots(const char* by) {
    for (auto& sl : pool_)
      if (sl.used) {
        sl = PoolSlot();
        sl.lost_by = by;
      }
  }
  // which (slot, generation) cache row b and image-embedding slot b hold (they are written together); every entry that writes
  // the working buffers forgets
  void forget_rows() { row_tag_.assign(row_tag_.size(), {-1, 0}); }
  std::vector<PoolSlot> pool_;
  int pool_maxP_ = 0;
  int64_t pool_gen_ = 0, pool_bytes_ = 0;
  void *pool_kv_ = nullptr, *pool_hid_ = nullptr, *pool_emb_ = nullptr;
  std::vector<std::pair<int, int64_t>> row_tag_;
  int pool_gathered_ = 0, pool_skipped_ = 0;  // rows of the last pooled call
  void *pool_ev0_ = nullptr, *pool_ev1_ = nullptr;  // hipEvent_t around the last gather
  bool pool_timed_ = false;
  // ---- adapter hot-swap (anyref_adapter_*) ----
  // before finalize: the LLaMA linears named by `targets` (ANYREF_LORA_* bits) keep their raw f32 tensor past finalize
  void adapter_reserve(uint32_t targets) {
    if (finalized_) throw std::runtime_error("anyref_adapter_reserve after anyref_finalize: reserve before the weights are packed");
    if (targets == 0 || (targets & ~(uint32_t)ANYREF_LORA_ALL))
      throw std::runtime_error("anyref_adapter_reserve: targets must be a non-empty mask of ANYREF_LORA_* bits");
    resv_mask_ = targets;
  }
  virtual void adapter_apply(hipStream_t s, const anyref_lora_pair* pairs, int n_pairs, float scaling) = 0;
  virtual void update_weight(hipStream_t s, const char* name, const void* ptr, int is_device, int dtype, const int64_t* shape,
                             int ndim) = 0;
  void adapter_stats(int32_t* targets_reserved, int32_t* pairs_active, int64_t* inexact, double* last_apply_ms) const {
    if (targets_reserved) *targets_reserved = (int32_t)lora_targets_.size();
    if (pairs_active) *pairs_active = pairs_active_;
    if (inexact) *inexact = inexact_weights();
    if (last_apply_ms) *last_apply_ms = last_apply_ms_;
  }
  // one reserved LoRA target: the unmerged base (the raw tensor finalize would have freed) and where its packed rows live
  struct LoraTarget {
    std::string name;
    float* base = nullptr;  // f32 [N, K], owned (tracked in allocs_)
    int d_in = ANYREF_F32;  // dtype it was handed over in
    int N = 0, K = 0;
    int layer = 0, kind = 0;  // kind: bit index of ANYREF_LORA_* (q k v o gate up down)
    int r = 0;                // rank merged into the packed rows now (0: the base)
    int64_t inexact = 0;      // elements of the packed rows that are not exactly the merged value
  };
  virtual void project_audio(hipStream_t s, const float* audio_emb, int n, float* out) = 0;
  virtual void audio_encode(hipStream_t s, const float* mel, int n, float* emb) = 0;
  virtual void seg_tail(hipStream_t s, const float* sam_images, const int64_t* ids, const int32_t* ids_lens,
                        const int32_t* ref_pos, int B, int Lmax, int teacher, const float* hidden, int hidden_rows,
                        const float* attn_mean, const int32_t* resized_hw, const int32_t* orig_hw,
                        int32_t* out_nseg, float* out_masks, int64_t out_masks_cap, int64_t* mask_offsets,
                        float* out_low) = 0;

  int64_t device_bytes() const { return bytes_; }
  // weight elements held in a value other than the one handed to set_weight (16-bit / fp8 packing at finalize)
  int64_t inexact_weights() const {
    if (!finalized_) throw std::runtime_error("inexact_weights before finalize");
    return inexact_;
  }
  void set_seg_range(int lo, int hi) {
    cfg.seg_lo = lo;
    cfg.seg_hi = hi;
  }
  // two-stream overlap of the SAM encoder with the LLM decode (default on; measurement harness can
  // switch it off to time kernels without a co-running stream)
  void set_overlap(bool on) { overlap_ = on; }
  // masks of generated [SEG]s decoded on the side stream while the greedy loop goes on (default on; batch 1)
  void set_early_tail(bool on) { early_off_ = !on; }
  // rephrase_weight > 0 on the fused launch pair, and with it under early masks, drafts and sessions (default off:
  // anyref_set_rephrase_paths)
  void set_rephrase_paths(bool on) { reph_paths_ = on; }
  // masks the last generating call decoded early (anyref_early_masks_done)
  int early_masks_done() const { return early_masks_last_; }
  // the NEXT generate / forward_teacher waits for this event on its stream just before it reads extra_embeds (the splice):
  // the caller may produce them (ImageBind audio trunk + projector) on a stream of its own, beside the CLIP tower
  void set_extra_event(void* ev) { extra_ev_ = ev; }
  void* extra_ev_ = nullptr;
  // proposed continuation for the NEXT generate (anyref_set_draft): one-shot, taken (and cleared) at its entry
  static constexpr int kDraftCap = 64;  // tokens per row a verification pass is fed at most
  void set_draft(const int64_t* ids, const int32_t* lens, int B, int Kmax) {
    draft_ids_.clear();  // (a refused call leaves nothing armed either)
    if (!ids || !lens) return;
    if (B < 1 || B > cfg.max_batch || Kmax < 0) throw std::runtime_error("set_draft: bad batch / Kmax");
    std::vector<std::vector<int64_t>> d(B);
    for (int b = 0; b < B; ++b) {
      if (lens[b] < 0 || lens[b] > Kmax) throw std::runtime_error("set_draft: draft_lens[b] outside [0, Kmax]");
      d[b].assign(ids + (size_t)b * Kmax, ids + (size_t)b * Kmax + lens[b]);
    }
    draft_ids_.swap(d);
  }
  void draft_stats(int32_t* offered, int32_t* accepted, int B, int32_t* decode_steps, int32_t* verify_passes) const {
    for (int b = 0; b < B; ++b) {
      if (offered) offered[b] = b < (int)stat_offered_.size() ? stat_offered_[b] : 0;
      if (accepted) accepted[b] = b < (int)stat_accepted_.size() ? stat_accepted_[b] : 0;
    }
    if (decode_steps) *decode_steps = stat_steps_;
    if (verify_passes) *verify_passes = stat_passes_;
  }
  // ---- token scores (anyref_set_token_scores / anyref_token_scores) ----
  // off (default): no launch, no allocation, the decode graphs of a handle that never heard of the switch.  The first
  // switch-on allocates sc_lp_ / sc_gap_ f32 [max_batch, llm_max_seq] -- indexed like hidden_all_, by the position of the row
  // that predicted the token -- the first token's dst map sc_dst_ i32 [max_batch], and their pinned host images
  void set_token_scores(bool on);
  // of the last generating call (decode_loop's copies, waited for here): row b's sc_n_[b] pairs in generation order
  void token_scores(int B, int n_cap, float* logprob, float* gap, int32_t* n);
  // every generating entry: the host state of the call before is gone
  void scores_clear(int B) { sc_n_.assign(scores_on_ && B > 0 ? B : 0, 0); }
  bool scores_on_ = false;
  float *sc_lp_ = nullptr, *sc_gap_ = nullptr;  // device
  int* sc_dst_ = nullptr;                       // device [max_batch]: b * llm_max_seq + slen[b] - 1 (the first token's rows)
  float* sc_host_ = nullptr;                    // pinned: logprob [max_batch, llm_max_seq] | gap [same]
  int* sc_stage_ = nullptr;                     // pinned image of sc_dst_
  void* sc_ev_ = nullptr;                       // hipEvent_t behind the last call's copies to sc_host_
  bool sc_pending_ = false;
  std::vector<int> sc_n_;                       // tokens per row of the last call; row b's pairs lead row b of sc_host_
  // ---- mask reports (anyref_set_mask_reports / anyref_set_packed_masks / anyref_mask_reports) ----
  // off (default): no launch, no allocation.  The first switch-on allocates rep_dev_ i32 [max_batch, max_seg, 8] and its
  // pinned host image.  The two sites that fill out_masks (early_seg_run, run_tail) launch the report behind their
  // postprocess; run_tail queues the copy to rep_host_ behind the last of them and mask_reports waits for rep_ev_
  void set_mask_reports(bool on, float offset);
  void set_packed_masks(uint32_t* dev, int64_t cap_words) {
    pack_armed_ = nullptr;
    pack_armed_cap_ = 0;
    if (!dev) return;
    if (!reports_on_) throw std::runtime_error("set_packed_masks: mask reports are off (anyref_set_mask_reports(h, 1, offset) first)");
    if (cap_words < 0) throw std::runtime_error("set_packed_masks: negative cap_words");
    pack_armed_ = dev;
    pack_armed_cap_ = cap_words;
  }
  void mask_reports(int B, int seg_cap, int32_t* n, int32_t* rec, int64_t* pack_offsets);
  // every mask-producing entry: the host state of the call before is gone, and the one-shot packed buffer is taken --
  // whatever happens below, nothing stays armed
  void reports_begin(int B) {
    const size_t rows = reports_on_ && B > 0 ? (size_t)(B < cfg.max_batch ? B : cfg.max_batch) : 0;
    rep_n_.assign(rows, 0);
    rep_off_.assign(rows, 0);
    pack_cur_ = reports_on_ ? pack_armed_ : nullptr;
    pack_cur_cap_ = pack_armed_cap_;
    pack_armed_ = nullptr;
    pack_armed_cap_ = 0;
  }
  static int64_t pack_words(int H, int W) { return (int64_t)H * (((int64_t)W + 31) / 32); }
  bool reports_on_ = false;
  float rep_offset_ = 1.f;
  int32_t* rep_dev_ = nullptr;    // device [max_batch, max_seg, 8]
  int32_t* rep_host_ = nullptr;   // pinned image
  void* rep_ev_ = nullptr;        // hipEvent_t behind the last call's copy to rep_host_
  bool rep_pending_ = false;
  std::vector<int> rep_n_;        // masks per row of the last call
  std::vector<int64_t> rep_off_;  // pack_offsets of the last call
  uint32_t *pack_armed_ = nullptr, *pack_cur_ = nullptr;  // for the next call / taken by the running one
  int64_t pack_armed_cap_ = 0, pack_cur_cap_ = 0;
  std::vector<std::vector<int64_t>> draft_ids_;  // per row; empty: nothing pending
  std::vector<int> stat_offered_, stat_accepted_;  // of the last generate
  int stat_steps_ = 0, stat_passes_ = 0;
  // the image session: row 0 of the KV cache / hidden states holds the prefix rows [0, sess_P_), image-embedding slot 0 the image
  bool sess_live_ = false;
  const char* sess_lost_by_ = nullptr;  // entry that ended the last session (for the error text)
  int sess_P_ = 0, sess_rows_ = 0;      // spliced prefix rows; cache rows [0, sess_rows_) hold them
  std::vector<int64_t> sess_prefix_;
  int32_t sess_rhw_[2] = {0, 0}, sess_ohw_[2] = {0, 0};
  // hipGraph replay of the greedy decode step (default on)
  void set_graphs(bool on) { use_graphs_ = on; }
  // workgroup cap of the encoder's GEMM / attention launches while it co-runs with the decode loop (0 = uncapped)
  // `steps`: the decode steps the capped encoder is spread over (its blocks are queued ceil(depth / steps) per step)
  void set_side_share(int wgs, int steps) {
    side_wgs_ = wgs < 0 ? 0 : wgs;
    if (steps > 0) side_steps_ = steps;
  }
  bool early_off_ = getenv("ANYREF_NO_EARLY_TAIL") != nullptr;
  Profiler prof;
  Stamper stamp;  // kernel-side timestamps of the decode GEMVs (bench.py's in-situ roofline)
  std::string err;
  int n_unknown = 0;

 protected:
  void* dalloc(size_t bytes);  // tracked hipMalloc (freed in the destructor)
  void dfree(void* p);
  const RawTensor& raw(const std::string& name) const;
  bool has_raw(const std::string& name) const { return raw_.count(name) != 0; }
  void drop_raw();

  anyref_config cfg;
  int device_;
  int64_t bytes_ = 0;
  std::unordered_map<void*, size_t> allocs_;
  std::map<std::string, RawTensor> raw_;
  bool finalized_ = false;
  // counts of the weight packing (launch_convert / launch_quant_fp8_rows): [0] inexact elements, [1] finite elements stored as
  // inf; a plain hipMalloc for the length of finalize (not in device_bytes), summed into inexact_ at its end
  unsigned long long* wcount_ = nullptr;
  unsigned long long* weight_counts();
  void close_weight_counts();
  int64_t inexact_ = 0;
  uint32_t resv_mask_ = 0;  // adapter_reserve
  std::vector<LoraTarget> lora_targets_;
  std::map<std::string, int64_t> upd_inexact_;  // inexact elements of the tensors anyref_update_weight can replace (reserving handles)
  int pairs_active_ = 0;
  double last_apply_ms_ = 0.0;
  bool overlap_ = true;
  bool use_graphs_ = true;
  bool reph_paths_ = false;   // set_rephrase_paths
  int early_masks_last_ = 0;  // early_masks_done
  int side_wgs_ = getenv("ANYREF_SIDE_WGS") ? atoi(getenv("ANYREF_SIDE_WGS")) : 128;
  int side_steps_ = getenv("ANYREF_SIDE_STEPS") ? atoi(getenv("ANYREF_SIDE_STEPS")) : 6;
  int side_head_ = getenv("ANYREF_SIDE_HEAD") ? atoi(getenv("ANYREF_SIDE_HEAD")) : 3;  // encoder blocks queued beside CLIP
  // 2 - 4 images per call (C3's per-GPU shape): the same feeding at a larger share over fewer steps (model.hip generate)
  int side_wgs_b_ = getenv("ANYREF_SIDE_WGS_B") ? atoi(getenv("ANYREF_SIDE_WGS_B")) : 160;
  int side_steps_b_ = getenv("ANYREF_SIDE_STEPS_B") ? atoi(getenv("ANYREF_SIDE_STEPS_B")) : 3;
  int side_cap_now_ = 0;  // the cap sam_feed applies during this call
};

std::unique_ptr<ModelBase> make_model(const anyref_config& cfg, int device);

}  // namespace anyref
