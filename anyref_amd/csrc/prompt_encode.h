// SAM spatial prompts (anyref_prompt_reserve / anyref_mask_decode_prompted / anyref_refine_masks, anyref_op_prompt_tokens /
// anyref_op_mask_prompt_embed; prompt_encoder.py:78-186).  The rule is stated once, on the CPU, in
// anyref_amd/prompts.py; references and bounds of the two kernels: tests/prompt_ops_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace anyref {

// rows of the decoder's token matrix: n_out output tokens, P points, the pad point (P > 0 and no boxes), two box corners, text
int prompt_token_rows(int n_out, int P, bool boxes, bool text);
// tokens [n, rows, C] for all prompts in one launch.  points f32 [n,P,2] (x, y) in pixels of the S x S input frame, labels
// i32 [n,P] (1 / 0 / -1), boxes f32 [n,4] or null, text f32 [n,C] or null, gauss f32 [2, C/2], emb5 f32 [5,C]:
// point_embeddings 0 .. 3 and not_a_point_embed.  C % 8 == 0.  max_wg > 0 caps the grid (0: 2048 workgroups).
// Throws before anything is queued on a shape it does not take.
void launch_prompt_tokens(const float* out_tokens, int n_out, const float* points, const int32_t* labels, int P,
                          const float* boxes, const float* text, const float* gauss, const float* emb5, int n, int C, int S,
                          float* tokens, hipStream_t s, int max_wg = 0);
// mask_downscaling's weights as the checkpoint stores them: conv 1 [c1,1,2,2], LayerNorm2d over c1, conv 2 [c2,c1,2,2],
// LayerNorm2d over c2, conv 3 [C,c2,1,1]
struct MaskDownW {
  const float *w1 = nullptr, *b1 = nullptr, *g1 = nullptr, *be1 = nullptr, *w2 = nullptr, *b2 = nullptr, *g2 = nullptr,
              *be2 = nullptr, *w3 = nullptr, *b3 = nullptr;
  int c1 = 0, c2 = 0;
};
// keys [n, g*g, C] = image_emb [g*g, C] + mask_downscaling(mask [n, 4g, 4g]) as NHWC, for all prompts in one launch.
// c1 <= 8, c2 <= 32, C % 4 == 0, C <= 1024.  Throws before anything is queued on a shape it does not take.
void launch_mask_prompt_embed(const float* mask, const float* image_emb, const MaskDownW& W, int n, int g, int C, float* keys,
                              hipStream_t s, int max_wg = 0);

}  // namespace anyref
