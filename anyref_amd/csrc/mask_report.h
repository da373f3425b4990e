// Mask reports (anyref_set_mask_reports / anyref_op_mask_report): one integer pass over f32 mask logits that
// are already in HBM.  The rule is stated once, on the CPU, in anyref_amd/maskreport.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// logits f32 [n, H, W] (contiguous; any 4-byte alignment), offset d >= 0.  Per mask m:
//   records i32 [n, 8] = {area #{x > 0}, area_hi #{x > d}, area_lo #{x > -d}, nonfinite #{NaN, +-inf},
//                         x0, y0, x1, y1: inclusive box of the bits x > 0, all 0 for an empty mask}
//   packed u32 [n, H, Wp], Wp = ceil(W / 32), or NULL: bit k of word w of row y = (x[y, 32 w + k] > 0), bits past W zero.
// NaN and -0.0 give bit 0.  The launcher clears the records itself, on `s` (the caller never does); sums and maxima by integer
// atomics, so a rerun is bit-identical.  Throws before anything is queued: H < 1, W < 1, H * W > INT32_MAX, n > 65535, an
// offset that is negative or not finite, null logits / records.  n <= 0: nothing happens.
void launch_mask_report(const float* logits, int n, int H, int W, float offset, int32_t* records, uint32_t* packed,
                        hipStream_t s);
