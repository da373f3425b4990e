// Split-pair flavour of the tiled MFMA GEMM with f16 terms (ANYREF_MODE_PARITY16_F16: f32 activations carried as two f16
// terms against exactly stored f16 weights, common.h `sp16h`); templates in gemm_impl.h, compiled beside gemm_sp16.hip.
#include "gemm_impl.h"

namespace anyref {

template void launch_gemm<sp16h>(const GemmArgs&, hipStream_t);

}  // namespace anyref
