// Logistic instantiations of the per-wave fp64 pass with per-row prior weights
// (IRLS weight omega w) for NT in {7, 8}.
#include "irls_wave_impl.hpp"

namespace dlsa {

DLSA_WAVE_UNIT(launch_irls_wave_wgt_g2, FamLogistic, EX_WGT, 7, 8)

}  // namespace dlsa
