// Poisson instantiations of the per-wave fp64 pass with per-row prior weights
// (IRLS weight omega w) for NT in {1, 2, 3, 4, 5, 6}.
#include "irls_wave_impl.hpp"

namespace dlsa {

DLSA_WAVE_UNIT(launch_irls_wave_pois_wgt_g1, FamPoisson, EX_WGT, 1, 2, 3, 4, 5, 6)

}  // namespace dlsa
