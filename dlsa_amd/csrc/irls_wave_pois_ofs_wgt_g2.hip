// Poisson instantiations of the per-wave fp64 pass with a per-row offset and
// per-row prior weights (eta = x . theta + eta_offset, IRLS weight omega w) for NT in {7, 8}.
#include "irls_wave_impl.hpp"

namespace dlsa {

DLSA_WAVE_UNIT(launch_irls_wave_pois_ofs_wgt_g2, FamPoisson, EX_OFS | EX_WGT, 7, 8)

}  // namespace dlsa
