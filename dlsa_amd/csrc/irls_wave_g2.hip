// Instantiations of the per-wave fp64 pass for NT in {7, 8}.
#include "irls_wave_impl.hpp"

namespace dlsa {

DLSA_WAVE_UNIT(launch_irls_wave_g2, FamLogisticGaussian, EX_NONE, 7, 8)

}  // namespace dlsa
