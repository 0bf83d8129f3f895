// Instantiations of the cooperative pass for NT in {8}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_g4, FamLogisticGaussian, EX_NONE, 8)

}  // namespace dlsa
