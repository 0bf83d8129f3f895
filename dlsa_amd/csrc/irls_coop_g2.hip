// Instantiations of the cooperative pass for NT in {5, 6}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_g2, FamLogisticGaussian, EX_NONE, 5, 6)

}  // namespace dlsa
