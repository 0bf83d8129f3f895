// Instantiations of the cooperative pass for NT in {1, 2, 3, 4}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_g1, FamLogisticGaussian, EX_NONE, 1, 2, 3, 4)

}  // namespace dlsa
