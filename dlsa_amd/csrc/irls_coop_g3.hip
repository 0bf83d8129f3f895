// Instantiations of the cooperative pass for NT in {7}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_g3, FamLogisticGaussian, EX_NONE, 7)

}  // namespace dlsa
