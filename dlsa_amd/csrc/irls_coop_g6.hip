// Instantiations of the cooperative pass for NT in {11, 12}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_g6, FamLogisticGaussian, EX_NONE, 11, 12)

}  // namespace dlsa
