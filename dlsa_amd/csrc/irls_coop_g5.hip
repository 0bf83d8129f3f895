// Instantiations of the cooperative pass for NT in {9, 10}.
#include "irls_coop_impl.hpp"

namespace dlsa {

DLSA_COOP_UNIT(launch_irls_coop_g5, FamLogisticGaussian, EX_NONE, 9, 10)

}  // namespace dlsa
