// Gram-mode kernels of the categorical pass (cat_gram_impl.hpp): the Poisson
// family, no row extras, d = s^2.
#include "cat_gram_impl.hpp"

namespace dlsa {

DLSA_CAT_GRAM_UNIT(FAMILY_POISSON, EX_NONE, CAT_ROW_GRAM_SCORE)

}  // namespace dlsa
