// nrf_kernels_hot_qqhh.hip -- persistent render kernel, hot instance under the static gather plan GATHER_QQHH:
// steps 0 and 1 from near quad copies, steps 2 and 3 hashed: copy budgets of about 100 to 256 MB
// (one static plan per translation unit, so that they compile side by side: nrf_render.h NRF_DEFINE_HOT_PLAN)
#include "nrf_render.h"

namespace nrf {

NRF_DEFINE_HOT_PLAN(qqhh, GATHER_QQHH)

}  // namespace nrf
