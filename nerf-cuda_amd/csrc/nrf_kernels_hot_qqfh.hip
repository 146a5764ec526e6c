// nrf_kernels_hot_qqfh.hip -- persistent render kernel, hot instance under the static gather plan GATHER_QQFH:
// steps 0 and 1 from near quad copies, step 2 from far ones, step 3 hashed: base.json's grid at the default copy budget (the headline)
// (one static plan per translation unit, so that they compile side by side: nrf_render.h NRF_DEFINE_HOT_PLAN)
#include "nrf_render.h"

namespace nrf {

NRF_DEFINE_HOT_PLAN(qqfh, GATHER_QQFH)

}  // namespace nrf
