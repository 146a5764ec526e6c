// nrf_kernels_hot_dmhh.hip -- persistent render kernel, hot instance under the static gather plan GATHER_DMHH:
// step 0 dense, step 1 mixed, steps 2 and 3 hashed: base.json's grid without quad copies
// (one static plan per translation unit, so that they compile side by side: nrf_render.h NRF_DEFINE_HOT_PLAN)
#include "nrf_render.h"

namespace nrf {

NRF_DEFINE_HOT_PLAN(dmhh, GATHER_DMHH)

}  // namespace nrf
