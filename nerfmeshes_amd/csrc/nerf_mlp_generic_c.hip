// Generic-shape instantiations of the fused MLP (mlp_device_g.h), part c: width classes NT = 14, 15, 16, 18, 20 (hidden_size <= 16 NT).
// One translation unit per group of classes so that the build compiles them side by side (nerfmeshes_amd/build.py).
#define NM_GENERIC_UNIT c
#include "nerf_mlp_generic_plan.h"

namespace nm {

void NM_PLANS_FN(std::vector<MlpPlan>& out) {
    out.push_back(generic_plan<14>());
    out.push_back(generic_plan<15>());
    out.push_back(generic_plan<16>());
    out.push_back(generic_plan<18>());
    out.push_back(generic_plan<20>());
}

}  // namespace nm
