// Generic-shape instantiations of the fused MLP (mlp_device_g.h), part b: width classes NT = 8, 9, 10, 11, 12, 13 (hidden_size <= 16 NT).
// One translation unit per group of classes so that the build compiles them side by side (nerfmeshes_amd/build.py).
#define NM_GENERIC_UNIT b
#include "nerf_mlp_generic_plan.h"

namespace nm {

void NM_PLANS_FN(std::vector<MlpPlan>& out) {
    out.push_back(generic_plan<8>());
    out.push_back(generic_plan<9>());
    out.push_back(generic_plan<10>());
    out.push_back(generic_plan<11>());
    out.push_back(generic_plan<12>());
    out.push_back(generic_plan<13>());
}

}  // namespace nm
