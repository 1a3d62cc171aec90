// Generic-shape instantiations of the fused MLP (mlp_device_g.h), part d: width classes NT = 22, 24 (hidden_size <= 16 NT).
// One translation unit per group of classes so that the build compiles them side by side (nerfmeshes_amd/build.py).
#define NM_GENERIC_UNIT d
#include "nerf_mlp_generic_plan.h"

namespace nm {

void NM_PLANS_FN(std::vector<MlpPlan>& out) {
    out.push_back(generic_plan<22>());
    out.push_back(generic_plan<24>());
}

}  // namespace nm
