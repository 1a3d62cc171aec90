// generic_plan<NT>(): the MlpPlan of one width class of the generic-shape family (mlp_device_g.h), shared by the translation
// units nerf_mlp_generic_{a..d}.hip.  A unit defines NM_GENERIC_UNIT (its letter) before it includes this and then lists its
// classes in NM_PLANS_FN.  Each unit is compiled twice: as it is, and from nerf_mlp_generic_<unit>_long.hip with NM_GENERIC_LONG
// defined -- the instantiations whose encoding stages take two parts (16 -- 31 functions; enc_stages_g in mlp_device_g.h),
// registered as plans of variant G_LONG_VARIANT.
#pragma once
#include <vector>

#include "nm_internal.h"
#include "mlp_device_g.h"

#define NM_CAT3_(a, b, c) a##b##c
#define NM_CAT3(a, b, c) NM_CAT3_(a, b, c)
#ifdef NM_GENERIC_LONG
#define NM_PLANS_FN NM_CAT3(generic_plans_, NM_GENERIC_UNIT, _long)
constexpr bool kLong = true;
#else
#define NM_PLANS_FN NM_CAT3(generic_plans_, NM_GENERIC_UNIT, )
constexpr bool kLong = false;
#endif

namespace nm {

template <int NT>
static MlpPlan generic_plan() {
    static_assert(NT <= 24, "wider classes: nerf_mlp_generic_s.hip");
    constexpr int NW = 8, KCH = 8;            // two waves per SIMD; ring slots of at most 48 KiB
    constexpr int SLOT = KCH * ((NT + 3) / 4) * 1024;
    return MlpPlan{16 * NT, -1, -1, NW, KCH, kLong ? G_LONG_VARIANT : 0, 2 * SLOT, &mlp_kernel_g<NT, NW, KCH, false, kLong>, NW * 16, 1,
                   &mlp_kernel_g<NT, NW, KCH, false, kLong>, NT, &mlp_kernel_g<NT, NW, KCH, true, kLong>, &mlp_backward_kernel_g<NT, NW, KCH>};
}

}  // namespace nm
