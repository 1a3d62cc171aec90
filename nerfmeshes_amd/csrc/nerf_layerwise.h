// The layer-wise network path (nerf_layerwise.hip): entry points.  The handle-side description (LwNet) is the packer's: mlp_pack.h.
#pragma once
#include <vector>

#include "nm_internal.h"

namespace nm {

int layerwise_forward(nm_mlp* m, const MlpArgs& args, int density_only, hipStream_t stream);
int layerwise_forward_train(nm_mlp* m, const MlpArgs& args, const nm_mlp_tape* tape, hipStream_t stream);
int layerwise_backward(nm_mlp* m, int64_t n, const nm_mlp_tape* tape, const float* d_radiance, const float* d_grad_radiance,
                       const nm_mlp_deltas* deltas, hipStream_t stream);
void layerwise_destroy(nm_mlp* m);

}  // namespace nm
