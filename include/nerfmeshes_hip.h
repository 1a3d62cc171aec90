/*
 * nerfmeshes_hip.h -- C ABI of the MI355X (gfx950) hot path of qway/nerfmeshes.
 *
 * The reference is pure Python/PyTorch and has no FFI of its own:
 * its boundary is the Python class surface (models.NeRFModel.forward/query/sample_points,
 * nerf.* helpers, mesh_nerf.extract_*).  This header is the C-ABI that sits *under* re-implemented
 * Python classes of the same names (package `nerfmeshes_amd`); every entry point cites the
 * reference code (file:line under /root/reference) whose arithmetic it replaces.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on failure; nm_last_error() gives the message
 *    (thread-local).  Nothing here ever falls back to a CPU path.
 *  - `d_` pointers are DEVICE pointers (HBM) owned by the caller; `h_` pointers are HOST pointers.
 *    The library allocates nothing on the hot calls; it owns only the packed weights in an
 *    nm_mlp handle.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous.
 *  - all floating point is IEEE fp32 (the reference never casts, train_nerf.py:38-41); index
 *    outputs are int32 (marching cubes faces) or int64 (BuFF voxel ids) as in the reference.
 */
#ifndef NERFMESHES_HIP_H
#define NERFMESHES_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): + nm_mc_count_slab / nm_mc_emit_slab, nm_np_chunk_count / nm_np_chunk_sums / nm_np_finish, use_viewdirs = 0
 * handles; nm_mc_workspace_bytes grew (per-cube decision table, cut-cube list).  Everything in version 1 is unchanged. */
/* 3 (round 4): nm_mlp_create accepts every FlexibleNeRFModel shape (generic kernel family; nm_mlp_kernel_variant >= 1000),
 * NM_KERNEL_GENERIC, training entry points for use_viewdirs = 0 and generic-shape handles (tape / delta fields those do not use
 * may be NULL), nm_mc_emit_slab accepts NULL outputs for an empty own share.  No signature changed; everything in version 2 is
 * unchanged. */
/* 4 (round 5): + nm_weight_grad_ex / nm_head_grad_ex (+ their workspace functions, nm_weight_grad_plan): weight gradients of
 * every layer shape, row stride and sample count; nm_weight_grad / nm_head_grad forward to them (their shape and n % 16
 * restrictions are gone), nm_encode_samples_strided writes whole rows for any stride.  No signature changed; everything in
 * version 3 is unchanged.  nm_mlp_create accepts hidden sizes above 512 and up to 32 encoding functions (layer-wise path). */
/* 5 (round 6): + nm_mlp_refresh_count / nm_mlp_weights_current (the stale-parameter guard), nm_mlp_tape.d_enc_xyz / d_enc_dir
 * (optional: the encoding rows written by the taping forward) + nm_mlp_tapes_encodings.  nm_mlp_tape grew at its end; a
 * zero-initialised struct of the old size keeps its meaning. */
/* 6 (round 6): + nm_mlp_backward_fused (+ _supported, _workspace_bytes, nm_mlp_param_grads): the 64-wide networks' whole
 * backward in one kernel; nm_mlp_tape.v_stride (0 = contiguous rows of d_v, as before); nm_mlp_backward_ex (flags),
 * nm_mlp_export_xyz_weight.  No signature changed. */
/* 6, later: + nm_mlp_sample_density, nm_mc_vertex_edges, nm_mc_edge_points, nm_mc_refine_vertices (mesh_nerf
 * --super-sampling).  Additions only: no struct and no signature changed, so the version stays 6. */
/* 6, later: + nm_mlp_density_grad (+ _workspace_bytes): d sigma / d x at arbitrary points (mesh_nerf --normals network).
 * Additions only. */
/* 6, later: + nm_surface_filter (+ _workspace_bytes), nm_surface_gather, nm_export_ply (mesh_surface_ray: the ray-marched
 * surface point cloud).  Additions only. */
/* 6, later: + nm_mesh_simplify_cluster (+ _workspace_bytes), nm_mesh_simplify_emit: mesh simplification by vertex clustering
 * (mesh_nerf --simplify-cell).  Additions only. */
/* 6, later: + nm_mesh_smooth_build (+ _workspace_bytes), nm_mesh_smooth_run, nm_mesh_vertex_normals: Taubin smoothing of the
 * mesh and the vertex normals of the result (mesh_nerf --smooth-iters).  Additions only. */
/* 6, later: + nm_mesh_rasterize (+ nm_mesh_raster_workspace_bytes), nm_mesh_interpolate: a deterministic software rasteriser of
 * the coloured mesh (mesh_render, mesh_nerf --render-views).  Additions only. */
/* 6, later: + nm_mesh_texture_layout, _samples, _fill, _uv, _lookup, nm_export_obj_textured: a texture atlas of per-face
 * charts baked from the network, and its fetch at the rasteriser's pixels (mesh_nerf --texture-res, mesh_render
 * --appearance).  Additions only. */
/* 6, later: + nm_mesh_visibility_views (+ _workspace_bytes), _select, _compact: the faces no camera of a set sees are dropped
 * (mesh_nerf --cull-hidden-views).  Additions only. */
/* 6, later: + nm_image_ssim: the structural similarity of two images, bit for bit a closed rule (eval_nerf --ssim, mesh_render
 * --ssim, mesh_nerf --render-ssim).  Additions only. */
/* 6, later: + nm_tsdf_integrate (+ nm_tsdf_workspace_bytes): rendered depth maps fused into a truncated signed distance field,
 * bit for bit a closed rule (mesh_nerf --geometry tsdf).  Additions only. */
/* 6, later: + nm_mesh_simplify_quadric_faces (+ nm_mesh_simplify_quadric_workspace_bytes), nm_mesh_simplify_emit_quadric:
 * quadric-optimal cluster vertices from exact integer quadrics (mesh_nerf --simplify-placement quadric).  Additions only. */
/* 6, later: + nm_mesh_simplify_adaptive_level (+ nm_mesh_simplify_adaptive_workspace_bytes), nm_mesh_simplify_adaptive_faces,
 * nm_mesh_simplify_adaptive_emit: error-bounded adaptive vertex clustering on nested grids (mesh_nerf --simplify-levels).
 * Additions only. */
#define NM_ABI_VERSION 6

const char* nm_last_error(void);
int nm_abi_version(void);
/* Number of visible HIP devices (<=0: none / error). */
int nm_device_count(void);

/* ------------------------------------------------------------------------------------------
 * FlexibleNeRFModel  (src/nerf/models.py:4-80; PositionalEncoding src/nerf/modules.py:8-37)
 * ------------------------------------------------------------------------------------------ */
typedef struct nm_mlp_desc {
    int32_t num_layers;           /* models.py:7   */
    int32_t hidden_size;          /* models.py:8   */
    int32_t skip_step;            /* models.py:9   */
    int32_t num_encoding_fn_xyz;  /* models.py:10  */
    int32_t num_encoding_fn_dir;  /* models.py:11  */
    int32_t include_input_xyz;    /* models.py:12  */
    int32_t include_input_dir;    /* models.py:13  */
    int32_t use_viewdirs;         /* models.py:16 -- 1: all shipped configs.  0 (models.py:77-79, trunk -> fc_out): fp32, inference
                                   * and training (the tape is the trunk's; see nm_mlp_tape) */
} nm_mlp_desc;

/* Host pointers to the tensors of FlexibleNeRFModel.state_dict(), torch.nn.Linear layout
 * (out_features, in_features) row-major fp32.  layers_xyz_* have num_layers-1 entries.
 * use_viewdirs = 0: the network ends in fc_out (4, hidden_size): pass its colour rows as fc_rgb_w = fc_out.weight (rows
 * 0..2, i.e. 3 x hidden_size contiguous floats) / fc_rgb_b = fc_out.bias, and its density row as fc_alpha_w =
 * fc_out.weight + 3 * hidden_size / fc_alpha_b = fc_out.bias + 3; layers_dir0_*, fc_feat_* and freq_dir are ignored. */
typedef struct nm_mlp_weights {
    const float* layer1_w;            const float* layer1_b;
    const float* const* layers_xyz_w; const float* const* layers_xyz_b;
    const float* layers_dir0_w;       const float* layers_dir0_b;
    const float* fc_alpha_w;          const float* fc_alpha_b;
    const float* fc_rgb_w;            const float* fc_rgb_b;
    const float* fc_feat_w;           const float* fc_feat_b;
    const float* freq_xyz;            /* encode_xyz.frequency_bands (num_encoding_fn_xyz) */
    const float* freq_dir;            /* encode_dir.frequency_bands (num_encoding_fn_dir) */
} nm_mlp_weights;

typedef struct nm_mlp nm_mlp;

/* Packs the weights into the MFMA operand stream and uploads them to `device`.
 * Every shape FlexibleNeRFModel's constructor accepts (models.py:5-58) is served: the shipped configs' shapes (hidden_size
 * 64 / 128 / 256, 6 or 10 xyz and 4 direction functions) by kernels tuned for exactly them, every other one -- any hidden_size
 * up to 512, 0..31 encoding functions per input (32 without the input itself), include_input_* on or off -- by the
 * generic-shape kernel family (padded to the next width class; nm_mlp_kernel_variant reports 1000 + class).  Beyond that -- a
 * hidden_size above 512 or an encoding of more than 48 MFMA k-steps -- the network is evaluated and trained LAYER BY LAYER on the
 * library's general MFMA GEMM (nm_mlp_kernel_variant 2000; the handle then owns a grow-only activation workspace that the
 * first call of a size allocates).  Only more than 32 encoding functions or a weight matrix of more than 2^24 elements fails,
 * with a message.  Every handle trains (generic-shape and layer-wise handles through the tape-row path: masks may be NULL,
 * nm_mlp_tape); NM_PREC_BF16X3 exists for the tuned (shipped) shapes only. */
int nm_mlp_create(const nm_mlp_desc* desc, const nm_mlp_weights* h_weights, int device, nm_mlp** out);

/* Arithmetic of the GEMMs.  NM_PREC_F32 (default, what nm_mlp_create builds): fp32 MFMA, the reference's fp32 arithmetic
 * up to summation order.  NM_PREC_BF16X3 (opt-in; the shipped widths 64 / 128 / 256 with 6 or 10 xyz and 4 direction functions): every product is emulated by six bf16 MFMA
 * products of a three-way split of both operands with fp32 accumulation -- fp32-class error (dropped terms <= 2^-24 of
 * a product) at ~2.3x the throughput, but not bit-comparable with the fp32 path; inference entry points only
 * (nm_mlp_forward_train / nm_mlp_backward refuse such a handle). */
enum { NM_PREC_F32 = 0, NM_PREC_BF16X3 = 1 };
/* OR into `precision` (with NM_PREC_F32): bind the handle to the generic-shape kernel family even where a tuned kernel exists
 * for the shape.  A cross-check, not a mode: the results are the tuned kernel's bit for bit. */
enum { NM_KERNEL_GENERIC = 0x100 };
int nm_mlp_create_ex(const nm_mlp_desc* desc, const nm_mlp_weights* host_weights, int device, int precision, nm_mlp** out);
int nm_mlp_precision(const nm_mlp* mlp);
void nm_mlp_destroy(nm_mlp* mlp);
/* Which kernel family the handle was bound to (0: a tuned kernel; 1000 + width class: the generic-shape family; 2000: the
 * layer-wise path) and its waves per workgroup. */
int nm_mlp_kernel_variant(const nm_mlp* mlp, int* waves_per_workgroup);
/* FLOP of one sample through the net (weights-only count). */
int64_t nm_mlp_flops_per_sample(const nm_mlp* mlp, int density_only);

/* Measurement hook (no reference counterpart): while enabled, every launch of the fused MLP kernel is
 * bracketed by hipEvents on its own stream.  nm_mlp_profile_read synchronises those events, returns
 * the number of launches, their summed duration and summed EXECUTED flops, and clears the list: total_flops is
 * the algorithmic count (samples x nm_mlp_flops_per_sample) minus, for the render calls' launches, what their
 * skipped tiles did not run -- skipped tiles x tile samples x (flops_per_sample(0) - flops_per_sample(1)); the tiles
 * are counted on the device (one counter per launch, allocated on every device by nm_mlp_profile_enable(1)) while
 * profiling is on.  A device has 2^20 counters: a skipping launch beyond that many since the last read evaluates
 * every tile (slower, and counted as such), so read at least that often.
 * Tiles that the render calls' ray termination did not evaluate at all (see nm_render_rays) are counted in a second word
 * per launch and leave total_flops with tile samples x flops_per_sample(0) each.  nm_mlp_profile_read_tiles is
 * nm_mlp_profile_read that also returns the two tile counts of the stretch (either pointer may be NULL). */
int nm_mlp_profile_enable(int on);
int nm_mlp_profile_read(int64_t* launches, double* total_ms, double* total_flops);
int nm_mlp_profile_read_tiles(int64_t* launches, double* total_ms, double* total_flops, int64_t* skipped_tiles,
                              int64_t* terminated_tiles);

/* BaseModel.sample_points / FlexibleNeRFModel.forward  (src/models/model_base.py:65-73,
 * src/nerf/models.py:60-80): d_points (n,3), d_dirs (n,3) -> d_radiance (n,4) = [sigmoid rgb, raw sigma]. */
int nm_mlp_sample_points(nm_mlp* mlp, const float* d_points, const float* d_dirs, int64_t n,
                         float* d_radiance, void* stream);

/* intervals_to_ray_points + model(...) of NeRFModel.forward  (src/models/model_helpers.py:32-35,
 * src/models/model_nerf.py:55-61,67-75): p = o + d * t (two roundings, as torch), view dir = d.
 * d_origins is (1,3) when origins_per_ray == 0, else (rays,3); d_dirs (rays,3); d_t (rays,samples);
 * d_radiance (rays,samples,4). */
int nm_mlp_eval_rays(nm_mlp* mlp, const float* d_origins, int origins_per_ray, const float* d_dirs,
                     const float* d_t, int64_t rays, int32_t samples, float* d_radiance, void* stream);

/* extract_radiance  (src/mesh_nerf.py:37-51): grid point (i,j,k) = (ax0[i], ax1[j], ax2[k]), flattened
 * with k fastest; the point itself is passed as view direction (mesh_nerf.py:45).  Evaluates points
 * [first, first+count) of the flattened grid.  If density_only != 0 writes raw sigma (count,) --
 * the colour branch is skipped -- else writes (count,4). */
int nm_mlp_grid_query(nm_mlp* mlp, const float* d_ax0, const float* d_ax1, const float* d_ax2,
                      int32_t n0, int32_t n1, int32_t n2, int64_t first, int64_t count,
                      int32_t density_only, float* d_out, void* stream);

/* Raw sigma of arbitrary points: d_points (n,3) -> d_sigma (n,), exactly what nm_mlp_grid_query(density_only = 1) writes
 * for the same fp32 triple (the point is its own view direction, as in the grid mode; sigma does not depend on it).  Every
 * fp32 kernel family; bf16x3 handles are rejected (geometry is fp32 by contract). */
int nm_mlp_sample_density(nm_mlp* mlp, const float* d_points, int64_t n, float* d_sigma, void* stream);

/* d sigma / d x of the raw sigma nm_mlp_sample_density returns, at arbitrary points: d_points (n,3) -> d_grad (n,3)
 * (nerf_input_grad.hip).  The gradient runs through fc_alpha (row 3 of fc_out without view directions), every layers_xyz[i] and
 * its ReLU (ReLU'(0) = 0, as torch), the skip layers' encoding columns, layer1 and the positional encoding
 * [x | sin(b_k x_c) | cos(b_k x_c)] (src/nerf/models.py:60-80, src/nerf/modules.py:26-34); sigma does not depend on the view
 * direction.  The matrix work is the training path's (nm_mlp_forward_train, nm_mlp_backward_ex seeded with d radiance =
 * (0, 0, 0, 1)) plus one fp32 MFMA kernel that contracts the deltas with the weights of the encoding columns and the
 * encoding's Jacobian, every weight out of the handle's packed image.  A point's result depends on that point and the packed
 * weights only -- not on n, its offset or the chunking (the entry chunks internally; a layer-wise handle always runs whole
 * fixed-size chunks).  Every fp32 handle; bf16x3 handles are rejected.  The workspace is bounded whatever n is: ask
 * nm_mlp_density_grad_workspace_bytes (0 for n = 0). */
int64_t nm_mlp_density_grad_workspace_bytes(const nm_mlp* mlp, int64_t n);
int nm_mlp_density_grad(nm_mlp* mlp, const float* d_points, int64_t n, void* d_workspace, int64_t workspace_bytes,
                        float* d_grad /* (n,3) */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ray-batch primitives
 * ------------------------------------------------------------------------------------------ */

/* get_ray_bundle  (src/nerf/nerf_helpers.py:226-277): h_c2w = 12 floats (rows of [:3,:4]);
 * writes unit directions for pixels [first, first+count) of the row-major (H,W) image into
 * d_dirs (count,3), and the origin c2w[:3,3] into h_origin[3]. */
int nm_ray_bundle(const float* h_c2w, int32_t height, int32_t width, float focal, int64_t first,
                  int64_t count, float* d_dirs, float* h_origin, void* stream);

/* A camera view: the inputs of get_ray_bundle (+ DataBundle.ndc, src/data/data_helpers.py:164-165).  Rays of a view
 * can be generated INSIDE the render kernels (nm_render_view below): ray r is pixel first+r of the row-major (H,W)
 * image; no origin / direction buffer is read or written, the host hands over 12 floats. */
typedef struct nm_view {
    float c2w[12];                 /* rows of tform_cam2world[:3,:4] */
    int32_t height, width;
    double focal;                  /* a python float in the reference: enters ndc_rays' constants in fp64 */
    int32_t use_ndc;               /* cfg.dataset.use_ndc: apply ndc_rays(H, W, focal, ndc_near, o, d) to every ray */
    double ndc_near;               /* 1.0 in the reference (data_helpers.py:165) */
} nm_view;

/* Materialise the rays of pixels [first, first+rays): d_origins (rays,3), d_dirs (rays,3) -- get_ray_bundle, then
 * ndc_rays when view->use_ndc (origins become per-ray). */
int nm_view_rays(const nm_view* view, int64_t first_pixel, int64_t rays, float* d_origins, float* d_dirs, void* stream);

/* ndc_rays  (src/nerf/nerf_helpers.py:280-307) on n rays: d_origins (1,3) or (n,3), d_dirs (n,3) ->
 * d_out_origins (n,3), d_out_dirs (n,3); op for op, python-float constants computed in fp64 and rounded once. */
int nm_ndc_rays(int32_t height, int32_t width, double focal, double near_, const float* d_origins, int origins_per_ray,
                const float* d_dirs, int64_t n, float* d_out_origins, float* d_out_dirs, void* stream);

/* PositionalEncoding.forward  (src/nerf/modules.py:26-34) on its own: d_x (n,dim) ->
 * d_out (n, [dim] + 2*dim*num_bands) = [x | sin(x_c * f_k), c-major | cos(...)]; h_bands = frequency_bands (host). */
int nm_positional_encoding(const float* d_x, int64_t n, int32_t dim, const float* h_bands, int32_t num_bands,
                           int32_t include_input, float* d_out, void* stream);

/* RaySampleInterval.forward, deterministic branch  (src/nerf/modules.py:157-186):
 * t[r][k] = near*(1-u[k]) + far*u[k]   (or the lindisp form).  d_u = linspace(0,1,samples) as the
 * module buffer holds it; d_near/d_far are (1,) when bounds_per_ray == 0 else (rays,). */
int nm_coarse_intervals(const float* d_u, const float* d_near, const float* d_far, int bounds_per_ray,
                        int lindisp, int64_t rays, int32_t samples, float* d_t, void* stream);

/* VolumeRenderer.forward + cumprod_exclusive  (src/nerf/modules.py:67-121,
 * src/nerf/nerf_helpers.py:199-223), noise = 0.  Any output pointer may be NULL.
 * d_radiance (rays,samples,4), d_t (rays,samples), d_dirs (rays,3). */
typedef struct nm_bundle_out {
    float* d_rgb_map;      /* (rays,3)       */
    float* d_depth_map;    /* (rays,)        */
    float* d_weights;      /* (rays,samples) */
    float* d_mask_weights; /* (rays,samples) */
    float* d_acc_map;      /* (rays,)        */
    float* d_disp_map;     /* (rays,)        */
} nm_bundle_out;
int nm_composite(const float* d_radiance, const float* d_t, const float* d_dirs, int64_t rays,
                 int32_t samples, float attenuation_threshold, int white_background, int training,
                 const nm_bundle_out* out, void* stream);

/* SamplePDF.forward / sample_pdf, deterministic u  (src/nerf/modules.py:197-248):
 * d_t (rays,coarse), d_weights (rays,coarse), d_u = linspace(0,1,fine) -> d_t_out (rays,coarse+fine) sorted. */
int nm_sample_pdf(const float* d_t, const float* d_weights, const float* d_u, int64_t rays,
                  int32_t coarse, int32_t fine, float* d_t_out, void* stream);

/* NeRFModel.forward  (src/models/model_nerf.py:37-78): the whole coarse -> resample -> fine chain in
 * one call, all intermediates in caller-provided workspace (nm_render_workspace_bytes).  `fine`
 * (and fine_out) may be NULL (models.use_fine False).
 * The radiance held in the workspace is internal: where no sample of a workgroup tile (128 samples: 8 adjacent rays x
 * 16 consecutive samples when the sample count is a multiple of 16, else 128 consecutive samples) has raw sigma > 0,
 * the fused 256-wide and 128-wide (10 xyz frequencies) fp32 kernels store {0, 0, 0, sigma} for the tile and do not evaluate its colour -- alpha
 * and weight of such samples are exactly 0, so every output map has the bits it has with the colours computed.
 * Ray termination: a call of at least two 8-ray blocks per resident workgroup, with sample counts that are multiples of 16,
 * does not evaluate a tile at all once the compositor's fp32 transmittance is provably 0 on all of its rays (a bound on
 * log2 of the product of the factors in front of it, kept per ray in the workspace, is below -160); the tile's radiance
 * is {0, 0, 0, 0}, its weights are the +0 they would have been.  The maps keep their bits for every finite sigma.  A
 * non-finite sigma BEHIND a ray that is already at transmittance 0 therefore no longer reaches the maps (it would have
 * made them NaN through 0 * alpha); in front of that point it propagates as before.  NM_RAY_TERMINATION=0 in the
 * environment switches ray termination off. */
typedef struct nm_render_cfg {
    int32_t num_coarse, num_fine;      /* cfg.nerf.train.num_coarse / num_fine (model_nerf.py:30-31) */
    int32_t lindisp;                   /* cfg.nerf.{train,validation}.lindisp */
    int32_t white_background;          /* cfg.dataset.white_background (model_base.py:31) */
    int32_t training;                  /* module.training: toggles depth_map[acc<1]=0 (modules.py:108) */
    float attenuation_threshold;       /* 1e-5 (model_base.py:32) */
} nm_render_cfg;
int64_t nm_render_workspace_bytes(int64_t rays, int32_t num_coarse, int32_t num_fine);
int nm_render_rays(nm_mlp* coarse, nm_mlp* fine, const nm_render_cfg* cfg, const float* d_origins,
                   int origins_per_ray, const float* d_dirs, const float* d_near, const float* d_far,
                   int bounds_per_ray, const float* d_u_coarse, const float* d_u_fine, int64_t rays,
                   void* d_workspace, const nm_bundle_out* coarse_out, const nm_bundle_out* fine_out,
                   void* stream);

/* The same for rays generated in the kernels from a camera pose (no ray buffers; saves the 24 B/ray read and the
 * host-side `batchify` H2D of src/nerf/nerf_helpers.py:128): pixels [first_pixel, first_pixel+rays) of `view`.
 * Bit-identical to nm_render_rays on the rays nm_view_rays materialises. */
int nm_render_view(nm_mlp* coarse, nm_mlp* fine, const nm_render_cfg* cfg, const nm_view* view, int64_t first_pixel,
                   int64_t rays, const float* d_near, const float* d_far, int bounds_per_ray, const float* d_u_coarse,
                   const float* d_u_fine, void* d_workspace, const nm_bundle_out* coarse_out,
                   const nm_bundle_out* fine_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training path: the arithmetic of NeRFModel.training_step
 * (src/models/model_nerf.py:88-151) -- forward with perturb / radiance noise / random resampling
 * (src/nerf/modules.py:82-91, 171-184, 224-228) and what loss.backward() computes for
 * FlexibleNeRFModel.forward (src/nerf/models.py:60-80) and VolumeRenderer.forward
 * (src/nerf/modules.py:67-121).  Random numbers are always the CALLER's device tensors
 * (torch.rand / torch.randn), so a run is reproducible from torch's generator state.
 * ------------------------------------------------------------------------------------------ */

/* Re-pack the network from DEVICE tensors (the live nn.Parameter storages, nn.Linear layout) after an
 * optimizer step: one gather kernel, asynchronous on `stream`, no host round trip.  Pointers as in
 * nm_mlp_weights; freq_xyz / freq_dir are ignored (buffers, fixed at nm_mlp_create). */
int nm_mlp_refresh(nm_mlp* mlp, const nm_mlp_weights* d_weights, void* stream);

/* Stale-parameter guard (ABI v5).  The reference has no packed copy to go stale: its forward reads the nn.Parameter
 * storages themselves (src/nerf/models.py:60-80), so ANY in-place edit -- an optimizer step (src/models/model_base.py:159-162),
 * `p.data.mul_()`, torch._foreach_* on `.data`, load_state_dict -- is visible to the next forward.  A handle holds a packed
 * image instead; these two calls let the host prove that the image still equals the live tensors:
 *   nm_mlp_refresh_count    how many times the image was (re)built since nm_mlp_create (create counts as 1).
 *   nm_mlp_weights_current  *differs = 0 when a checksum of the caller's live tensors (same pointers as nm_mlp_refresh),
 *                           taken through the gather's own index map, equals the checksum the last gather recorded of
 *                           what it packed; 1 otherwise.  One read-only kernel over the parameters (8x256: 2.4 MB) and an
 *                           8-byte read-back: it SYNCHRONISES `stream`.  64-bit sum of bits(value) * (2 * position + 1). */
int64_t nm_mlp_refresh_count(const nm_mlp* mlp);
int nm_mlp_weights_current(nm_mlp* mlp, const nm_mlp_weights* d_weights, void* stream, int32_t* differs);

/* Activations recorded by the training forward, n = rays * samples, tiles = ceil(n / 16), L = num_layers,
 * H = hidden_size.  Rows are the operands of the weight-gradient GEMMs (dW = delta^T @ rows).
 * A use_viewdirs = 0 handle tapes the trunk only: d_feat, d_v and d_mask_v are not touched and may be NULL (likewise the
 * d_feat / d_v of nm_mlp_deltas).  A generic-shape handle (nm_mlp_kernel_variant >= 1000) writes no masks -- its backward
 * kernel reads ReLU' off the activation rows, which nm_mlp_backward therefore needs (d_h, d_feat, d_v) --: d_mask_h and
 * d_mask_v may be NULL. */
typedef struct nm_mlp_tape {
    float* d_h;          /* (L, n, H): [0] layer1 output; [1+i] relu(layers_xyz[i](.))               */
    float* d_feat;       /* (n, H): relu(fc_feat(x))                                               */
    float* d_v;          /* (n, H/2): relu(layers_dir[0](cat(feat, view)))                         */
    uint64_t* d_mask_h;  /* (L, tiles, 64) ReLU masks of layers_xyz[0..L-2] and fc_feat, kernel-private layout */
    uint64_t* d_mask_v;  /* (tiles, 64)                                                            */
    /* ABI v5, optional (NULL: not written).  The PositionalEncoding rows (src/nerf/modules.py:26-34) of every sample point /
     * view direction, 64 floats per sample in the reference's column order [x | sin c-major | cos c-major] -- what the layer1 /
     * skip / view weight gradients contract with.  The taping kernel has these values in registers anyway; writing them here
     * saves the separate nm_encode_samples_strided pass of the backward.  Tuned-family handles only (nm_mlp_kernel_variant
     * < 1000, both encodings <= 64 wide); other handles leave the buffers untouched -- ask nm_mlp_tapes_encodings().
     * Columns beyond the encoding's width are not written. */
    float* d_enc_xyz;    /* (n, 64) or NULL                                                         */
    float* d_enc_dir;    /* (n, 64) or NULL                                                         */
    /* ABI v6: floats between consecutive rows of d_v; 0 = H/2 (contiguous rows).  Tuned-family handles only.  The 64-wide
     * networks' fused backward wants the 32-float rows of d_v INSIDE the direction-encoding rows -- d_v = d_enc_dir + 32,
     * v_stride = 64: an encoding row is 27 floats of its 64 -- so that one block of rows feeds both layers_dir[0]'s and fc_rgb's
     * weight gradients (nm_mlp_backward_fused). */
    int32_t v_stride;
    /* ABI v6: non-zero = do not write d_h[0] (layer1's output; the plane stays allocated, untouched).  For a backward that takes
     * layer1's and layers_xyz[0]'s gradients by linearity (nm_mlp_backward_ex + NM_BACKWARD_STOP_AT_XYZ0, nm_mlp_backward_fused):
     * neither reads it -- a tenth of the tape's bytes.  Tuned-family handles only. */
    int32_t skip_h0;
} nm_mlp_tape;
/* 1 when nm_mlp_forward_train on this handle fills d_enc_xyz / d_enc_dir (when given), 0 when the caller still needs
 * nm_encode_samples_strided. */
int nm_mlp_tapes_encodings(const nm_mlp* mlp);

/* dL/d(pre-activation) of every layer, written by nm_mlp_backward (same row layout as the tape). */
typedef struct nm_mlp_deltas {
    float* d_h;          /* (L, n, H): [0] at layer1's output; [1+i] at layers_xyz[i]'s pre-activation */
    float* d_feat;       /* (n, H) at fc_feat's pre-activation                                       */
    float* d_v;          /* (n, H/2) at layers_dir[0]'s pre-activation                               */
    float* d_last;       /* (n, 4): at fc_rgb's output (pre-sigmoid) x3, at fc_alpha's output        */
} nm_mlp_deltas;

/* FlexibleNeRFModel.forward over ray samples (as nm_mlp_eval_rays) that also records the tape. */
int nm_mlp_forward_train(nm_mlp* mlp, const float* d_origins, int origins_per_ray, const float* d_dirs,
                         const float* d_t, int64_t rays, int32_t samples, const nm_mlp_tape* tape,
                         float* d_radiance, void* stream);

/* Back-propagation through the network: d_grad_radiance (n,4) = dL/d(sigmoid(rgb), sigma) and the
 * forward's own d_radiance (n,4) -> deltas.  The weight gradients are products of those rows with the tape rows:
 * grad(layers_xyz[i].weight) = deltas.d_h[1+i]^T @ tape.d_h[i] (@ the encoding rows for the skip columns), grad(bias) =
 * column sums -- nm_weight_grad_ex / nm_head_grad_ex below compute them for every shape (nerfmeshes_amd/train_ops.py:
 * backward lists all of them; tests/cabi_smoke.c does one from plain C). */
int nm_mlp_backward(nm_mlp* mlp, int64_t n, const nm_mlp_tape* tape, const float* d_radiance,
                    const float* d_grad_radiance, const nm_mlp_deltas* deltas, void* stream);

/* ABI v6.  nm_mlp_backward with flags.  NM_BACKWARD_STOP_AT_XYZ0: the chain ends at layers_xyz[0]'s pre-activation -- d_h[1] is
 * the last delta written, d_h[0] is NOT produced, one of the L + 1 transposed layers is never applied (an eighth of the kernel at
 * 8 layers).  layer1 has no activation (src/nerf/models.py:62), so the delta at its output is linear in d_h[1] and its gradients
 * follow from sums over the samples:  grad(layer1.weight) = W0^T (d_h[1]^T @ encoding rows),  grad(layer1.bias) = W0^T (column
 * sums of d_h[1]),  W0 = layers_xyz[0].weight's hidden columns -- two calls of nm_weight_grad_ex, the second over H rows
 * (nerfmeshes_amd/train_ops.py: backward).  Tuned-family handles with num_layers >= 3 (nm_mlp_backward_stops_at_xyz0).
 * nm_mlp_export_xyz_weight writes layers_xyz[layer].weight, (H, H) or (H, H + dx) row-major, out of the handle's PACKED image --
 * the values the kernels of this forward / backward pair used, whatever happened to the live tensors since. */
#define NM_BACKWARD_STOP_AT_XYZ0 1
int nm_mlp_backward_stops_at_xyz0(const nm_mlp* mlp);
int nm_mlp_backward_ex(nm_mlp* mlp, int64_t n, const nm_mlp_tape* tape, const float* d_radiance,
                       const float* d_grad_radiance, const nm_mlp_deltas* deltas, int32_t flags, void* stream);
int nm_mlp_export_xyz_weight(nm_mlp* mlp, int32_t layer, float* d_out, void* stream);
/* The same identity gives layers_xyz[0]'s own weight gradient without its activation rows: tape.d_h[0] = layer1(enc) = W1 enc + b1, so
 *     grad(layers_xyz[0].weight) = d_h[1]^T @ tape.d_h[0] = [d_h[1]^T enc | sum d_h[1]] @ [W1 | b1]^T
 * -- the (H, dx + 1) matrix of sums the caller already has, times (dx + 1, H) = nm_mlp_export_layer1_transposed: rows 0 .. dx - 1
 * hold layer1.weight^T, row dx layer1.bias, again out of the packed image.  One of the L hidden x hidden weight-gradient products
 * over all samples becomes a product over dx + 1 rows. */
int nm_mlp_export_layer1_transposed(nm_mlp* mlp, float* d_out, void* stream);
/* Both products in one launch, the parameters read out of the packed image: d_sums (H, dx) with row stride ld = d_h[1]^T @ enc,
 * d_colsum (H) = the column sums of d_h[1]  ->  d_l1w (H, dx), d_l1b (H) = grad(layer1), d_x0w (H, H) = grad(layers_xyz[0].weight).
 * What nerfmeshes_amd/train_ops.py: backward calls behind the weight-gradient batch. */
int nm_mlp_linear_layer1_finish(nm_mlp* mlp, const float* d_sums, int32_t ld, const float* d_colsum, float* d_l1w, float* d_l1b,
                                float* d_x0w, void* stream);

/* ABI v6.  The whole back-propagation of a 64-wide network in ONE kernel (nerf_bwd_fused.hip): the delta chain of
 * nm_mlp_backward AND the weight / bias gradients of layer1, layers_xyz[*], fc_feat and layers_dir[0] -- what loss.backward()
 * leaves in the .grad of those parameters under NeRFModel.training_step (src/models/model_nerf.py:88-151, through
 * FlexibleNeRFModel.forward, src/nerf/models.py:60-80) -- without a delta row ever reaching HBM (the tape is read once, the
 * per-workgroup partials of all products are added up by one order-fixed reduction: deterministic).  The two 4-row heads
 * (fc_alpha, fc_rgb) are products of the same kernel: their delta d_last (n, 4) is staged in LDS next to the layers' deltas; it
 * is also written to d_last when that is not NULL (as nm_mlp_backward does).  The tape must hold the view layer's activation
 * rows inside the direction-encoding rows (nm_mlp_tape.v_stride: d_v = d_enc_dir + 32, v_stride = 64).
 * Served: tuned-family fp32 handles with hidden_size 64, use_viewdirs = 1, 2 <= num_layers <= 8, at most one skip layer, that
 * tape their encodings (nm_mlp_tapes_encodings; tape->d_enc_xyz / d_enc_dir must be given), n a multiple of 128 -- ask
 * nm_mlp_backward_fused_supported; everything else takes nm_mlp_backward + nm_weight_grad_batch.  Wider networks do not fit:
 * the accumulators of all products must stay resident per workgroup (128 wide: 630 KB, a CU's register file is 512 KB).
 * Gradient buffers are written in the parameters' own shapes: layer1 (H, dx), layers_xyz[i] (H, H) or (H, H + dx) for the
 * skip layer, fc_feat (H, H), layers_dir[0] (H / 2, H + dd), biases (rows,). */
#define NM_FUSED_MAX_LAYERS 8
typedef struct nm_mlp_param_grads {
    float* layer1_weight;
    float* layer1_bias;
    float* xyz_weight[NM_FUSED_MAX_LAYERS];   /* layers_xyz[0 .. num_layers - 2] */
    float* xyz_bias[NM_FUSED_MAX_LAYERS];
    float* feat_weight;
    float* feat_bias;
    float* dir_weight;
    float* dir_bias;
    float* alpha_weight;                      /* fc_alpha (1, H), (1,) */
    float* alpha_bias;
    float* rgb_weight;                        /* fc_rgb (3, H / 2), (3,) */
    float* rgb_bias;
} nm_mlp_param_grads;
int nm_mlp_backward_fused_supported(const nm_mlp* mlp, int64_t n);
int64_t nm_mlp_backward_fused_workspace_bytes(const nm_mlp* mlp);
int nm_mlp_backward_fused(nm_mlp* mlp, int64_t n, const nm_mlp_tape* tape, const float* d_radiance,
                          const float* d_grad_radiance, float* d_last, const nm_mlp_param_grads* grads, void* d_workspace,
                          void* stream);

/* PositionalEncoding.forward (src/nerf/modules.py:26-34) of the sample points / view directions as
 * rows in the reference's column order: d_enc_xyz (n, 3+6*Fx), d_enc_dir (n, 3+6*Fd); either may be NULL. */
int nm_encode_samples(nm_mlp* mlp, const float* d_origins, int origins_per_ray, const float* d_dirs,
                      const float* d_t, int64_t rays, int32_t samples, float* d_enc_xyz, float* d_enc_dir,
                      void* stream);

/* The same with explicit row strides (floats per row >= encoding width): whole rows are written, zero padding up to the
 * stride included (64-float rows are what the tuned nm_weight_grad kernel streams; any stride serves nm_weight_grad_ex, a
 * multiple of 4 floats gives it 16-byte DMA pieces).  d_enc_dir must be NULL for use_viewdirs = 0 handles. */
int nm_encode_samples_strided(nm_mlp* mlp, const float* d_origins, int origins_per_ray, const float* d_dirs,
                              const float* d_t, int64_t rays, int32_t samples, float* d_enc_xyz, int32_t stride_xyz,
                              float* d_enc_dir, int32_t stride_dir, void* stream);

/* Weight and bias gradient of one Linear from tape rows -- what autograd's addmm backward computes for every layer of
 * FlexibleNeRFModel (src/nerf/models.py:60-80):  d_dw[o * dw_ld + dw_col0 + c] = sum_n delta[n][o] * act[n][c] for
 * c < in_features, and (d_dbias != NULL) d_dbias[o] = sum_n delta[n][o].  d_delta (n, out_features) and d_act
 * (n, act_stride) are row-major; n must be a multiple of 16, out_features and act_stride multiples of 64 (activation rows
 * zero-padded beyond in_features).  Supported (out_features, act_stride): (256,256) (256,64) (128,256) (128,128)
 * (128,64) (64,128).  fp32 MFMA, split over the samples across one workgroup per CU, order-fixed reduction of the
 * per-workgroup partials (deterministic; no atomics).  Workspace: nm_weight_grad_workspace_bytes. */
int nm_mlp_num_cus(const nm_mlp* mlp);
int64_t nm_weight_grad_workspace_bytes(int32_t out_features, int32_t act_stride, int32_t num_cus);
int nm_weight_grad(int num_cus, const float* d_delta, int32_t out_features, const float* d_act, int32_t act_stride,
                   int32_t in_features, int64_t n, void* d_workspace, float* d_dw, int32_t dw_ld, int32_t dw_col0,
                   float* d_dbias, void* stream);

/* The 4-row head gradients (fc_alpha: row 3 of dlast^T h[L-1]; fc_rgb: rows 0..2 of dlast^T v -- models.py:74-78's two
 * Linear layers share the delta dlast (n, 4)): d_dw[r * in_features + k] = sum_n dlast[n][r] * act[n][k], d_dbias[r] =
 * sum_n dlast[n][r] (may be NULL).  in_features 64, 128 or 256.  HBM-bound VALU kernel + the order-fixed partial reduction. */
int64_t nm_head_grad_workspace_bytes(int32_t in_features);
int nm_head_grad(const float* d_dlast, const float* d_act, int32_t in_features, int64_t n, void* d_workspace,
                 float* d_dw, float* d_dbias, void* stream);

/* The general forms (ABI v4): ANY out_features / in_features (what FlexibleNeRFModel's constructor accepts,
 * src/nerf/models.py:5-58), ANY row strides (floats; >= the feature counts), ANY n >= 1 -- no padding of rows or columns is
 * required or written: columns beyond a width only reach dW entries nobody reads, rows beyond n are read as zeros through
 * the buffer descriptor's exact extent.  Same dataflow as nm_weight_grad (fp32 MFMA, operands DMA'd HBM -> LDS as they lie
 * in memory, one workgroup per CU, order-fixed reduction: deterministic), its geometry -- tiles per wave, how the 8 waves of
 * a workgroup split the output block and the samples, how many blocks a wide output is cut into -- picked from the shape
 * alone by a planner (nm_weight_grad_plan reports it: [nba, nbb, wa, wb, wk, ta, tb, rows per chunk]).  nm_weight_grad and
 * nm_head_grad forward here for every shape / sample count their tuned kernels do not serve, so no weight gradient of any
 * network the library accepts is a library GEMM. */
int64_t nm_weight_grad_workspace_bytes_ex(int32_t out_features, int32_t delta_stride, int32_t in_features, int32_t act_stride,
                                          int32_t num_cus);
int nm_weight_grad_ex(int num_cus, const float* d_delta, int32_t out_features, int32_t delta_stride, const float* d_act,
                      int32_t in_features, int32_t act_stride, int64_t n, void* d_workspace, float* d_dw, int32_t dw_ld,
                      int32_t dw_col0, float* d_dbias, void* stream);
int nm_weight_grad_plan(int32_t out_features, int32_t delta_stride, int32_t in_features, int32_t act_stride,
                        int32_t aligned16, int32_t num_cus, int32_t* plan8);

/* Several products of ONE shape, stride pair and row count in one launch + one reduction -- the same-shape layers of a network
 * (models.py:63-70: layers_xyz[*] and fc_feat are all hidden x hidden).  A job gets 1 / jobs of the CUs and jobs times the
 * samples per workgroup: the same matrix work, but jobs times fewer per-workgroup partials to write and to reduce (eight
 * 256 x 256 layers: 64 MB instead of 512 MB) and 2 launches instead of 2 * jobs.  At most 16 jobs; the workspace of ONE
 * product (nm_weight_grad_workspace_bytes_ex) suffices: it holds max(1, num_cus / output blocks) sample parts, and a batch
 * that needs more (layers wider than ~1000: the output is cut into many blocks) is issued in sub-batches that re-use it, one
 * after the other on the stream.  Deterministic; the summation grouping differs from jobs separate
 * calls (fewer, longer sample parts). */
typedef struct nm_weight_grad_job {
    const float* d_delta;    /* (n, out_features), row stride delta_stride */
    const float* d_act;      /* (n, in_features), row stride act_stride    */
    float* d_dw;             /* d_dw[o * dw_ld + dw_col0 + c]               */
    int32_t dw_ld, dw_col0;
    float* d_dbias;          /* (out_features,) or NULL                     */
} nm_weight_grad_job;
int nm_weight_grad_batch(int num_cus, int32_t jobs, const nm_weight_grad_job* job, int32_t out_features, int32_t delta_stride,
                         int32_t in_features, int32_t act_stride, int64_t n, void* d_workspace, void* stream);
int64_t nm_head_grad_workspace_bytes_ex(int32_t in_features);
int nm_head_grad_ex(const float* d_dlast, const float* d_act, int32_t in_features, int32_t act_stride, int64_t n,
                    void* d_workspace, float* d_dw, float* d_dbias, void* stream);

/* RaySampleInterval.forward's stratified jitter (src/nerf/modules.py:171-184): d_rand (rays,samples) in [0,1). */
int nm_perturb_intervals(const float* d_t, const float* d_rand, int64_t rays, int32_t samples, float* d_t_out,
                         void* stream);

/* VolumeRenderer.forward in training mode: sigma + d_noise (rays,samples; NULL = no noise) before the
 * ReLU (src/nerf/modules.py:82-93), depth_map not zeroed (modules.py:108). */
int nm_composite_train(const float* d_radiance, const float* d_t, const float* d_dirs, const float* d_noise,
                       int64_t rays, int32_t samples, float attenuation_threshold, int white_background,
                       const nm_bundle_out* out, void* stream);

/* Upstream gradients of the bundle (any may be NULL = zero); disp_map / mask_weights are not differentiable here. */
typedef struct nm_bundle_grads {
    const float* d_rgb_map;   /* (rays,3)       */
    const float* d_acc_map;   /* (rays,)        */
    const float* d_depth_map; /* (rays,)        */
    const float* d_weights;   /* (rays,samples) */
} nm_bundle_grads;
int nm_composite_backward(const float* d_radiance, const float* d_t, const float* d_dirs, const float* d_noise,
                          int64_t rays, int32_t samples, int white_background, const nm_bundle_grads* grads,
                          float* d_grad_radiance, void* stream);

/* SamplePDF.forward with per-ray random u (src/nerf/modules.py:224-228): d_u (rays,fine). */
int nm_sample_pdf_rand(const float* d_t, const float* d_weights, const float* d_u, int64_t rays, int32_t coarse,
                       int32_t fine, float* d_t_out, void* stream);

/* numpy's fp32 statistics of a device array, bit for bit (src/mesh_nerf.py:56-65 picks the marching-cubes level from
 * density.min() / .max() / .std() / .mean() of a numpy fp32 array; the mesh topology depends on that level):
 * h_out6 = [sum, mean, var, std, min, max] as numpy computes them (8192-element buffer chunks accumulated sequentially,
 * pairwise summation with 8 interleaved accumulators inside a chunk, fp32 throughout).  Synchronises the stream. */
int64_t nm_np_stats_workspace_bytes(int64_t n);
int nm_np_stats(const float* d_x, int64_t n, void* d_workspace, float* h_out6, void* stream);

/* The same statistics when the array is spread over several devices (multi-GPU mesh extraction: every rank holds an axis-0
 * slab of the density grid and the adaptive iso level of src/mesh_nerf.py:56-65 still has to be numpy's, bit for bit).
 * numpy sums 8192-element chunks pairwise and accumulates the chunk sums sequentially, so the two stages separate:
 *   nm_np_chunk_sums  a rank holding the global elements [first, first + count) sums the chunks [chunk_lo, chunk_hi) of
 *                     the GLOBAL array of n elements (all of their elements must be held).  First pass
 *                     (squared_deviation = 0): sums + per-chunk min / max (NaN-propagating, as numpy); second pass
 *                     (squared_deviation = 1, with the mean of the first): sums of (x - mean)^2; d_csum then needs room
 *                     for chunk_hi - chunk_lo + 1 floats.
 *   nm_np_finish      the chunk sums of all ranks concatenated in chunk order -> [sum, mean, -, -, min, max] (first pass)
 *                     or [-, -, var, std, -, -] (second pass) in d_out6 / h_out6; synchronises the stream. */
int64_t nm_np_chunk_count(int64_t n);
int nm_np_chunk_sums(const float* d_x, int64_t first, int64_t count, int64_t n, int64_t chunk_lo, int64_t chunk_hi,
                     int32_t squared_deviation, float mean, float* d_csum, float* d_cmin, float* d_cmax, void* stream);
int nm_np_finish(const float* d_csum, const float* d_cmin, const float* d_cmax, int64_t chunks, int64_t n,
                 int32_t squared_deviation, float* d_out6, float* h_out6, void* stream);

/* ------------------------------------------------------------------------------------------
 * BuFF voxel-tree sampler: TreeSampling.batch_ray_voxel_intersect, deterministic branch
 * (src/nerf/tree.py:215-343).  d_voxels (nvox,2,3) min/max corners; d_origins (1,3) or (rays,3);
 * d_u = linspace(0,1,samples).  Outputs: d_z (rays,samples) sorted depths, d_idx (rays,samples) int64
 * voxel ids, d_mask (rays,) uint8 "ray crosses at least one voxel inside [near, far]".
 * Synchronises the stream (overflow check: a ray may cross at most 512 voxels).
 * ------------------------------------------------------------------------------------------ */
int nm_buff_intersect(const float* d_voxels, int32_t nvox, const float* d_origins, int origins_per_ray,
                      const float* d_dirs, float near_, float far_, const float* d_u, int64_t rays,
                      int32_t samples, float* d_z, int64_t* d_idx, uint8_t* d_mask, void* stream);

/* The same with an explicit tie order for the three sorts of the reference (src/nerf/tree.py:300,306,335 call
 * torch.sort with its UNSTABLE default):
 *   NM_TIES_STABLE     ties keep voxel-index / sample order: every id is the voxel its sample lies in (default);
 *   NM_TIES_REFERENCE  ties ordered as torch's CPU sort orders them (libstdc++ std::sort over (key, index) pairs,
 *                      restated in the kernel): d_idx equals the reference's output bit for bit, including its
 *                      scrambled attribution of samples to the crossed voxels.  The three introsorts are evaluated
 *                      wave-parallel and exactly (one wavefront per ray; 7.6 ms vs 1.3 ms per 65 536 rays x 192
 *                      samples on 1728 voxels); nvox <= 8192, at most 512 crossed voxels per ray (error 4 beyond).
 *                      Synchronises the stream.  d_z and d_mask are identical in both. */
enum { NM_TIES_STABLE = 0, NM_TIES_REFERENCE = 1 };
int nm_buff_intersect_ex(const float* d_voxels, int32_t nvox, const float* d_origins, int origins_per_ray,
                         const float* d_dirs, float near_, float far_, const float* d_u, int64_t rays,
                         int32_t samples, int32_t tie_order, float* d_z, int64_t* d_idx, uint8_t* d_mask, void* stream);

/* The `tree.use_random_sampling` branch of the same function (src/nerf/tree.py:280-297, :337-341) as a function of the
 * draws: d_u_pick (rays,samples) DOUBLE = the uniforms torch.multinomial(weights, samples, replacement=True) consumes
 * (weights 1 for crossed voxels, 1e-12 otherwise: an inverse-CDF pick among the crossed voxels in index order, decided
 * in fp32 as ATen does), d_u_pos (rays,samples) float = torch.rand_like(values_min) (the position inside the drawn
 * voxel's [t_enter, t_exit]).  Outputs as above; given the reference's own draws they equal its output bit for bit on
 * every ray that crosses a voxel (one exception: a draw u below the 1e-12 weights' own share, u < 1.7e-9, selects a
 * NON-crossed voxel in the reference and the first crossed one here).  Rows of rays that cross nothing are zero-filled (d_mask 0): the reference samples
 * arbitrary voxels there, its caller overwrites those depths (src/models/model_buff.py:53) and nothing reads the ids.
 * Synchronises the stream (overflow check). */
int nm_buff_intersect_random(const float* d_voxels, int32_t nvox, const float* d_origins, int origins_per_ray,
                             const float* d_dirs, float near_, float far_, const double* d_u_pick,
                             const float* d_u_pos, int64_t rays, int32_t samples, float* d_z, int64_t* d_idx,
                             uint8_t* d_mask, void* stream);

/* TreeSampling.ray_batch_integration (src/nerf/tree.py:177-206), training-time tree maintenance: the samples of
 * the rays that hit the tree -- d_idx / d_weights / d_mask_weights, `count` elements each (= indices[mask],
 * weights[mask], mask_weights[mask] flattened) -- update the running voxel weights d_memm (nvox,) in place:
 * memm[v] += (sum_w[v] / sum_mask[v] - memm[v]) / counter wherever sum_mask[v] > 0.  `counter` is the tree's
 * 1-based integration counter (the caller increments it).  Workspace: nm_tree_workspace_bytes(nvox). */
int64_t nm_tree_workspace_bytes(int32_t nvox);
int nm_tree_integrate(const int64_t* d_idx, const float* d_weights, const float* d_mask_weights, int64_t count,
                      int32_t nvox, int32_t counter, float* d_memm, void* d_workspace, void* stream);


/* ------------------------------------------------------------------------------------------
 * Marching cubes: skimage.measure.marching_cubes(volume, level) as called at src/mesh_nerf.py:79
 * (third-party scikit-image 0.17.2, Lewiner MC33, defaults: step_size=1, gradient_direction='descent',
 * allow_degenerate=True, no mask).  Output-identical: vertices (V,3) fp32 in (axis0,axis1,axis2) order,
 * faces (F,3) int32 (same vertex numbering and triangle order), normals (V,3), values (V,).
 * Two-phase because V and F are data dependent:
 *   nm_mc_count  classifies every cube and returns V and F (synchronises the stream);
 *   nm_mc_emit   writes the four arrays (caller-allocated from those counts).
 * d_workspace (nm_mc_workspace_bytes) must be kept between the two calls; d_vertex_scratch
 * (nm_mc_vertex_scratch_bytes(V, F)) is only used by nm_mc_emit.  V == 0 is skimage's
 * RuntimeError('No surface found at the given iso value.'); the level-in-range ValueError is the
 * host wrapper's check, as in skimage's Python wrapper.
 * ------------------------------------------------------------------------------------------ */
int64_t nm_mc_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int64_t nm_mc_vertex_scratch_bytes(int64_t vertices, int64_t faces);
int nm_mc_count(const float* d_volume, int32_t n0, int32_t n1, int32_t n2, double iso, void* d_workspace,
                int64_t* h_vertices, int64_t* h_faces, void* stream);
int nm_mc_emit(const float* d_volume, int32_t n0, int32_t n1, int32_t n2, double iso, void* d_workspace,
               void* d_vertex_scratch, int64_t vertices, int64_t faces, float* d_verts, int32_t* d_faces,
               float* d_normals, float* d_values, void* stream);

/* Per-slab marching cubes (multi-GPU mesh extraction: every rank meshes its own axis-0 slab, only the triangles are
 * gathered -- SURVEY.md 8(e), BASELINE.json north_star "all-gather of emitted triangles"; replaces the all-gather of the
 * density grid in front of skimage.measure.marching_cubes, src/mesh_nerf.py:79).
 * d_volume holds the global planes [z_global, z_global + n0) of the grid.  Its first cube layer is a ghost of the slab below
 * when ghost_below = 1 (classified and numbered -- the faces of the layer above reference the vertices it creates -- but
 * nothing of it is emitted), its last one a ghost of the slab above when ghost_above = 1 (never classified; its voxels are
 * read when the normals of this slab's top vertices replay the cubes around them).  Vertex ownership follows the GLOBAL
 * plane index, so a slab creates exactly the vertices the single-volume run creates in its layers, in the same order.
 *   nm_mc_count_slab  -> V, F including the ghost layer's, and the ghost layer's own V_g, F_g;
 *   nm_mc_emit_slab   writes the slab's V - V_g vertices / normals / values and F - F_g faces; face entries are
 *                     local id + index_base: with index_base = (vertices of all lower slabs) - V_g the concatenation of
 *                     the ranks' arrays in rank order IS the single-volume mesh, bit for bit, vertex numbering included.
 * With z_global = ghost_below = ghost_above = 0 these are nm_mc_count / nm_mc_emit. */
int nm_mc_count_slab(const float* d_volume, int32_t n0, int32_t n1, int32_t n2, double iso, int32_t z_global,
                     int32_t ghost_below, int32_t ghost_above, void* d_workspace, int64_t* h_vertices, int64_t* h_faces,
                     int64_t* h_ghost_vertices, int64_t* h_ghost_faces, void* stream);
int nm_mc_emit_slab(const float* d_volume, int32_t n0, int32_t n1, int32_t n2, double iso, int32_t z_global,
                    int32_t ghost_below, int32_t ghost_above, void* d_workspace, void* d_vertex_scratch, int64_t vertices,
                    int64_t faces, int64_t ghost_vertices, int64_t ghost_faces, int64_t index_base, float* d_verts,
                    int32_t* d_faces, float* d_normals, float* d_values, void* stream);

/* Super-sampled marching cubes (mesh_nerf --super-sampling ss; the reference's src/mesh_nerf.py:95-128 is dead code, the
 * semantics are DESIGN.md's): the plain mesh's topology, normals and values, with every EDGE vertex moved along its own
 * edge to the first sign change among the ss interior samples of that edge.  Keys name a vertex's edge:
 *   key = global linear index of the lower-corner voxel * 4 + axis, axis in ARRAY order (0 = axis 0, the slowest, and
 *   the first vertex column); axis 3 = the centre vertex of an MC33 tiling (the key's voxel is then its cube's origin).
 *
 * nm_mc_vertex_edges: after nm_mc_emit / nm_mc_emit_slab, with the same dims, z_global and d_vertex_scratch, and the
 *   `vertices` / `ghost_vertices` that call was given (0 for nm_mc_emit; they fix the scratch's layout), writes the key of
 *   each of the call's own vertex rows: d_keys (vertices - ghost_vertices,), row r = the emit's row r.  The scratch keeps
 *   these values until it is reused.
 * nm_mc_edge_points: d_keys (V,) of a global (n0,n1,n2) grid -> d_points (V,ss,3): interior sample s = 1..ss of the edge of
 *   the voxel (i0,i1,i2) along array axis a is the point whose coordinate a is fine_a[i_a*(ss+1) + s], the others base.
 *   d_base_a has n_a entries, d_fine_a (n_a-1)*(ss+1)+1 (linspace(-limit, limit, .) in fp32).  Centre rows get an in-range
 *   point, which refinement ignores.  ss = 0 writes nothing (d_points and the fine axes may then be NULL).
 * nm_mc_refine_vertices: d_volume holds the global planes [z_global, z_global + n0) of the grid (a slab, or the whole grid
 *   with z_global = 0); d_fine_sigma (V,ss) the densities of those points.  For each edge row: d_0 = v_lo - iso,
 *   d_1..d_ss = fine - iso, d_ss+1 = v_hi - iso (fp64); m = the first index with (d_m > 0) != (d_m+1 > 0);
 *   w1 = 1/(eps + |d_m|), w2 = 1/(eps + |d_m+1|) (eps = skimage's 2^-52); column a of d_verts (V,3) becomes
 *   i_a + (m + w2/(w1+w2)) / (ss+1), rounded to fp32 once.  Centre rows are untouched.  With ss = 0 (d_fine_sigma = NULL)
 *   this is nm_mc_emit's own interpolation, bit for bit.
 * ss is in [0, 64]; every fine axis must fit int32.  One thread per vertex, no workspace, no host synchronisation. */
int nm_mc_vertex_edges(const void* d_vertex_scratch, int64_t vertices, int64_t ghost_vertices, int32_t n0, int32_t n1,
                       int32_t n2, int32_t z_global, int64_t* d_keys, void* stream);
int nm_mc_edge_points(const int64_t* d_keys, int64_t V, int32_t n0, int32_t n1, int32_t n2, int32_t ss,
                      const float* d_base0, const float* d_base1, const float* d_base2, const float* d_fine0,
                      const float* d_fine1, const float* d_fine2, float* d_points, void* stream);
int nm_mc_refine_vertices(const float* d_volume, int32_t n0, int32_t n1, int32_t n2, int32_t z_global, double iso,
                          const int64_t* d_keys, int64_t V, int32_t ss, const float* d_fine_sigma, float* d_verts,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh export: export_obj (src/nerf/nerf_helpers.py:86-111), byte-identical text.  HOST arrays:
 * vertices (V,3), diffuse (C,3) with C <= V allowed (colours only while they last), normals (N,3),
 * triangles (F,3) int32, 0-based.  Numbers are printed as Python prints repr(float(x)).  Multi-threaded.
 * ------------------------------------------------------------------------------------------ */
int nm_export_obj(const float* h_vertices, int64_t num_vertices, const float* h_diffuse, int64_t num_diffuse,
                  const float* h_normals, int64_t num_normals, const int32_t* h_triangles, int64_t num_triangles,
                  const char* path);

/* ------------------------------------------------------------------------------------------
 * Surface point cloud (mesh_surface_ray; the reference's src/mesh_surface_ray.py:115-141 on the device; DESIGN.md,
 * "Surface point cloud").  One image of height x width rays, row-major; all buffers on the device, fp32:
 * d_origins (1,3) shared or, with per_ray_o != 0, (height*width,3); d_dirs (height*width,3); d_depth (height*width);
 * d_opacity (height*width) or NULL.
 *
 * nm_surface_filter: depth used z = d_depth when d_opacity is NULL, else (opacity >= (float)min_opacity ? depth : 0).
 *   Surface point p = o + d * z (two roundings).  votes(row, col) = number of offsets (a, b) in [-step, step]^2 whose
 *   neighbour q at (clamp(row + a, 0, height-1), clamp(col + b, 0, width-1)) -- the centre and clamped duplicates count --
 *   has ((qx-px)^2 + (qy-py)^2) + (qz-pz)^2 < (float)dist_threshold (a SQUARED distance).
 *   keep = votes >= min_votes && z > 0; NaN never votes and is never kept.  Outputs, each optional (NULL): d_votes
 *   (height*width) int32, d_keep (height*width) bytes 0 / 1, d_count (1) int64 = pixels kept.  d_workspace
 *   (nm_surface_filter_workspace_bytes(height, width) bytes, 16-byte aligned) receives the keep bits and their prefix sums
 *   for nm_surface_gather and must stay untouched until then.
 * nm_surface_gather: with the same inputs and that workspace, writes the kept pixels IN ROW-MAJOR PIXEL ORDER to rows
 *   row_offset, row_offset + 1, ... of the output arrays of `capacity` rows (rows beyond capacity are dropped, never
 *   written): d_points (.,3) = p, d_normals (.,3) = -d, d_colors (.,3) = d_rgb's row, d_colors_u8 (.,3) bytes =
 *   trunc(clamp(rgb * 255, 0, 255)), NaN -> 0.  Each output may be NULL; d_rgb (height*width,3) may be NULL when both colour
 *   outputs are.
 * step is in [0, 8], height * width <= 2^30.  No allocation and no host synchronisation: both entries can be captured
 * into a HIP graph.  Argument errors return 2 before any HIP call.
 * ------------------------------------------------------------------------------------------ */
int64_t nm_surface_filter_workspace_bytes(int32_t height, int32_t width);
int nm_surface_filter(const float* d_origins, int per_ray_o, const float* d_dirs, const float* d_depth,
                      const float* d_opacity, double min_opacity, int32_t height, int32_t width, int32_t step,
                      double dist_threshold, int32_t min_votes, int32_t* d_votes, uint8_t* d_keep, int64_t* d_count,
                      void* d_workspace, void* stream);
int nm_surface_gather(const void* d_workspace, const float* d_origins, int per_ray_o, const float* d_dirs,
                      const float* d_depth, const float* d_opacity, double min_opacity, const float* d_rgb, int32_t height,
                      int32_t width, int64_t row_offset, int64_t capacity, float* d_points, float* d_normals,
                      float* d_colors, uint8_t* d_colors_u8, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh components (mesh_nerf --min-component-faces / --keep-largest; DESIGN.md, "Mesh components").  An indexed triangle
 * mesh on the device: d_faces (F,3) int32 with entries in [0, V).  Two vertices are connected when a triangle holds both; a
 * component is a connected set of vertices plus the triangles on them.  Its LABEL is its smallest vertex index, its SIZE its
 * number of triangles; a vertex in no triangle is a component of size 0.
 *
 * nm_mesh_components: d_labels (V,) int32 = the label of every vertex; d_face_counts (V,) int32 = the size of the component
 *   at its label's entry, 0 everywhere else.  No host synchronisation.  A face with an index outside [0, V) joins nothing
 *   and is counted in the first 8 bytes of the workspace (uint64), which nm_mesh_components_select turns into an error.
 * nm_mesh_components_select: with those two arrays and the same workspace, decides what stays: components with fewer than
 *   min_faces triangles are dropped; of the rest, with keep_largest = K > 0, the K with most triangles stay, ties going to
 *   the smaller label (all of them when fewer than K are left); K = 0 keeps them all.  Returns on the HOST the numbers of
 *   vertices and faces kept, of components in the mesh and of components kept (the one synchronisation of the stream),
 *   and leaves the keep bits and their prefix sums in the workspace.  May be called again with other limits.
 * nm_mesh_components_compact: with that workspace, writes the kept rows IN THEIR ORIGINAL ORDER: d_out_faces
 *   (faces_kept,3) with vertices renumbered by the exclusive prefix sum of the vertex keep mask (numpy:
 *   new = cumsum(keep_v) - 1; out = new[faces[keep_f]]), and for every input that is not NULL -- d_verts (V,3), d_normals (V,3),
 *   d_values (V,) fp32, d_keys (V,) int64 -- its kept rows.  vertices_kept / faces_kept are the select call's and bound
 *   every write.  No host synchronisation.
 * V and F are in [0, 2^31 - 64); keep_largest is at most NM_MESH_KEEP_LARGEST_MAX.  The workspace
 * (nm_mesh_components_workspace_bytes, 0 for sizes out of range; 256-byte aligned) must stay untouched between the calls.
 * Argument errors return 2 before any HIP call.  Everything is integer work: the results do not depend on the order the
 * workgroups ran in.
 * ------------------------------------------------------------------------------------------ */
#define NM_MESH_KEEP_LARGEST_MAX 1024
int64_t nm_mesh_components_workspace_bytes(int64_t num_vertices, int64_t num_faces);
int nm_mesh_components(const int32_t* d_faces, int64_t num_faces, int64_t num_vertices, int32_t* d_labels,
                       int32_t* d_face_counts, void* d_workspace, void* stream);
int nm_mesh_components_select(const int32_t* d_faces, int64_t num_faces, int64_t num_vertices, const int32_t* d_labels,
                              const int32_t* d_face_counts, int64_t min_faces, int32_t keep_largest, void* d_workspace,
                              int64_t* h_vertices_kept, int64_t* h_faces_kept, int64_t* h_components,
                              int64_t* h_components_kept, void* stream);
int nm_mesh_components_compact(const void* d_workspace, const int32_t* d_faces, int64_t num_faces, int64_t num_vertices,
                               const float* d_verts, const float* d_normals, const float* d_values, const int64_t* d_keys,
                               int64_t vertices_kept, int64_t faces_kept, float* d_out_verts, int32_t* d_out_faces,
                               float* d_out_normals, float* d_out_values, int64_t* d_out_keys, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh quality: chamfer distance (mesh_chamfer, mesh_nerf --target-mesh, the validation chamfer branch; DESIGN.md, "Mesh
 * quality: chamfer distance").  All arrays on the device; d_verts (V,3) fp32, d_faces (F,3) int32.  Every fp32 operation
 * below is rounded on its own (no fused multiply-add), sqrt and division correctly rounded, in the order written, so a
 * numpy fp32 restatement (tests/mesh_metrics.py) reproduces every output bit for bit.
 *
 * nm_mesh_face_weights: area-proportional sampling weights as integers.  With e1 = v1 - v0, e2 = v2 - v0 and
 *   c = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x): area = 0.5f * sqrt((cx cx + cy cy) + cz cz); a non-finite
 *   area, and the area of a face with an index outside [0, V) (never dereferenced), is 0.  With m the largest area and
 *   m = f * 2^e, f in [0.5, 1): weight_i = (uint64) trunc((double) area_i * 2^(32-e)), so the largest weight lies in
 *   [2^31, 2^32) and A FACE WHOSE AREA IS BELOW m * 2^-32 HAS WEIGHT 0 AND IS NEVER SAMPLED.  d_areas (F,) fp32 (may be NULL);
 *   d_cdf (F,) uint64 = the inclusive prefix sums of the weights: exact, whatever order the workgroups ran in.  The workspace
 *   (nm_mesh_face_weights_workspace_bytes(), 16-byte aligned) begins with uint64 bad_faces (faces with an index out of
 *   range), uint64 total = d_cdf[F-1] (0 for F = 0), uint32 float bits of m.  No host synchronisation.
 * nm_mesh_sample_points: d_u (N,3) fp32 draws in [0, 1).  t = (uint64) trunc((double) u0 * (double) total); face = the first
 *   i with d_cdf[i] > t (binary search; t is clamped to total - 1 for a draw outside [0, 1)); s = sqrt(u1), w0 = 1 - s,
 *   w1 = s (1 - u2), w2 = s u2 (pytorch3d's barycentric weights); p = (w0 v0 + w1 v1) + w2 v2 per component.  Outputs, each
 *   may be NULL: d_points (N,3), d_face_ids (N,) int32, d_normals (N,3) = c / |c| of the face.  total = 0 writes nothing:
 *   read it from nm_mesh_face_weights' workspace first.  No host synchronisation.
 * nm_points_nearest: d_x (N,3), d_y (M,3) fp32.  For every row i of x: d_dist2[i] = min over j of
 *   ((dx dx + dy dy) + dz dz) with dx = x_i.x - y_j.x, ...; d_index[i] (int32) = the smallest j that attains it.  A pair whose
 *   d2 is NaN never wins; a row that no pair wins (a NaN query, M = 0) gets (+inf, -1).  Brute force over all N * M pairs with
 *   no N x M intermediate: the workspace is nm_points_nearest_workspace_bytes(N, M) = O(N) bytes (0 for sizes out of
 *   range; 256-byte aligned).  The result does not depend on the order the workgroups ran in.  No host synchronisation.
 * V, F, N and M are in [0, 2^31 - 64).  Argument errors return 2 before any HIP call.  Nothing allocates.
 * ------------------------------------------------------------------------------------------ */
int64_t nm_mesh_face_weights_workspace_bytes(void);
int nm_mesh_face_weights(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces, float* d_areas,
                         uint64_t* d_cdf, void* d_workspace, void* stream);
int nm_mesh_sample_points(const float* d_u, int64_t num_points, const float* d_verts, int64_t num_vertices, const int32_t* d_faces,
                          int64_t num_faces, const uint64_t* d_cdf, float* d_points, int32_t* d_face_ids, float* d_normals,
                          void* stream);
int64_t nm_points_nearest_workspace_bytes(int64_t num_x, int64_t num_y);
int nm_points_nearest(const float* d_x, int64_t num_x, const float* d_y, int64_t num_y, float* d_dist2, int32_t* d_index,
                      void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Point to mesh: the exact distance of points to the TRIANGLES of a mesh (mesh_chamfer --surface exact, mesh_nerf
 * --target-surface exact; DESIGN.md, "Mesh quality: exact surface distance").  d_x (N,3) fp32, d_verts (V,3) fp32, d_faces
 * (F,3) int32, all on the device.  fp32 with every operation rounded on its own (no fused multiply-add), division correctly
 * rounded, dot(u, v) = (ux vx + uy vy) + uz vz, u x v = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx), so a numpy fp32
 * restatement (tests/mesh_surface_distance.py) reproduces every output bit for bit.  Per query p and face (a, b, c):
 *   ab = b - a, ac = c - a, bc = c - b, ca = a - c;  ap = p - a, bp = p - b, cp = p - c.
 *   seg(q, e): r = 1 / dot(e, e); t = dot(q, e) * r; t = fmin(fmax(t, 0), 1) with fmax / fmin returning their non-NaN operand
 *     (a zero-length edge has r = inf, t = NaN or inf -> 0 or 1 times a zero vector: the distance to the point);
 *     d = q - t * e per component; the term is dot(d, d).
 *   s1 = seg(ap, ab), s2 = seg(bp, bc), s3 = seg(cp, ca).
 *   n = ab x ac, nn = dot(n, n); inside = dot(n, ab x ap) >= 0 && dot(n, bc x bp) >= 0 && dot(n, ca x cp) >= 0 && nn > 0;
 *   h = dot(n, ap); pl = (h * h) * (1 / nn) where `inside` holds and the value is finite, else +inf.
 *   d2 = min(min(s1, s2), min(s3, pl)), and NaN when any of s1, s2, s3 is NaN.
 * The value of one face never depends on another face, and every degenerate face is defined: a zero-area face is its
 * segments, a point face the point.  d_dist2[i] = the smallest d2 over the faces; d_face[i] (int32) = the smallest face index
 * that attains it; d_face_normals (N,3), may be NULL = c / |c| of that face exactly as nm_mesh_sample_points writes it (NaN
 * for |c| = 0).  A pair whose d2 is NaN never wins (a NaN vertex takes out its own faces only); a face with an index outside
 * [0, V) is never dereferenced and never wins; a row that no face wins (a NaN query, F = 0) gets (+inf, -1, NaN normal).
 * Brute force over all N * F pairs, no spatial culling: a bound computed in fp32 could exceed the computed distance of a
 * near-coplanar face.  The workspace is nm_points_to_mesh_workspace_bytes(N, F) bytes (one 112-byte record per face and 8
 * bytes per query; 0 for sizes out of range; 256-byte aligned).  The result does not depend on the order the workgroups ran
 * in.  V, F and N are in [0, 2^31 - 64).  Argument errors return 2 before any HIP call.  No allocation, no host
 * synchronisation.
 * ------------------------------------------------------------------------------------------ */
int64_t nm_points_to_mesh_workspace_bytes(int64_t num_x, int64_t num_faces);
int nm_points_to_mesh(const float* d_x, int64_t num_x, const float* d_verts, int64_t num_vertices, const int32_t* d_faces,
                      int64_t num_faces, float* d_dist2, int32_t* d_face, float* d_face_normals, void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mesh simplification by vertex clustering (mesh_nerf --simplify-cell; DESIGN.md, "Mesh simplification").  All arrays on
 * the device: d_verts (V,3) fp32, d_faces (F,3) int32, d_normals (V,3) fp32 or NULL.  The grid is (origin, cell): cell is
 * finite and > 0, the origin finite.  Every fp32 / fp64 operation below is rounded on its own (no fused multiply-add), sqrt
 * and division correctly rounded, so a numpy restatement (tests/mesh_simplify.py) reproduces every output bit for bit; all
 * sums are exact integer sums, so the outputs do not depend on the order the workgroups ran in.
 *
 *   cell      c = floorf((x - origin) / cell) per axis.  A vertex with a non-finite coordinate or a c outside [0, 2^21) is BAD:
 *             counted, in no cluster.  A face with an index outside [0, V) (never dereferenced) or with a bad vertex is BAD:
 *             counted, left out.  A caller should treat either count as an error (hip_ops.mesh_simplify raises).
 *   cluster   all vertices of one cell; its REPRESENTATIVE is its smallest vertex index.
 *   position  one member: that member's row, bit for bit (position and normal).  More: with lo = origin + c * cell,
 *             t = (x - lo) / cell, q = (int64) rint((double) t * 2^30) clamped to [-2^31, 2^31] (t lies in [0, 1] up to
 *             rounding; the clamp makes the bound hold for every input), S = the int64 sum of q over the n members (fewer
 *             than 2^31 of them, so |S| < 2^62: exact):  p = (float)((double) lo + (double) cell * ((double) S / ((double) n * 2^30))).
 *   normal    q = (int64) rint((double) component * 2^30) of the members whose three components are finite and at most 2 in
 *             magnitude (|q| <= 2^31, the same bound); any other member contributes nothing.  With s = (float) S per
 *             component: normal = s / sqrt((sx sx + sy sy) + sz sz) in fp32, or the representative's own normal when S is
 *             the zero vector.
 *   faces     every corner is replaced by its cluster.  A face with two equal corners is DEGENERATE and goes.  Two of the
 *             others are DUPLICATES when they have the same corners in the same cyclic order (compare with the smallest
 *             corner rotated to the front); opposite windings are not duplicates.  Of duplicates the smallest face index
 *             stays.  Kept faces stay in input order, corners in their own order.
 *   vertices  a cluster no kept face references goes; the others are numbered by ascending representative (numpy:
 *             new = cumsum(used) - 1 over the representatives' indices).
 *
 * nm_mesh_simplify_cluster: clusters, filters and scans; returns on the HOST (the one synchronisation of the stream)
 *   h_counts[NM_MESH_SIMPLIFY_COUNTS]: clusters, vertices kept, faces kept, degenerate faces, duplicate faces, bad vertices,
 *   bad faces (the NM_MESH_SIMPLIFY_* indices below).  flags: 0, or NM_MESH_SIMPLIFY_AGGREGATE to sum the lanes of a wave
 *   that share a cluster in registers before the atomics (the same results; another speed).
 * nm_mesh_simplify_emit: with that workspace and THE SAME mesh and grid, writes d_out_verts (vertices_kept,3), d_out_faces
 *   (faces_kept,3) and d_out_normals (vertices_kept,3; NULL when d_normals is NULL).  vertices_kept / faces_kept are the
 *   cluster call's and bound every write.  No host synchronisation.
 * V and F are in [0, 2^31 - 64).  The workspace (nm_mesh_simplify_workspace_bytes, 0 for sizes out of range; 256-byte
 * aligned; 64 bytes per slot of a table of the smallest power of two >= 2 V slots, 4 per slot of one of >= 2 F) must stay
 * untouched between the two calls.  Argument errors -- a null array with a non-zero size, a cell that is not finite or
 * <= 0, a non-finite origin -- return 2 before any HIP call.
 *
 * QUADRIC PLACEMENT (mesh_nerf --simplify-placement quadric): the clustering, the faces, the numbering, the normals and a
 * cluster of one member are the above; only the position of a cluster of n >= 2 members changes, to the point of its cell
 * nearest (least squares, area^2 weights) to the planes of the faces around it -- Lindstrom's quadric-optimal representative
 * with integer quadrics.  c, lo, t, S and n are the above; MSQ_LATTICE = 2^8, MSQ_MAX_CONTRIBUTIONS = 2^13, MSQ_LAMBDA = 2^-6.
 *   lattice   u = (int64) rint((double) t * 2^8) per axis, clamped to [-2^9, 2^9]: a vertex on a lattice local to its cell.
 *   corner    every face that is not BAD contributes once per corner k, to the cluster of that corner.  With C = (int64) c:
 *             e1 = (C1 - C0) * 2^8 + (u1 - u0), e2 likewise for the third corner, in the face's cyclic order starting at k.
 *             A component of e1 or e2 beyond 2^9 in magnitude (two cells) makes the corner FAR: counted, no contribution.
 *             Else nrm = e1 x e2 (|component| <= 2^19), d = -(nrm . u0) (|d| <= 3 * 2^28), and the corner adds the six
 *             nrm_i nrm_j (<= 2^38) to A, the three nrm_i d (< 2^49) to B and 1 to the cluster's contributions.  A face
 *             with two corners in one cluster adds twice; one with a repeated index adds zeros and counts.
 *   crowded   a cluster with more than 2^13 contributions is CROWDED: its sums are not read, it gets the mean.  Below that
 *             |sum A| <= 2^51 and |sum B| < 2^62: exact int64 sums in any order.
 *   position  of a kept cluster with n >= 2, 1 <= contributions <= 2^13 and tr > 0, in fp64, every operation rounded on its own:
 *               m_j = ((double) S_j / ((double) n * 2^30)) * 2^8;  a = (double) A, b = (double) B;  tr = (a00 + a11) + a22
 *               M = a with tr * 2^-6 added to the diagonal;  r_j = -(((a_j0 m0 + a_j1 m1) + a_j2 m2) + b_j)
 *               c00 = M11 M22 - M12 M12   c01 = M02 M12 - M01 M22   c02 = M01 M12 - M02 M11
 *               c11 = M00 M22 - M02 M02   c12 = M01 M02 - M00 M12   c22 = M00 M11 - M01 M01
 *               det = (M00 c00 + M01 c01) + M02 c02
 *               delta0 = ((c00 r0 + c01 r1) + c02 r2) / det   delta1 = ((c01 r0 + c11 r1) + c12 r2) / det
 *               delta2 = ((c02 r0 + c12 r1) + c22 r2) / det
 *             det > 0 fails or a delta is not finite: SINGULAR, the mean.  Else x = m + delta, each component clamped to
 *             [0, 2^8] (CLAMPED when a clamp acted), p = (float)((double) lo + (double) cell * (x / 2^8)): SOLVED.  The
 *             regulariser bounds the condition number by about 200 and leaves the vertex at the mean along directions the
 *             planes do not constrain (flat regions, open boundaries, a crease along itself).  0 contributions or tr = 0:
 *             the mean, counted nowhere.
 * nm_mesh_simplify_quadric_faces: after nm_mesh_simplify_cluster, with its workspace and THE SAME mesh and grid: zeroes the
 *   second workspace (nm_mesh_simplify_quadric_workspace_bytes: 128 bytes per slot of the vertex table; 0 for sizes out of
 *   range) and sums the corners' contributions into it.  flags as above.  No host synchronisation.
 * nm_mesh_simplify_emit_quadric: nm_mesh_simplify_emit with the positions above; returns on the HOST (it synchronises the
 *   stream) h_counts[NM_MESH_SIMPLIFY_QUADRIC_COUNTS]: the kept clusters that are SOLVED (the CLAMPED among them included),
 *   CROWDED, SINGULAR and CLAMPED, and the FAR corners of all faces.  Both workspaces must stay untouched between the calls.
 * ------------------------------------------------------------------------------------------ */
#define NM_MESH_SIMPLIFY_AGGREGATE 1
#define NM_MESH_SIMPLIFY_CLUSTERS 0
#define NM_MESH_SIMPLIFY_VERTICES_KEPT 1
#define NM_MESH_SIMPLIFY_FACES_KEPT 2
#define NM_MESH_SIMPLIFY_DEGENERATE 3
#define NM_MESH_SIMPLIFY_DUPLICATE 4
#define NM_MESH_SIMPLIFY_BAD_VERTICES 5
#define NM_MESH_SIMPLIFY_BAD_FACES 6
#define NM_MESH_SIMPLIFY_COUNTS 7
int64_t nm_mesh_simplify_workspace_bytes(int64_t num_vertices, int64_t num_faces);
int nm_mesh_simplify_cluster(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                             const float* d_normals, float origin_x, float origin_y, float origin_z, float cell, int32_t flags,
                             void* d_workspace, int64_t* h_counts, void* stream);
int nm_mesh_simplify_emit(const void* d_workspace, const float* d_verts, int64_t num_vertices, const int32_t* d_faces,
                          int64_t num_faces, const float* d_normals, float origin_x, float origin_y, float origin_z, float cell,
                          int64_t vertices_kept, int64_t faces_kept, float* d_out_verts, int32_t* d_out_faces,
                          float* d_out_normals, void* stream);
#define NM_MESH_SIMPLIFY_QUADRIC_SOLVED 0
#define NM_MESH_SIMPLIFY_QUADRIC_CROWDED 1
#define NM_MESH_SIMPLIFY_QUADRIC_SINGULAR 2
#define NM_MESH_SIMPLIFY_QUADRIC_CLAMPED 3
#define NM_MESH_SIMPLIFY_QUADRIC_FAR 4
#define NM_MESH_SIMPLIFY_QUADRIC_COUNTS 5
int64_t nm_mesh_simplify_quadric_workspace_bytes(int64_t num_vertices, int64_t num_faces);
int nm_mesh_simplify_quadric_faces(const void* d_workspace, const float* d_verts, int64_t num_vertices, const int32_t* d_faces,
                                   int64_t num_faces, float origin_x, float origin_y, float origin_z, float cell, int32_t flags,
                                   void* d_quadric_workspace, void* stream);
int nm_mesh_simplify_emit_quadric(const void* d_workspace, void* d_quadric_workspace, const float* d_verts, int64_t num_vertices,
                                  const int32_t* d_faces, int64_t num_faces, const float* d_normals, float origin_x,
                                  float origin_y, float origin_z, float cell, int64_t vertices_kept, int64_t faces_kept,
                                  float* d_out_verts, int32_t* d_out_faces, float* d_out_normals, int64_t* h_counts,
                                  void* stream);

/* ------------------------------------------------------------------------------------------
 * ADAPTIVE LEVELS of the quadric placement (mesh_nerf --simplify-levels L / --simplify-error E; DESIGN.md, "Adaptive
 * clustering"): Schaefer and Warren's adaptive vertex clustering on the nested grids (origin, cell * 2^l), l = 0 .. L
 * (1 <= L <= NM_MESH_SIMPLIFY_MAX_LEVELS = 8).  cell * 2^l is exact in fp32 (it must stay finite), so a vertex's cell at
 * level l is c_0 >> l per axis: the cells of level l + 1 are unions of eight cells of level l.  Every vertex joins the
 * cluster of the COARSEST level whose cell is acceptable; everything else is the quadric placement above, bit for bit.
 *   level     a cluster of level l is the set of vertices of one cell of that grid.  Its members, representative, position
 *             and normal sums, its quadric (on the lattice of 2^8 points per edge of THAT level's cell, FAR meaning two of that
 *             level's cells), its status and its place x are what the sections above define for a grid of that cell size,
 *             computed from the faces directly -- never from its children's sums --, so every overflow bound above holds per level.
 *   error     of a cluster of n >= 2 members that is SOLVED: over every corner that contributed to it with nrm != 0, with
 *             x = (x / 2^8) * 2^8 in fp64 as the position step leaves it (clamped), u0 the corner's lattice point, all in fp64,
 *             every operation rounded on its own:
 *               d2 = ((n0 (x0 - u0_0) + n1 (x1 - u0_1)) + n2 (x2 - u0_2))^2 / ((n0 n0 + n1 n1) + n2 n2)
 *             the squared distance, in lattice units, of x from the corner's plane.  The cluster's error is the MAXIMUM d2
 *             (0 without such a corner): a maximum of non-negative doubles is the maximum of their bits and does not depend
 *             on the order it is taken in.
 *   accept    at level l >= 1 a cluster of one member is acceptable; one of more members iff it is SOLVED (clamped or not: so
 *             neither CROWDED nor SINGULAR, with a contribution and a positive trace), none of its corners is FAR (such a
 *             corner's plane was never tested) and its error <= tol_l^2, where, in fp64 in this order,
 *               tol_l = (max_error / (double) (cell * 2^l)) * 2^8,  tol_l^2 = tol_l * tol_l     (max_error >= 0, +inf allowed).
 *             Every cluster of level 0 is acceptable: the output is never finer than the uniform clustering with `cell`
 *             and never coarser than the one with cell * 2^L.
 *   choice    a vertex joins the cluster of the largest l whose cell is acceptable.  Acceptance is a property of the cell,
 *             and all members of a cell share every coarser cell, so they choose alike: the chosen cells partition the
 *             vertices.  A refused cluster none of whose coarser cells was chosen is counted once, by the first reason of:
 *             crowded, no contribution (or zero trace), singular, far, error.
 *   output    faces, duplicates and numbering as above through the final representatives.  A chosen cluster of one member
 *             emits its rows bit for bit; another p = (float)((double) lo_l + (double) (cell * 2^l) * (x / 2^8)) (the mean
 *             where level 0 is not SOLVED) and the normal of the level's integer normal sum by the rule above.
 * nm_mesh_simplify_adaptive_level: ONE level: call it for level = levels, levels - 1, .., 0 in this order with THE SAME mesh,
 *   grid, error and three workspaces -- nm_mesh_simplify_workspace_bytes, nm_mesh_simplify_quadric_workspace_bytes, both
 *   reused by every level, and nm_mesh_simplify_adaptive_workspace_bytes (a header and 30 bytes per vertex of staged rows; 0
 *   for sizes out of range): memory does not grow with the number of levels.  `cell` is level 0's.  flags:
 *   NM_MESH_SIMPLIFY_AGGREGATE for the vertex pass, NM_MESH_SIMPLIFY_AGGREGATE_FACES for the two face passes (the same
 *   results; another speed).  No host synchronisation.
 * nm_mesh_simplify_adaptive_faces: after level 0: filters the faces and scans; returns on the HOST (it synchronises the stream)
 *   h_counts[NM_MESH_SIMPLIFY_ADAPTIVE_COUNTS]: the NM_MESH_SIMPLIFY_* counts (clusters: the chosen ones of all levels), then
 *   for l = 0 .. levels at NM_MESH_SIMPLIFY_COUNTS + l * NM_MESH_SIMPLIFY_LEVEL_FIELDS the NM_MESH_SIMPLIFY_LEVEL_* fields:
 *   vertices that chose level l, clusters chosen there, clusters refused there per reason, and the bits of the largest error
 *   d2 of a cluster of n >= 2 chosen there (l >= 1; lattice units of that level, squared).
 * nm_mesh_simplify_adaptive_emit: writes the outputs as nm_mesh_simplify_emit does (with_normals: d_normals was given to the
 *   levels); returns on the HOST h_counts[NM_MESH_SIMPLIFY_ADAPTIVE_EMIT_COUNTS]: the NM_MESH_SIMPLIFY_QUADRIC_* counts of the
 *   kept clusters at their chosen level (FAR: level 0's corners), then the kept clusters of level 0 .. levels.
 * Argument errors return 2 before any HIP call.  A mesh with BAD vertices or faces gives the counts and unspecified rows.
 * ------------------------------------------------------------------------------------------ */
#define NM_MESH_SIMPLIFY_AGGREGATE_FACES 2
#define NM_MESH_SIMPLIFY_MAX_LEVELS 8
#define NM_MESH_SIMPLIFY_LEVEL_VERTICES 0
#define NM_MESH_SIMPLIFY_LEVEL_CLUSTERS 1
#define NM_MESH_SIMPLIFY_LEVEL_REFUSED_ERROR 2
#define NM_MESH_SIMPLIFY_LEVEL_REFUSED_CROWDED 3
#define NM_MESH_SIMPLIFY_LEVEL_REFUSED_SINGULAR 4
#define NM_MESH_SIMPLIFY_LEVEL_REFUSED_FAR 5
#define NM_MESH_SIMPLIFY_LEVEL_REFUSED_EMPTY 6
#define NM_MESH_SIMPLIFY_LEVEL_MAX_D2 7
#define NM_MESH_SIMPLIFY_LEVEL_FIELDS 8
#define NM_MESH_SIMPLIFY_ADAPTIVE_COUNTS (NM_MESH_SIMPLIFY_COUNTS + (NM_MESH_SIMPLIFY_MAX_LEVELS + 1) * NM_MESH_SIMPLIFY_LEVEL_FIELDS)
#define NM_MESH_SIMPLIFY_ADAPTIVE_EMIT_COUNTS (NM_MESH_SIMPLIFY_QUADRIC_COUNTS + NM_MESH_SIMPLIFY_MAX_LEVELS + 1)
int64_t nm_mesh_simplify_adaptive_workspace_bytes(int64_t num_vertices, int64_t num_faces);
int nm_mesh_simplify_adaptive_level(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                                    const float* d_normals, float origin_x, float origin_y, float origin_z, float cell,
                                    int32_t level, int32_t levels, double max_error, int32_t flags, void* d_workspace,
                                    void* d_quadric_workspace, void* d_adaptive_workspace, void* stream);
int nm_mesh_simplify_adaptive_faces(const int32_t* d_faces, int64_t num_faces, int64_t num_vertices, int32_t levels,
                                    void* d_workspace, void* d_adaptive_workspace, int64_t* h_counts, void* stream);
int nm_mesh_simplify_adaptive_emit(const void* d_workspace, void* d_adaptive_workspace, const int32_t* d_faces, int64_t num_faces,
                                   int64_t num_vertices, int32_t levels, int32_t with_normals, int64_t vertices_kept,
                                   int64_t faces_kept, float* d_out_verts, int32_t* d_out_faces, float* d_out_normals,
                                   int64_t* h_counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Taubin smoothing of a mesh (mesh_nerf --smooth-iters; DESIGN.md, "Mesh smoothing").  All arrays on the device: d_verts
 * (V,3) fp32, d_faces (F,3) int32.  A uniform umbrella Laplacian applied with a factor lambda in (0, 1], then with mu in
 * [-1, 0] (mu = 0: the second half-step is skipped, which is plain Laplacian smoothing).  Every fp32 / fp64 operation below
 * is rounded on its own, division and sqrt correctly rounded, and every per-vertex sum is an exact integer sum, so a numpy
 * restatement (tests/mesh_smooth.py) reproduces every output bit for bit, whatever the order of the workgroups, of a
 * neighbour list or of the numbering.
 *
 *   validity   a vertex with a non-finite coordinate is BAD; a face with an index outside [0, V) (never dereferenced) is BAD.
 *              Both are counted; a caller should treat either count as an error (hip_ops.mesh_smooth raises).  A face with
 *              two equal corners is DEGENERATE: counted, it contributes no edge.
 *   edges      every other face contributes its three undirected edges (min, max).  u and v are NEIGHBOURS when an edge joins
 *              them; a neighbour counts once however many faces share the edge (duplicate faces, both windings, fans).
 *   boundary   an edge on exactly one face is a BOUNDARY edge and its two ends are boundary vertices; an edge on more than two
 *              faces is NON-MANIFOLD (counted, not boundary).  Boundary vertices are pinned unless NM_MESH_SMOOTH_FREE_BOUNDARY;
 *              a vertex of degree 0 (ISOLATED) never moves.  A pinned or isolated vertex leaves bit for bit as it came.
 *   half-step  with factor f, degree n, e = the binary exponent of the largest |coordinate| of the INPUT mesh (every
 *              |x| < 2^e; frexp's) and shift = 40 - e:
 *                q  = (int64) rint(ldexp((double) x, shift)) clamped to [-2^43, 2^43] (a NaN to the lower bound)
 *                hi = sum (q >> 20), lo = sum (q & 0xFFFFF) over the neighbours, per component (|hi| < 2^54, lo < 2^51: exact)
 *                m  = ldexp(((double) hi * 2^20 + (double) lo) / (double) n, -shift)
 *                x' = (float)((double) x + (double) f * (m - (double) x))
 *              every vertex reads the previous half-step's positions.  A mesh whose largest |coordinate| is 0 is returned as is.
 *   normals    per non-degenerate face n = cross(b - a, c - a) in fp32 (each component left - right of two rounded
 *              products), len = sqrt((nx nx + ny ny) + nz nz); a face whose len is zero or not finite is skipped;
 *              q = (int64) rint((double) ((n / len) * flip) * 2^30) per component is added to the three corners (int64:
 *              exact).  With s = (float) S per component: normal = s / sqrt((sx sx + sy sy) + sz sz), or, when S is the
 *              zero vector, the vertex's input normal ((0, 0, 0) when d_in_normals is NULL).
 *
 * nm_mesh_smooth_build: validates, builds the edge table, the boundary bits and the adjacency (CSR, 64-bit offsets); returns
 *   on the HOST (the one synchronisation of the stream) h_counts[NM_MESH_SMOOTH_COUNTS]: edges, boundary edges, non-manifold
 *   edges, boundary vertices, isolated vertices, degenerate faces, bad vertices, bad faces and the exponent e (0 for a largest
 *   coordinate of 0) -- the NM_MESH_SMOOTH_* indices below.
 * nm_mesh_smooth_run: with that workspace and THE SAME vertices, launches the 2 * iterations half-steps (iterations when
 *   mu = 0) with no host round trip; the second position buffer lives in the workspace; d_out_verts (V,3) must not be d_verts.
 *   iterations in [0, 1000]; 0 copies the input.  flags: 0 or NM_MESH_SMOOTH_FREE_BOUNDARY.
 * nm_mesh_vertex_normals: the vertex normals of (d_verts, d_faces) into d_out_normals (V,3); flip is +1 or -1; d_in_normals
 *   (V,3) or NULL.  The workspace is one of nm_mesh_smooth_workspace_bytes(V, F); the call clears the part it uses and leaves
 *   what nm_mesh_smooth_build put there alone.  No host synchronisation.
 * V and F are in [0, 2^31 - 64).  The workspace (nm_mesh_smooth_workspace_bytes, 0 for sizes out of range; 256-byte aligned;
 * 12 bytes per slot of a table of the smallest power of two >= 6 F slots, 4 * 6 F for the neighbour lists, 52 V for the
 * rest) must stay untouched between build and run.  Argument errors -- a null array with a non-zero size, lambda, mu or
 * iterations out of range, unknown flags, a flip that is not +-1 -- return 2 before any HIP call.
 * ------------------------------------------------------------------------------------------ */
#define NM_MESH_SMOOTH_FREE_BOUNDARY 1
#define NM_MESH_SMOOTH_EDGES 0
#define NM_MESH_SMOOTH_BOUNDARY_EDGES 1
#define NM_MESH_SMOOTH_NONMANIFOLD_EDGES 2
#define NM_MESH_SMOOTH_BOUNDARY_VERTICES 3
#define NM_MESH_SMOOTH_ISOLATED_VERTICES 4
#define NM_MESH_SMOOTH_DEGENERATE 5
#define NM_MESH_SMOOTH_BAD_VERTICES 6
#define NM_MESH_SMOOTH_BAD_FACES 7
#define NM_MESH_SMOOTH_EXPONENT 8
#define NM_MESH_SMOOTH_COUNTS 9
int64_t nm_mesh_smooth_workspace_bytes(int64_t num_vertices, int64_t num_faces);
int nm_mesh_smooth_build(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces, void* d_workspace,
                         int64_t* h_counts, void* stream);
int nm_mesh_smooth_run(const void* d_workspace, const float* d_verts, int64_t num_vertices, int32_t iterations, float lambda,
                       float mu, int32_t flags, float* d_out_verts, void* stream);
int nm_mesh_vertex_normals(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                           const float* d_in_normals, int32_t flip, void* d_workspace, float* d_out_normals, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rasteriser of a mesh (mesh_render, mesh_nerf --render-views; DESIGN.md, "Mesh render"): which face a pinhole camera sees at
 * every pixel, its depth and its barycentrics.  All arrays on the device: d_verts (V,3) fp32, d_faces (F,3) int32.  Coverage is
 * exact integer work and visibility a 64-bit minimum, every fp32 / fp64 operation is rounded on its own and division is
 * correctly rounded, so a numpy restatement (tests/mesh_raster.py) reproduces every output bit for bit, whatever the order of
 * the workgroups and whichever path drew a face.
 *
 *   view       a non-NDC nm_view: R = c2w[:3,:3], t = c2w[:3,3], height and width in [1, 16384], focal finite and > 0.
 *   vertex     in fp64: d = (double) p - (double) t; xc = (R00 dx + R10 dy) + R20 dz, yc and zc with columns 1 and 2 of R;
 *              w = (float)(-zc); u = (xc / (double) w) focal + width 0.5; v = -(yc / (double) w) focal + height 0.5;
 *              X = rint(u 256), Y = rint(v 256): 8 sub-pixel bits.  Pixel (row j, column i) is sampled at (X, Y) = (256 i,
 *              256 j), without a half-pixel offset: get_ray_bundle's convention.  The camera-space ray is (x, y, -1) and w the
 *              distance along the camera's axis; get_ray_bundle normalises its directions, so the NeRF's depth_map is w times
 *              |(x, y, -1)| of the pixel (mesh_render.ray_lengths).  A vertex is NOT FINITE when a coordinate or w is not finite, OUT OF RANGE
 *              when not |u 256| <= 2^24 or not |v 256| <= 2^24 (every edge function then stays below 2^51 in int64).
 *   face       rejected, and counted under the FIRST of these reasons that holds: an index outside [0, V) (never
 *              dereferenced); a corner not finite; a corner with w < near (there is no near-plane clipping: the count tells);
 *              a corner out of range; back-facing under NM_MESH_RASTER_CULL_BACK (A > 0: clockwise on the screen, whose Y axis
 *              points down; front faces wind counter-clockwise as seen, the OBJ convention); no pixel centre inside the
 *              bounding box clipped to the screen; A == 0.  A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) in int64.
 *   coverage   e0 = (X2 - X1)(Py - Y1) - (Y2 - Y1)(Px - X1), e1 and e2 with the corners rotated, in int64.  For A < 0 every e,
 *              every edge vector and A change sign: the face with two corners swapped, the barycentrics staying in the face's
 *              own corner order.  A pixel is inside when every e > 0, or e == 0 on a top or left edge (edge vector (dx, dy):
 *              dy < 0, or dy == 0 and dx > 0).  A sheet of triangles covers every pixel exactly once, vertices on pixel
 *              centres included.
 *   depth      lk = (double) ek / (double) A; ik = 1.0 / (double) wk; q = (l0 i0 + l1 i1) + l2 i2; depth = (float)(1.0 / q);
 *              bk = (float)((lk ik) / q).  A pixel whose depth is not finite or not > 0 is not covered.
 *   winner     the minimum over the covering faces of (bits of depth) << 32 | face index: the nearest face, an exact tie to
 *              the smallest index.
 *
 * nm_mesh_rasterize -> d_face_id (H,W) int32 (-1: nothing drawn), d_depth (H,W) fp32 (0), d_bary (H,W,3) fp32 (0) and, on the
 *   DEVICE, d_counts[NM_MESH_RASTER_COUNTS] int64: the faces drawn, those rejected under each reason, those of the drawn ones
 *   that took the large path, the covered pixels and the fragments -- the (face, pixel) pairs that passed the coverage and depth
 *   rules, each of which is a candidate for the pixel's word: the most atomics a frame can issue -- the NM_MESH_RASTER_*
 *   indices below.  A face whose clipped bounding box
 *   holds more than large_threshold (>= 0) pixel centres is drawn by a whole wave, the others by one lane each: the same
 *   bytes, another speed.  The entry allocates nothing and never waits for the host; it can be captured into a graph.
 * nm_mesh_interpolate: out[p][c] = (b0 a0[c] + b1 a1[c]) + b2 a2[c] in fp32 with ak the rows of d_attributes (V,C), C in
 *   [1, 16], at the corners of face d_face_id[p]; d_background[c] where the id is not in [0, F) or the face has an index
 *   outside [0, V).  d_out is (pixels, C).  Capturable likewise.
 * V and F are in [0, 2^31 - 64).  The workspace (nm_mesh_raster_workspace_bytes, 0 for sizes out of range; 256-byte aligned):
 * 8 H W for the visibility words, 12 V for the projected vertices, 4 F for the queue of the large path.  Argument errors -- a
 * null array with a non-zero size, an NDC view, near not finite and > 0, unknown flags, C out of range -- return 2 before any
 * HIP call.
 * ------------------------------------------------------------------------------------------ */
#define NM_MESH_RASTER_CULL_BACK 1
#define NM_MESH_RASTER_DRAWN 0
#define NM_MESH_RASTER_BAD_INDEX 1
#define NM_MESH_RASTER_NOT_FINITE 2
#define NM_MESH_RASTER_NEAR 3
#define NM_MESH_RASTER_OUT_OF_RANGE 4
#define NM_MESH_RASTER_CULLED 5
#define NM_MESH_RASTER_OFF_SCREEN 6
#define NM_MESH_RASTER_DEGENERATE 7
#define NM_MESH_RASTER_LARGE 8
#define NM_MESH_RASTER_COVERED 9
#define NM_MESH_RASTER_FRAGMENTS 10
#define NM_MESH_RASTER_COUNTS 11
#define NM_MESH_INTERPOLATE_MAX_CHANNELS 16
int64_t nm_mesh_raster_workspace_bytes(int64_t num_vertices, int64_t num_faces, int32_t height, int32_t width);
int nm_mesh_rasterize(const nm_view* view, const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                      float near, int32_t flags, int32_t large_threshold, void* d_workspace, int32_t* d_face_id, float* d_depth,
                      float* d_bary, int64_t* d_counts, void* stream);
int nm_mesh_interpolate(const int32_t* d_face_id, const float* d_bary, int64_t num_pixels, const int32_t* d_faces, int64_t num_faces,
                        const float* d_attributes, int64_t num_vertices, int32_t channels, const float* d_background, float* d_out,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Hidden faces of a mesh (mesh_nerf --cull-hidden-views; DESIGN.md, "Hidden faces"): the faces that no camera of a set sees
 * are dropped.  Built on the rasteriser above: integer work only, the same bytes whatever order the workgroups ran in, and a
 * numpy restatement (tests/mesh_visibility.py) reproduces every array and every count bit for bit.  THE RULE:
 *
 *   inputs     d_verts (V,3) fp32, d_faces (F,3) int32; M views under the constraints of nm_mesh_rasterize (non-NDC, sides in
 *              [1, 16384], focal finite and > 0); near, large_threshold as there; rings >= 0.
 *   seen       the views are taken in the order given.  Each runs the rasteriser's vertex stage and its two face paths exactly
 *              as nm_mesh_rasterize does without NM_MESH_RASTER_CULL_BACK: both windings drawn, the same reject reasons.  Face f
 *              is SEEN when it is the winner -- the low 32 bits of the pixel's word -- of at least one pixel of at least one
 *              view.  new_faces[k] = the faces whose bit view k set first: the views run in stream order, exactly one atomic OR
 *              per bit observes it clear, and a bit read as set is never counted (bits only rise, as the pixels' words only
 *              fall).
 *   rings      `rings` times: (1) the vertex bit of every corner of every kept face is set; (2) every face with valid indices
 *              and at least one marked corner becomes kept.  Step 2 reads only what step 1 finished writing.  This keeps the
 *              faces smaller than a pixel, which win no pixel centre, next to faces that did.  rings = 0 keeps the winners.
 *   bad faces  a face with an index outside [0, V) is never dereferenced and never kept; it is counted.
 *   output     the kept faces in their original order; a vertex is kept iff a kept face uses it; renumbering as numpy's
 *              new = cumsum(keep_v) - 1; out = new[faces[keep_f]] (csrc/compact.h: no atomic queue); the kept rows of every
 *              per-vertex input that is not NULL; optionally the kept faces' original indices.
 *
 * nm_mesh_visibility_views: `views` is a HOST array of num_views >= 0 nm_view.  Per view: the words cleared, the vertex stage,
 *   the two face paths, then one thread per pixel marks the winner (a lane whose left neighbour holds the same face leaves the
 *   atomic to it; the count is taken per wave by ballot).  clear != 0 zeroes the seen bits first; with clear == 0 a call
 *   accumulates onto the bits of the calls before it (the first call on a workspace must clear).  d_new_faces (num_views,)
 *   int64 on the DEVICE; d_reject_counts (num_views, NM_MESH_RASTER_COUNTS) int64 on the device, or NULL: every view's
 *   nm_mesh_rasterize counts.  Allocates nothing and never waits for the host.
 * nm_mesh_visibility_select: the rings, the final vertex bits and the prefix sums, then the one host synchronisation: the
 *   numbers of vertices and faces kept, of faces seen and of bad faces.  It starts from the seen bits and leaves them intact: it
 *   may be called again with another `rings` (at most NM_MESH_VISIBILITY_MAX_RINGS).
 * nm_mesh_visibility_compact: with that workspace, d_out_verts / d_out_normals (vertices_kept,3) for the inputs that are not
 *   NULL, d_out_faces (faces_kept,3), d_out_face_index (faces_kept,) int32 or NULL.  No host synchronisation.
 * V and F are in [0, 2^31 - 64).  The workspace (nm_mesh_visibility_workspace_bytes, 0 for sizes out of range; 256-byte aligned)
 * holds a header, the seen, face and vertex bits (one 64-bit word per 64 elements), their popcount prefix sums and the
 * rasteriser's workspace for max_height max_width pixels, the product no view may exceed; it must stay untouched between the
 * calls.  Argument errors return 2 before any HIP call, in the rasteriser's words where the condition is the rasteriser's.
 * ------------------------------------------------------------------------------------------ */
#define NM_MESH_VISIBILITY_MAX_RINGS 1024
int64_t nm_mesh_visibility_workspace_bytes(int64_t num_vertices, int64_t num_faces, int32_t max_height, int32_t max_width);
int nm_mesh_visibility_views(const nm_view* views, int64_t num_views, const float* d_verts, int64_t num_vertices,
                             const int32_t* d_faces, int64_t num_faces, float near, int32_t large_threshold, int32_t clear,
                             void* d_workspace, int64_t* d_new_faces, int64_t* d_reject_counts, void* stream);
int nm_mesh_visibility_select(const int32_t* d_faces, int64_t num_faces, int64_t num_vertices, int32_t rings, void* d_workspace,
                              int64_t* h_vertices_kept, int64_t* h_faces_kept, int64_t* h_faces_seen, int64_t* h_bad_faces,
                              void* stream);
int nm_mesh_visibility_compact(const void* d_workspace, const int32_t* d_faces, int64_t num_faces, int64_t num_vertices,
                               const float* d_verts, const float* d_normals, int64_t vertices_kept, int64_t faces_kept,
                               float* d_out_verts, int32_t* d_out_faces, float* d_out_normals, int32_t* d_out_face_index,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Texture atlas of a mesh (mesh_nerf --texture-res, mesh_render --appearance; DESIGN.md, "Texture atlas"): every face gets
 * the same right-triangle chart on a barycentric lattice, two charts tile one cell, the cells tile the image.  Every index
 * is a formula: no parametrisation, no packing, no compaction, and the bytes do not depend on the order of the workgroups.
 * Every fp32 operation is rounded on its own, division and square root correctly rounded, so a numpy restatement
 * (tests/mesh_texture.py) reproduces every output bit for bit.  THE RULE:
 *
 *   lattice    n in [1, 255] intervals per triangle side; T = (n + 1)(n + 2) / 2 samples per face: the lattice points (i, j)
 *              with i, j >= 0 and i + j <= n, at index j (n + 1) - j (j - 1) / 2 + i within the face (rows of constant j, i
 *              fastest); sample row of face f: f T + index.  Corner 0 of the face is lattice (0, 0), corner 1 is (n, 0),
 *              corner 2 is (0, n): the weights are b1 = (float) i / (float) n, b2 = (float) j / (float) n,
 *              b0 = (float)(n - i - j) / (float) n.
 *   cell       Cw = n + 3 texels wide, Ch = n + 2 high.  Cell c holds face 2c ("lower") and face 2c + 1 ("upper").  Local
 *              texel (a, b) belongs to the lower face when a + b <= n + 1, at lattice (a, b); otherwise to the upper face,
 *              at lattice (n + 2 - a, n + 1 - b).  In either face a lattice point with i + j == n + 1 is on that face's
 *              GUTTER diagonal.  2 T + 2 (n + 2) = Cw Ch: the two faces tile the cell and each owns its own gutter, which
 *              is why the cell is one texel wider than high.
 *   atlas      P = ceil(F / 2) cells; cols = the smallest integer >= 1 with cols Cw >= ceil(P / cols) Ch; rows =
 *              ceil(P / cols); W = cols Cw, H = rows Ch, so H <= W.  Cell c starts at x0 = (c mod cols) Cw,
 *              y0 = (c div cols) Ch; row 0 is the TOP row of the image.  Integer arithmetic only.  W > 16384 is refused.
 *   gutter     for lattice (i, j) with i + j == n + 1, per channel in fp32: i, j >= 1: (c(i-1, j) + c(i, j-1)) - c(i-1, j-1);
 *              i == 0: c(0, n); j == 0: c(n, 0).  A bilinear fetch inside a chart then equals linear interpolation on the
 *              lattice triangle up to the hypotenuse, before quantisation.
 *   empty      a texel of a face >= F (the upper face of the last cell when F is odd, the tail of the last row) is 0.
 *   quantise   u8 = (uint8)(min(max(c, 0), 1) * 255 + 0.5), a NaN -> 0.
 *   uv         per face corner, at the centre of the corner's texel (x, y): u = (float)(2x + 1) / (float)(2W),
 *              v = (float)(2(H - y) - 1) / (float)(2H): v points up, the OBJ convention.
 *   sample     position (b0 p0 + b1 p1) + b2 p2 per coordinate (nm_mesh_interpolate's order; a NaN is written as the
 *              canonical 0x7fc00000).  Direction: m = the same blend of the corner normals, L = sqrt((mx mx + my my) + mz mz);
 *              with L > 0 and finite, d = -(m / L).  Otherwise -- or without normals -- the sample is a FALLBACK sample:
 *              e1 = p1 - p0, e2 = p2 - p0, g = e1 x e2 (gx = e1y e2z - e1z e2y, and cyclic), G = sqrt((gx gx + gy gy) + gz gz);
 *              with G > 0 and finite, d = (g / G) * (float)(-flip), flip = +1 or -1 (marching cubes winds its triangles
 *              against its normals: -1); otherwise d = (0, 0, -1).  A face with an index outside [0, V) is never
 *              dereferenced: its rows are zeros, and its samples are counted under NM_MESH_TEXTURE_BAD_INDEX only.
 *   lookup     per pixel with face_id f in [0, F): uv = (b0 uv0 + b1 uv1) + b2 uv2 per component with uvk the rows of
 *              d_face_uv[f]; tx = u (float) Wt - 0.5, ty = (1 - v)(float) Ht - 0.5, each clamped: min(max(t, 0), side - 1)
 *              (clamp to edge); ix0 = floor(tx), ix1 = min(ix0 + 1, Wt - 1), fx = tx - (float) ix0, likewise in y; texel
 *              value (float) u8 / 255.0f; per channel top = c00 + fx (c10 - c00), bottom = c01 + fx (c11 - c01) with cXY the
 *              texel (ixX, iyY), out = top + fy (bottom - top).  d_background where f is not in [0, F) or u or v is not finite.
 *
 * nm_mesh_texture_layout (host code; no HIP call): h_layout[NM_MESH_TEXTURE_LAYOUT] = W, H, cols, rows, T.
 * nm_mesh_texture_samples: faces [first, first + count) -> d_positions, d_directions (count T, 3) fp32; d_normals (V,3) or
 *   NULL; d_counts[2] int64 on the DEVICE: the fallback samples and the samples of faces with a bad index, of this window.
 * nm_mesh_texture_fill: d_colors (F T, 3) fp32 -> d_atlas (H, W, 3) uint8.  nm_mesh_texture_uv -> d_face_uv (F, 3, 2) fp32.
 * nm_mesh_texture_lookup: ANY d_face_uv (F,3,2) and ANY d_texture (Ht, Wt, 3) uint8 with sides in [1, 16384], at the pixels of
 *   a nm_mesh_rasterize result -> d_out (pixels, 3) fp32.
 * One thread per output element, nothing allocates and nothing waits for the host: every entry can be captured into a graph.
 * F is in [0, 2^31 - 64), as is count T.  Argument errors -- a null array with a non-zero size, n outside [1, 255], a window
 * outside [0, F], flip not +-1, sizes out of range, W > 16384 -- return 2 before any HIP call.
 * nm_export_obj_textured (HOST arrays, as nm_export_obj, whose `v` and `vn` lines it writes byte for byte): `mtllib <mtllib>`,
 *   the v lines, the vn lines, 3F lines `vt u v` from h_face_uv (F,3,2) (numbers printed by the same rule), `usemtl <material>`,
 *   then `f a/t/a b/t/b c/t/c`, 1-based, t = 3f + k + 1.
 * ------------------------------------------------------------------------------------------ */
#define NM_MESH_TEXTURE_MAX_RES 255
#define NM_MESH_TEXTURE_MAX_SIDE 16384
#define NM_MESH_TEXTURE_W 0
#define NM_MESH_TEXTURE_H 1
#define NM_MESH_TEXTURE_COLS 2
#define NM_MESH_TEXTURE_ROWS 3
#define NM_MESH_TEXTURE_T 4
#define NM_MESH_TEXTURE_LAYOUT 5
#define NM_MESH_TEXTURE_FALLBACK 0
#define NM_MESH_TEXTURE_BAD_INDEX 1
#define NM_MESH_TEXTURE_COUNTS 2
int nm_mesh_texture_layout(int64_t num_faces, int32_t n, int64_t* h_layout);
int nm_mesh_texture_samples(const float* d_verts, int64_t num_vertices, const int32_t* d_faces, int64_t num_faces,
                            const float* d_normals, int32_t n, int32_t flip, int64_t first, int64_t count, float* d_positions,
                            float* d_directions, int64_t* d_counts, void* stream);
int nm_mesh_texture_fill(const float* d_colors, int64_t num_faces, int32_t n, uint8_t* d_atlas, void* stream);
int nm_mesh_texture_uv(int64_t num_faces, int32_t n, float* d_face_uv, void* stream);
int nm_mesh_texture_lookup(const int32_t* d_face_id, const float* d_bary, int64_t num_pixels, const float* d_face_uv,
                           int64_t num_faces, const uint8_t* d_texture, int32_t tex_height, int32_t tex_width,
                           const float* d_background, float* d_out, void* stream);
int nm_export_obj_textured(const float* h_vertices, int64_t num_vertices, const float* h_diffuse, int64_t num_diffuse,
                           const float* h_normals, int64_t num_normals, const int32_t* h_triangles, int64_t num_triangles,
                           const float* h_face_uv, const char* mtllib, const char* material, const char* path);

/* ------------------------------------------------------------------------------------------
 * Image SSIM (eval_nerf --ssim, mesh_render --ssim, mesh_nerf --render-ssim; DESIGN.md, "Image SSIM"): the structural
 * similarity of Wang et al. 2004 as scikit-image's structural_similarity(gaussian_weights=True, use_sample_covariance=False,
 * data_range=1) computes it on float images, as a closed rule that a numpy restatement (tests/image_ssim.py) reproduces bit
 * for bit -- the map, the sums and the mean.  THE RULE:
 *
 *   inputs     two fp32 images a, b of shape (H, W, C), row 0 on top, channels interleaved; 11 <= H, W <= 16384, 1 <= C <= 4.
 *              The data range is 1.0; nothing is clamped or quantised.
 *   arithmetic fp64 throughout, every product, sum and difference rounded on its own (no fused multiply-add), IEEE division.
 *   window     11 taps, sigma = 1.5, normalised -- these constants, not a call to exp:
 *                w[0] = w[10] = 0x1.0d956b52a1d6cp-10    w[1] = w[9] = 0x1.f1fe01ae5a5b8p-8    w[2] = w[8] = 0x1.26eb175d83f67p-5
 *                w[3] = w[7]  = 0x1.bff0fe8e98418p-4     w[4] = w[6] = 0x1.b43c3f52b19f2p-3    w[5]        = 0x1.106560aa892c0p-2
 *   fields     per channel five fields f in {x, y, x x, y y, x y} with x = (double) a, y = (double) b.
 *   filter     horizontal first, then vertical, over the valid positions only (no padding): the output is (H - 10, W - 10).
 *              h[r][c] = w[0] f[r][c], then + w[k] f[r][c + k] for k = 1..10 in ascending order; v[r][c] likewise over
 *              h[r + k][c].  This is scikit-image's own crop of the 5-pixel border.
 *   pixel      with the five filtered values ux, uy, uxx, uyy, uxy: vx = uxx - ux ux, vy = uyy - uy uy, vxy = uxy - ux uy,
 *              S = (((2 ux) uy + C1) (2 vxy + C2)) / (((ux ux + uy uy) + C1) ((vx + vy) + C2)),
 *              C1 = 0.01 * 0.01 and C2 = 0.03 * 0.03 as fp64 products.
 *   mean       per channel an int64 sum of llrint(S 2^32) (round half to even) over the finite S and an int64 count of the
 *              non-finite S, which are left out of the sum: integer addition does not depend on the order of the workgroups.
 *              ssim_c = sum_c / ((H - 10)(W - 10) 2^32), the correctly rounded quotient of the two integers; ssim = the mean
 *              of the ssim_c, added in channel order and divided by C, or NaN if any non-finite S was counted.  At 16384^2
 *              |sum_c| < 2^60; the fixed point moves the mean by at most 2^-33.  (|S| <= 1 up to rounding for every finite
 *              input whose squares stay far below fp64's range; the rounding of an |S| >= 2^31 is not defined.)
 *
 * d_map: NULL or (H - 10, W - 10, C) fp64, which receives S.  d_sums: (C, 2) int64 on the DEVICE, [c][NM_IMAGE_SSIM_SUM] and
 * [c][NM_IMAGE_SSIM_NONFINITE]; the call zeroes it on the stream in front of its one kernel.  Nothing allocates and nothing
 * waits for the host.  Argument errors -- a null d_a, d_b or d_sums, a side below 11 ("image must be at least 11x11") or above
 * 16384, channels outside [1, 4] -- return 2 before any HIP call.
 * ------------------------------------------------------------------------------------------ */
#define NM_IMAGE_SSIM_WINDOW 11
#define NM_IMAGE_SSIM_MAX_SIDE 16384
#define NM_IMAGE_SSIM_MAX_CHANNELS 4
#define NM_IMAGE_SSIM_SUM 0
#define NM_IMAGE_SSIM_NONFINITE 1
int nm_image_ssim(const float* d_a, const float* d_b, int32_t height, int32_t width, int32_t channels, double* d_map,
                  int64_t* d_sums, void* stream);

/* ------------------------------------------------------------------------------------------
 * TSDF fusion (mesh_nerf --geometry tsdf; DESIGN.md, "TSDF geometry"): depth maps rendered from V cameras are fused into a
 * truncated signed distance field on a range of the voxels of a grid, as a closed rule that a numpy restatement
 * (tests/tsdf_fuse.py) reproduces bit for bit -- the field, the observation counts and the three counters.  THE RULE:
 *
 *   inputs     V views (a HOST array of nm_view, 1 <= V <= NM_TSDF_MAX_VIEWS, all of one height H and width W in [1, 16384],
 *              use_ndc = 0, focal finite and > 0; R = c2w[:3,:3], c = c2w[:3,3]); depth (V,H,W) fp32: the depth of the surface
 *              every pixel sees, measured ALONG THE CAMERA'S AXIS (camera z), row 0 on top; opacity (V,H,W) fp32 or NULL; the
 *              three fp32 axes of the (n0,n1,n2) grid, as nm_mlp_grid_query takes them; the flat voxel range [first, first +
 *              count), last axis fastest; trunc > 0, near > 0, min_opacity.
 *   arithmetic fp64 throughout -- every fp32 input widened first --, every product, sum, difference and quotient rounded on
 *              its own (no fused multiply-add), IEEE division, in exactly the order written here.
 *   voxel      p = (ax0[i0], ax1[i1], ax2[i2]); sum = 0, n = 0, occluded = false; the views in index order:
 *   project    d = p - c;  cx = (R00 dx + R10 dy) + R20 dz, cy and cz likewise from columns 1 and 2 of R;  z = -cz.
 *              Unless z >= near the voxel is not in this view.
 *              col = rint((cx / z) focal + 0.5 W), row = rint(0.5 H - (cy / z) focal), rint rounding half to even: pixel i
 *              sits at u = i, get_ray_bundle's grid and the rasteriser's.  Unless 0 <= col <= W - 1 and 0 <= row <= H - 1
 *              the voxel is not in this view.
 *   hit        D = depth[v][row][col].  The ray is a hit iff D is finite and D > 0 and -- where there is an opacity map --
 *              opacity[v][row][col] >= min_opacity (a NaN opacity is a miss).
 *   observe    miss: t = -1 (the ray saw free space all the way).  hit: s = z - D; if s > trunc the voxel is occluded in this
 *              view (occluded = true) and there is no observation; otherwise t = max(-1, s / trunc).
 *              An observation does sum = sum + t, n = n + 1.
 *   field      inside-positive: phi = (float)(sum / (double) n) if n > 0; +1 if n == 0 and occluded (interior); -1 if n == 0
 *              and not occluded: the voxel was in no view's frustum and counts as empty.
 *   counters   int64: [NM_TSDF_OBSERVED] voxels with n > 0, [NM_TSDF_INTERIOR] n == 0 and occluded, [NM_TSDF_OUTSIDE] the
 *              rest; integer additions, so the order the workgroups run in shows in no output.
 *
 * d_field (count,) fp32; d_observations NULL or (count,) int32, which receives n; d_counts (3,) int64 on the DEVICE, zeroed by
 * the call on the stream.  d_workspace: nm_tsdf_workspace_bytes(V, H, W) bytes (0 for sizes the entry refuses): the view table
 * and the merged hit-depth map.  The views are read before the call returns.  Nothing allocates and nothing waits for the
 * host.  Argument errors -- a null pointer, V outside [1, 1024], views of unequal size or with use_ndc, a focal, trunc or near
 * that is not finite and > 0, a NaN min_opacity, a voxel range outside the grid -- return 2 before any HIP call.
 * ------------------------------------------------------------------------------------------ */
#define NM_TSDF_MAX_VIEWS 1024
#define NM_TSDF_OBSERVED 0
#define NM_TSDF_INTERIOR 1
#define NM_TSDF_OUTSIDE 2
int64_t nm_tsdf_workspace_bytes(int64_t num_views, int32_t height, int32_t width);
int nm_tsdf_integrate(const nm_view* views, int64_t num_views, const float* d_depth, const float* d_opacity, const float* d_ax0,
                      const float* d_ax1, const float* d_ax2, int32_t n0, int32_t n1, int32_t n2, int64_t first, int64_t count,
                      double trunc, double near, double min_opacity, void* d_workspace, float* d_field, int32_t* d_observations,
                      int64_t* d_counts, void* stream);

/* PLY export of a point cloud (HOST arrays): element vertex with x y z nx ny nz as float and red green blue as uchar, the
 * property names of the reference's export_ply (src/mesh_surface_ray.py:46-58).  binary = 0: "format ascii 1.0", one vertex
 * per line, floats printed as nm_export_obj prints them (they read back to the same fp32); binary != 0:
 * "format binary_little_endian 1.0", 27 bytes per vertex.  Returns 2 for a null array with n > 0, 6 if the file cannot be
 * opened or written. */
int nm_export_ply(const float* h_points, const float* h_normals, const uint8_t* h_colors_u8, int64_t n, int binary,
                  const char* path);

#ifdef __cplusplus
}
#endif
#endif /* NERFMESHES_HIP_H */
