"""Bit-exact record of the ray operators' outputs (nerfmeshes_amd/csrc/ray_ops.hip), shared by tests/tools/record_composite_bits.py
(writes tests/golden/composite_bits.json) and tests/test_gpu_ray_ops_bits.py (recomputes and compares).

The compositing kernels are deterministic -- one wave per ray, a fixed shuffle order, no atomics --, so a change of ray_ops.hip
that is meant to keep the arithmetic reproduces every output bit.  Per case of composite_cases.CASES the record holds the sha256
of the raw bytes (on the CPU, contiguous) of

    train_forward   train_ops.composite under no_grad with the case's noise: the six bundle fields
    eval_forward    hip_ops.composite with the case's white background: the same six
    radiance_grad   the gradient as tests/test_gpu_ray_ops.py::_gpu_backward forms it (upstream gradients a case leaves out: absent)

and, for the ray generators, of hip_ops.ray_bundle on a 7 x 5 image (whole, and first=3 count=29), hip_ops.ndc_rays on those
rays and hip_ops.view_rays with ndc_near set on the same view."""
import hashlib
import json
import os

import numpy as np
import torch

from tests import composite_cases as CC

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composite_bits.json")
FIELDS = ("weights", "mask_weights", "rgb_map", "acc_map", "depth_map", "disp_map")
HEIGHT, WIDTH, FOCAL, NDC_NEAR = 7, 5, 6.25, 1.0


def pose():
    """A forward-facing camera (so that ndc_rays divides by nothing near 0), rotated about all three axes, off the origin."""
    a, b, c = 0.31, -0.17, 0.23
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    out = np.eye(4)
    out[:3, :3] = rz @ ry @ rx
    out[:3, 3] = (0.3, -0.2, 4.0)
    return out.astype(np.float32)


def sha(x):
    return hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def composite_entry(hip_ops, train_ops, case):
    from tests.test_gpu_ray_ops import _gpu_backward
    samples, white, _, _ = case
    ref = CC.reference(case)
    rad, t, dirs = ref["rad"].cuda(), ref["t"].cuda(), ref["dirs"].cuda()
    noise = None if ref["noise"] is None else ref["noise"].cuda()
    with torch.no_grad():
        train = train_ops.composite(rad, t, dirs, noise, CC.render_spec(samples, white).attenuation_threshold, white)
        evald = hip_ops.composite(rad, t, dirs, white_background=white)
    _, grad = _gpu_backward(train_ops, ref, case)
    return {"train_forward": {k: sha(train[k]) for k in FIELDS}, "eval_forward": {k: sha(evald[k]) for k in FIELDS},
            "radiance_grad": sha(grad)}


def ray_entries(hip_ops):
    p = pose()
    origin, dirs = hip_ops.ray_bundle(p, HEIGHT, WIDTH, FOCAL)
    _, part = hip_ops.ray_bundle(p, HEIGHT, WIDTH, FOCAL, first=3, count=29)
    ndc_o, ndc_d = hip_ops.ndc_rays(HEIGHT, WIDTH, FOCAL, NDC_NEAR, origin, dirs)
    view_o, view_d = hip_ops.view_rays(hip_ops.make_view(p, HEIGHT, WIDTH, FOCAL, ndc_near=NDC_NEAR))
    return {"ray_bundle": {"origin": sha(origin), "dirs": sha(dirs)}, "ray_bundle_first3_count29": {"dirs": sha(part)},
            "ndc_rays": {"origins": sha(ndc_o), "dirs": sha(ndc_d)}, "view_rays_ndc": {"origins": sha(view_o), "dirs": sha(view_d)}}


def recorded():
    with open(PATH) as fh:
        return json.load(fh)
