"""The compositing kernels of ray_ops.hip (nm_composite / nm_composite_train and nm_composite_backward) on the shapes the project
ships -- 65 536 rays of 64 and of 192 samples (a render chunk: the evaluation forward), 2 048 rays of 128 and of 192 samples (a
training batch: the training forward with noise) -- and on one long case, 4 096 rays of 1 025 samples.  Forward and backward
(all four upstream gradients) of every shape, called through the C ABI on preallocated buffers: 20 warm-up calls, then 40
windows of 50 back-to-back calls under HIP events; a window's figure is its time per call and the shape's the median window.
The small shapes move a few MB per call: their figure is the launch rate of the queue as much as the kernel.

With --against OTHER_LIB the tool times nothing itself: it starts itself --runs times per library, in fresh processes and
alternating OTHER_LIB (the parent commit's build) with the tree's own, and reports per shape every run's median, the parent's
run-to-run spread (largest minus smallest run median) and whether the median of the tree's run medians lies within that spread
of the parent's.

    python tests/tools/time_composite.py [--lib PATH]
    python tests/tools/time_composite.py --against PARENT_LIB [--runs 5] [--out profiles/r14_composite_refactor.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# (rays, samples, training)
SHAPES = ((65536, 64, False), (65536, 192, False), (2048, 128, True), (2048, 192, True), (4096, 1025, True))
WARMUP, WINDOWS, CALLS = 20, 40, 50


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(lib_path):
    import torch
    from nerfmeshes_amd import _lib
    if lib_path:
        _lib.LIB_PATH = os.path.abspath(lib_path)
    from nerfmeshes_amd import hip_ops
    from nerfmeshes_amd.hip_ops import _ptr, _stream
    lib = _lib.load()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "lib": _lib.LIB_PATH, "shapes": {}}

    def per_call_ms(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        windows = []
        for _ in range(WINDOWS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            torch.cuda.synchronize()
            windows.append(a.elapsed_time(b) / CALLS)
        return {"median_ms": median(windows), "min_ms": min(windows), "max_ms": max(windows)}

    for rays, samples, training in SHAPES:
        g = torch.Generator().manual_seed(samples)
        t = torch.sort(2.0 + 4.0 * torch.rand(rays, samples, generator=g), dim=-1).values.to(dev)
        rad = torch.cat((torch.rand(rays, samples, 3, generator=g), 3.0 * torch.randn(rays, samples, 1, generator=g)), -1).contiguous().to(dev)
        dirs = torch.nn.functional.normalize(torch.randn(rays, 3, generator=g), dim=-1).to(dev)
        noise = torch.randn(rays, samples, generator=g).to(dev) if training else None
        tensors, bundle = hip_ops._alloc_bundle(rays, samples, dev)
        G = [torch.randn(rays, 3, device=dev), torch.randn(rays, device=dev), torch.randn(rays, device=dev), torch.randn(rays, samples, device=dev)]
        grads = _lib.BundleGrads(*[_ptr(x) for x in G])
        grad_rad = torch.empty_like(rad)
        stream = _stream()

        def forward():
            if training:
                rc = lib.nm_composite_train(_ptr(rad), _ptr(t), _ptr(dirs), _ptr(noise), rays, samples, 1e-5, 0, C.byref(bundle), stream)
            else:
                rc = lib.nm_composite(_ptr(rad), _ptr(t), _ptr(dirs), rays, samples, 1e-5, 0, 0, C.byref(bundle), stream)
            _lib.check(rc, "composite forward")

        def backward():
            _lib.check(lib.nm_composite_backward(_ptr(rad), _ptr(t), _ptr(dirs), _ptr(noise), rays, samples, 0, C.byref(grads), _ptr(grad_rad),
                                                 stream), "nm_composite_backward")

        row = {"forward": per_call_ms(forward), "backward": per_call_ms(backward)}
        out["shapes"][f"{rays}x{samples}" + ("_train" if training else "_eval")] = row
        del tensors
    return out


def compare(opt):
    own = os.path.join(ROOT, "nerfmeshes_amd", "csrc", "libnerfmeshes_hip.so")
    runs = {"parent": [], "tree": []}
    for _ in range(opt.runs):
        for name, path in (("parent", opt.against), ("tree", own)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", path], check=True, capture_output=True, text=True, timeout=600)
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(name, json.dumps({k: {d: round(v[d]["median_ms"], 5) for d in v} for k, v in runs[name][-1]["shapes"].items()}), flush=True)
    out = {"device": runs["tree"][0]["device"], "method": f"{WARMUP} warm-up calls, {WINDOWS} windows of {CALLS} calls under HIP events, median window per run; "
           f"{opt.runs} fresh processes per library, alternating", "shapes": {}, "all_within_parent_spread": True}
    for shape in runs["tree"][0]["shapes"]:
        for direction in ("forward", "backward"):
            pm = [r["shapes"][shape][direction]["median_ms"] for r in runs["parent"]]
            tm = [r["shapes"][shape][direction]["median_ms"] for r in runs["tree"]]
            spread = max(pm) - min(pm)
            ok = median(tm) <= median(pm) + spread
            out["shapes"][f"{shape} {direction}"] = {"parent_run_medians_ms": pm, "tree_run_medians_ms": tm, "parent_median_ms": median(pm),
                                                     "tree_median_ms": median(tm), "parent_run_to_run_spread_ms": spread,
                                                     "tree_within_parent_spread": ok}
            out["all_within_parent_spread"] &= ok
    print(json.dumps(out), flush=True)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="time this build of libnerfmeshes_hip.so, not the tree's")
    ap.add_argument("--against", default=None, help="the parent commit's libnerfmeshes_hip.so: compare the tree's build with it")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    if opt.against:
        compare(opt)
    else:
        print(json.dumps(measure(opt.lib)), flush=True)


if __name__ == "__main__":
    main()
