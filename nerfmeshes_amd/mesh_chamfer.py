"""Chamfer distance between two triangle meshes on the MI355X (addition: the reference's only mesh-quality measure, the
chamfer branch of `validation_epoch_end`, src/models/model_base.py:82-102, is dead code there and needs pytorch3d).

    python -m nerfmeshes_amd.mesh_chamfer --mesh A.obj --target B.obj [--samples 100000] [--seed 0] [--normalize] [--out FILE.json]
                                          [--surface sampled|exact] [--fscore T1,T2,...]

`--samples` points are drawn uniformly over the surface of each mesh (hip_ops.mesh_sample_points: integer area weights,
pytorch3d's barycentric rule) from ONE device generator seeded with `--seed`, mesh A first; every point's exact nearest
neighbour in the other cloud comes from the brute-force kernel (hip_ops.points_nearest).  Reported: `chamfer` = `x_to_y` +
`y_to_x`, the two means of SQUARED distances (pytorch3d's `chamfer_distance` defaults), their square roots `rms_x_to_y` /
`rms_y_to_x`, the sample count, and V / F / total area of both meshes.  `--normalize` first applies `create_mesh`'s rule to each
mesh on its own (subtract the vertex mean, divide by the largest absolute coordinate); without it both meshes are compared
in the frame they come in.

`--surface exact` measures every sample against the other mesh's TRIANGLES instead of against its samples
(hip_ops.mesh_surface_distance: the same draws, no noise floor from the second sampling): the numbers above then come from
exact distances, and the report gains `surface`, `accuracy` / `completeness` (mean unsquared distance each way), the Hausdorff
maxima and the normal consistency (mean |cos| between a sample's face normal and the normal of the face nearest to it).
`--fscore T1,T2,...` (with `--surface exact`) adds precision / recall / F-score at each distance threshold, in the frame the
meshes are compared in.  Without either option the report and the printed lines are what they were before the options existed.
"""
import argparse
import json
import math

import torch

from . import hip_ops

KEYS = ("chamfer", "x_to_y", "y_to_x", "rms_x_to_y", "rms_y_to_x")
SURFACES = ("sampled", "exact")
EXACT_KEYS = ("accuracy", "completeness", "hausdorff_x_to_y", "hausdorff_y_to_x", "hausdorff", "normal_consistency_x_to_y",
              "normal_consistency_y_to_x", "normal_consistency", "normal_pairs_x_to_y", "normal_pairs_y_to_x")


def parse_thresholds(text):
    """`T1,T2,...` -> tuple of floats, each finite and > 0 (ValueError otherwise); None or "" -> ()"""
    if text is None or isinstance(text, (tuple, list)):
        values = tuple(float(t) for t in (text or ()))
    else:
        try:
            values = tuple(float(t) for t in str(text).split(",") if t.strip())
        except ValueError:
            raise ValueError(f"thresholds must be numbers separated by commas, got {text!r}") from None
    if any(not (0.0 < t < float("inf")) for t in values):
        raise ValueError(f"thresholds must be finite and > 0, got {text!r}")
    return values


def check_surface(surface, fscore):
    """the two options together -> the thresholds as floats; ValueError for a combination that is refused"""
    if surface not in SURFACES:
        raise ValueError(f"the surface must be one of {', '.join(SURFACES)}, got {surface!r}")
    fscore = parse_thresholds(fscore)
    if fscore and surface != "exact":
        raise ValueError("F-score thresholds need the exact surface distance (--surface exact): a distance between two samplings "
                         "has a noise floor that moves with the sample count")
    return fscore


def compare_meshes(verts_a, faces_a, verts_b, faces_b, samples=100000, seed=0, normalize=False, device=None, surface="sampled",
                   fscore=()):
    """The numbers of the CLI for two meshes given as arrays (host or device) -> dict of Python numbers.  Under
    torch.distributed every rank must call it with the same meshes: the draws are the same on every rank, the searches are
    shared out (hip_ops.chamfer_distance, hip_ops.mesh_surface_distance) and every rank returns the single-rank numbers bit
    for bit.  `surface="exact"`: point-to-triangle distances, the additional keys of EXACT_KEYS and `surface`; `fscore`:
    thresholds, one dict(threshold, precision, recall, fscore) each under `fscore`."""
    from .mesh_nerf import normalize_vertices
    fscore = check_surface(surface, fscore)
    samples = int(samples)
    if samples < 1:
        raise ValueError(f"the number of samples must be >= 1, got {samples}")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    clouds, meshes, info = [], [], {}
    for name, verts, faces in (("mesh", verts_a, faces_a), ("target", verts_b, faces_b)):
        verts = torch.as_tensor(verts).to(device=device, dtype=torch.float32)
        faces = torch.as_tensor(faces).to(device=device, dtype=torch.int32)
        if normalize:
            verts = normalize_vertices(verts)
        areas, _ = hip_ops.mesh_face_weights(verts, faces)
        if surface == "sampled":
            points, _ = hip_ops.mesh_sample_points(verts, faces, n=samples, generator=gen)
            clouds.append(points)
        meshes += [verts, faces]
        info[name] = dict(vertices=int(verts.shape[0]), faces=int(faces.shape[0]), area=float(areas.double().sum().item()))
    if surface == "sampled":
        res = hip_ops.chamfer_distance(clouds[0], clouds[1])
    else:                                                  # the same draws from the same generator, mesh A first
        res = hip_ops.mesh_surface_distance(*meshes, n=samples, generator=gen, thresholds=fscore)
    out = dict(chamfer=res["chamfer"], x_to_y=res["x_to_y"], y_to_x=res["y_to_x"], rms_x_to_y=math.sqrt(res["x_to_y"]),
               rms_y_to_x=math.sqrt(res["y_to_x"]), samples=samples, seed=int(seed), normalize=bool(normalize))
    out.update(info)
    if surface == "exact":
        out["surface"] = surface
        out.update({k: res[k] for k in EXACT_KEYS})
        if fscore:
            out["fscore"] = res["fscore"]
    return out


def format_report(report):
    """The lines both CLIs print."""
    lines = [f"Chamfer distance over {report['samples']} samples per mesh (seed {report['seed']}"
             f"{', normalized' if report['normalize'] else ''}): {report['chamfer']}"]
    lines.append(f"  mesh -> target: mean squared distance {report['x_to_y']}, rms {report['rms_x_to_y']}")
    lines.append(f"  target -> mesh: mean squared distance {report['y_to_x']}, rms {report['rms_y_to_x']}")
    for name in ("mesh", "target"):
        m = report[name]
        lines.append(f"  {name}: {m['vertices']} vertices, {m['faces']} faces, area {m['area']}")
    if report.get("surface", "sampled") == "exact":
        lines.append(f"Exact distance to the other mesh's triangles: accuracy (mesh -> target) {report['accuracy']}, "
                     f"completeness (target -> mesh) {report['completeness']}")
        lines.append(f"  Hausdorff {report['hausdorff']}: mesh -> target {report['hausdorff_x_to_y']}, "
                     f"target -> mesh {report['hausdorff_y_to_x']}")
        lines.append(f"Normal consistency {report['normal_consistency']}: mean |cos| between a sample's normal and the nearest "
                     "face's")
        lines.append(f"  mesh -> target {report['normal_consistency_x_to_y']} over {report['normal_pairs_x_to_y']} pairs, "
                     f"target -> mesh {report['normal_consistency_y_to_x']} over {report['normal_pairs_y_to_x']} pairs")
        for row in report.get("fscore", ()):
            lines.append(f"F-score at {row['threshold']}: {row['fscore']} (precision {row['precision']}, recall {row['recall']})")
    return lines


def write_report(report, path):
    with open(path, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


def build_parser():
    p = argparse.ArgumentParser(description="Chamfer distance between two OBJ meshes, sampled and searched on the GPU")
    p.add_argument("--mesh", type=str, required=True, help="the mesh to judge (OBJ)")
    p.add_argument("--target", type=str, required=True, help="the mesh to compare it with (OBJ)")
    p.add_argument("--samples", type=int, default=100000, help="points sampled on each mesh")
    p.add_argument("--seed", type=int, default=0, help="seed of the one device generator both meshes draw from (--mesh first)")
    p.add_argument("--normalize", action="store_true", default=False,
                   help="centre each mesh on its vertex mean and scale it by its largest absolute coordinate first "
                        "(mesh_nerf.create_mesh's rule); default: both meshes in the frame they come in")
    p.add_argument("--out", type=str, default=None, help="also write the numbers to this JSON file")
    p.add_argument("--surface", choices=SURFACES, default="sampled",
                   help="sampled: every sample against the other mesh's samples (default); exact: against the other mesh's "
                        "triangles, which adds accuracy / completeness, Hausdorff and normal consistency to the report")
    p.add_argument("--fscore", type=str, default=None, metavar="T1,T2,...",
                   help="distance thresholds (in the frame the meshes are compared in) for precision / recall / F-score; "
                        "needs --surface exact")
    return p


def main(argv=None):
    from .nerf.nerf_helpers import load_obj
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        fscore = check_surface(args.surface, args.fscore)
    except ValueError as e:
        parser.error(f"--fscore: {e}")
    if not torch.cuda.is_available():
        raise SystemExit("mesh_chamfer needs a MI355X: the HIP path has no CPU fallback")
    (va, fa), (vb, fb) = load_obj(args.mesh), load_obj(args.target)
    report = compare_meshes(va, fa, vb, fb, samples=args.samples, seed=args.seed, normalize=args.normalize,
                            surface=args.surface, fscore=fscore)
    report["mesh"]["path"], report["target"]["path"] = args.mesh, args.target
    for line in format_report(report):
        print(line)
    if args.out:
        write_report(report, args.out)
        print(f"Chamfer report saved to {args.out}")
    return report


if __name__ == "__main__":
    main()
