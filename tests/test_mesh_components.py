"""CPU: the mesh-component filter's host side -- the numpy restatement (tests/mesh_components.py) against
scipy.sparse.csgraph on every mesh of the marching-cubes fixture, the tie rule and the compaction on it, mesh_nerf's two
options (defaults, negatives, the --route script rejection) and the argument checks of the four C entries."""
import ctypes as C

import numpy as np
import pytest

from tests import mesh_components as MC
from tests.helpers import load_golden


@pytest.fixture(scope="module")
def meshes():
    g = load_golden("mc_cases")
    out = []
    for i in range(int(g["count"])):
        if f"err_{i}" in g.files:
            continue
        out.append((i, g[f"verts_{i}"], g[f"faces_{i}"].astype(np.int32), g[f"normals_{i}"], g[f"values_{i}"]))
    return out


@pytest.fixture(scope="module")
def labelled(meshes):
    return [(i, v, f) + MC.components(f, len(v)) for i, v, f, _, _ in meshes]


def test_fixture_is_what_the_filter_was_designed_on(meshes, labelled):
    assert len(meshes) == 667
    multi = tied = most = 0
    for _, v, f, lab, counts in labelled:
        assert len(f) > 0 and np.array_equal(np.unique(f), np.arange(len(v))), "no unreferenced vertex"
        sizes = counts[lab == np.arange(len(v))]
        multi += len(sizes) > 1
        tied += int((sizes == sizes.max()).sum() > 1)
        most = max(most, len(sizes))
    assert (multi, tied, most) == (272, 104, 16)


def _sequential_components(faces, num_vertices):
    """scipy's answer where scipy is not installed: a plain sequential union-find -> (count, labels in its own numbering)"""
    parent = list(range(num_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(faces).tolist():
        for u, w in ((a, b), (b, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)
    roots = np.array([find(x) for x in range(num_vertices)])
    return len(np.unique(roots)), np.unique(roots, return_inverse=True)[1]


def test_restatement_matches_scipy_on_every_fixture_mesh(labelled):
    reference = MC.scipy_components if MC.scipy_components(np.zeros((0, 3), np.int32), 1) is not None else _sequential_components
    for i, v, f, lab, counts in labelled:
        n, other = reference(f, len(v))
        roots = np.flatnonzero(lab == np.arange(len(v)))
        assert len(roots) == n, i
        assert np.array_equal(MC.canonical(other, len(v)), lab), f"mesh {i}: another partition, or a label that is not the minimum"
        assert int(counts.sum()) == len(f) and not counts[lab != np.arange(len(v))].any()
        for r in roots:                                           # size = triangles whose vertices all carry the label
            assert counts[r] == int((lab[f] == r).all(axis=1).sum())


def test_labels_on_hand_made_meshes():
    # two triangles sharing an edge, one sharing only a vertex with them, one apart, vertices 9 and 11 in no triangle
    f = np.array([[7, 3, 5], [5, 3, 8], [8, 10, 12], [1, 2, 6]], np.int32)
    lab, counts = MC.components(f, 13)
    assert lab.tolist() == [0, 1, 1, 3, 4, 3, 1, 3, 3, 9, 3, 11, 3]
    assert counts.tolist() == [0, 1, 0, 3] + [0] * 9
    # a long strip numbered against the propagation direction
    n = 2000
    strip = np.stack((np.arange(n - 2), np.arange(1, n - 1), np.arange(2, n)), 1)
    perm = np.random.default_rng(0).permutation(n)
    lab, counts = MC.components(perm[strip], n)
    assert not lab.any() and counts[0] == n - 2 and counts.sum() == n - 2
    assert MC.components(np.zeros((0, 3), np.int32), 4)[0].tolist() == [0, 1, 2, 3]


def test_selection_rules():
    f = np.array([[0, 1, 2], [3, 4, 5], [4, 5, 6], [7, 8, 9], [8, 9, 10], [11, 12, 13], [12, 13, 14], [13, 14, 15]], np.int32)
    lab, counts = MC.components(f, 17)                            # sizes: 0 -> 1, 3 -> 2, 7 -> 2, 11 -> 3, 16 -> 0
    roots = lambda **kw: np.flatnonzero(MC.select(lab, counts, **kw)).tolist()   # noqa: E731
    assert roots() == [0, 3, 7, 11, 16]
    assert roots(min_faces=1) == [0, 3, 7, 11] and roots(min_faces=2) == [3, 7, 11] and roots(min_faces=4) == []
    assert roots(keep_largest=1) == [11] and roots(keep_largest=2) == [3, 11], "the tie between 3 and 7 goes to the smaller label"
    assert roots(keep_largest=3) == [3, 7, 11] and roots(keep_largest=9) == [0, 3, 7, 11, 16]
    assert roots(min_faces=3, keep_largest=2) == [11], "fewer than K survive: all of them stay"
    v = np.arange(17 * 3, dtype=np.float32).reshape(17, 3)
    ov, of, on, oval, okeys, info = MC.filter_components(v, f, -v, v[:, 0], np.arange(17) * 10, min_faces=2, keep_largest=2)
    assert of.tolist() == [[0, 1, 2], [1, 2, 3], [4, 5, 6], [5, 6, 7], [6, 7, 8]]
    assert np.array_equal(ov, v[[3, 4, 5, 6, 11, 12, 13, 14, 15]]) and np.array_equal(on, -ov) and np.array_equal(oval, ov[:, 0])
    assert okeys.tolist() == [30, 40, 50, 60, 110, 120, 130, 140, 150]
    assert info == dict(components=5, components_kept=2, faces=8, faces_kept=5, vertices=17, vertices_kept=9)
    none = MC.filter_components(v, f, -v, min_faces=4)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3) and none[3] is None and none[5]["components_kept"] == 0


def test_tie_rule_on_the_fixture(meshes, labelled):
    tied = 0
    for (i, v, f, nrm, val), (_, _, _, lab, counts) in zip(meshes, labelled):
        roots = np.flatnonzero(lab == np.arange(len(v)))
        sizes = counts[roots]
        if (sizes == sizes.max()).sum() < 2:
            continue
        tied += 1
        winner = int(roots[sizes == sizes.max()].min())
        ov, of, on, oval, _, info = MC.filter_components(v, f, nrm, val, keep_largest=1)
        keep_v = lab == winner
        assert info["components_kept"] == 1 and info["faces_kept"] == int(sizes.max()) and info["vertices_kept"] == int(keep_v.sum())
        assert np.array_equal(ov, v[keep_v]) and np.array_equal(on, nrm[keep_v]) and np.array_equal(oval, val[keep_v])
        # the kept triangles are the winner's, in their order, over the same points
        assert np.array_equal(ov[of], v[f[keep_v[f[:, 0]]]])
    assert tied == 104


def test_parser_defaults_and_negatives():
    from nerfmeshes_amd import mesh_nerf
    p = mesh_nerf.build_parser()
    a = p.parse_args([])
    assert (a.min_component_faces, a.keep_largest) == (0, 0)
    a = p.parse_args(["--min-component-faces", "50", "--keep-largest", "3"])
    assert (a.min_component_faces, a.keep_largest) == (50, 3)
    for bad in (["--min-component-faces", "-1"], ["--keep-largest", "-2"], ["--keep-largest", "1.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


@pytest.mark.parametrize("option", [["--min-component-faces", "4"], ["--keep-largest", "1"]])
def test_route_script_rejects_the_filter(tmp_path, option):
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args([*option, "--route", "script", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="route script"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert not any(tmp_path.iterdir()), "rejected before anything is written"


def test_keep_largest_over_the_cap_is_rejected_before_anything_runs(tmp_path):
    from nerfmeshes_amd import hip_ops, mesh_nerf
    args = mesh_nerf.build_parser().parse_args(["--keep-largest", str(hip_ops.KEEP_LARGEST_MAX + 1), "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError, match="keep-largest"):
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert not any(tmp_path.iterdir())


NO_STEP = "no --route script: the reference's script has no such step"
SMOOTH_OPTIONS = "--smooth-iters / --smooth-lambda / --smooth-mu / --smooth-boundary have " + NO_STEP
CULL_OPTIONS = "--cull-hidden-views / --cull-size / --cull-rings / --cull-radius have " + NO_STEP


# one option per record of mesh_nerf.FEATURES, and the two of the hidden-face filter that no other test sets on their own
@pytest.mark.parametrize("option, text", [
    (["--normals", "network"], "--normals network has no --route script: the reference's script only has the grid's normals"),
    (["--keep-largest", "1"], "--min-component-faces / --keep-largest have " + NO_STEP),
    (["--cull-hidden-views", "2"], CULL_OPTIONS), (["--cull-size", "512"], CULL_OPTIONS), (["--cull-radius", "2.5"], CULL_OPTIONS),
    (["--smooth-mu", "-0.4"], SMOOTH_OPTIONS),
    (["--simplify-cell", "2"], "--simplify-cell has " + NO_STEP),
    (["--target-mesh", "t.obj"], "--target-mesh has " + NO_STEP),
    (["--render-views", "2"], "--render-views has " + NO_STEP),
    (["--texture-res", "4"], "--texture-res has " + NO_STEP)], ids=lambda x: x[0] if isinstance(x, list) else None)
def test_route_script_rejects_every_feature_in_its_own_words(tmp_path, option, text):
    from nerfmeshes_amd import mesh_nerf
    args = mesh_nerf.build_parser().parse_args([*option, "--route", "script", "--save-dir", str(tmp_path)])
    with pytest.raises(ValueError) as e:
        mesh_nerf.export_marching_cubes(None, args, None, "cpu")
    assert str(e.value) == text
    assert not any(tmp_path.iterdir()), "rejected before anything is written"


def test_a_namespace_without_the_newer_options_passes_the_checks():
    import argparse
    from nerfmeshes_amd import mesh_nerf
    assert mesh_nerf.check_features(argparse.Namespace()) == set()
    assert mesh_nerf.check_features(argparse.Namespace(route="script", min_component_faces=0)) == set()
    assert mesh_nerf.check_features(argparse.Namespace(simplify_cell=2.0, normals="network")) == {"simplify", "normals"}
    # smoothing's other options do not switch it on, but they are checked
    assert mesh_nerf.check_features(argparse.Namespace(smooth_lambda=0.4)) == set()
    with pytest.raises(ValueError, match="--smooth-lambda in"):
        mesh_nerf.check_features(argparse.Namespace(smooth_lambda=1.5))


@pytest.mark.parametrize("options, expected", [
    (["--min-component-faces", "4", "--cull-hidden-views", "2", "--smooth-iters", "3", "--simplify-cell", "2"],
     ["filter_components", "cull_hidden", "smooth_mesh", "simplify_mesh"]),
    (["--simplify-cell", "2", "--keep-largest", "1", "--smooth-lambda", "0.4", "--cull-rings", "2"],
     ["filter_components", "simplify_mesh"]),
    ([], [])], ids=["all four", "two", "none"])
def test_postprocess_runs_the_enabled_stages_in_order(monkeypatch, options, expected):
    """the stubs are set on the module: postprocess must look the stage functions up when it calls them, as the timing tools
    replace them the same way"""
    from nerfmeshes_amd import mesh_nerf
    calls = []

    def stub(name):
        def record(vertices, triangles, normals, *rest):
            calls.append((name, vertices, rest))
            return vertices + 1, triangles, normals
        return record

    for name in ("filter_components", "cull_hidden", "smooth_mesh", "simplify_mesh"):
        monkeypatch.setattr(mesh_nerf, name, stub(name))
    args = mesh_nerf.build_parser().parse_args(options)
    assert mesh_nerf.postprocess(0, "t", "n", args) == (len(expected), "t", "n")
    assert [c[0] for c in calls] == expected
    assert [c[1] for c in calls] == list(range(len(expected))), "each stage gets what the one before returned"
    for name, _, rest in calls:               # the signatures the stage functions have
        assert rest == {"filter_components": (args.min_component_faces, args.keep_largest), "cull_hidden": (args,),
                        "smooth_mesh": (args,), "simplify_mesh": (args.simplify_cell, args)}[name]


def test_argument_errors_without_a_gpu():
    from nerfmeshes_amd import _lib, hip_ops
    lib = _lib.load()
    null, one = C.c_void_p(None), C.c_void_p(256)           # never dereferenced: validation fails first
    out = [C.c_int64(-7) for _ in range(4)]
    refs = [C.byref(o) for o in out]

    def err():
        return (lib.nm_last_error() or b"").decode()

    def label(f=one, nf=10, nv=20, lab=one, cnt=one, ws=one):
        return lib.nm_mesh_components(f, nf, nv, lab, cnt, ws, null)

    def select(f=one, nf=10, nv=20, lab=one, cnt=one, mn=0, k=0, ws=one, refs=refs):
        return lib.nm_mesh_components_select(f, nf, nv, lab, cnt, mn, k, ws, *refs, null)

    def compact(ws=one, f=one, nf=10, nv=20, v=one, n=one, val=null, keys=null, kv=5, kf=5, ov=one, of=one, on=one, oval=null,
                okeys=null):
        return lib.nm_mesh_components_compact(ws, f, nf, nv, v, n, val, keys, kv, kf, ov, of, on, oval, okeys, null)

    for kw in (dict(f=null), dict(lab=null), dict(cnt=null), dict(ws=null)):
        assert label(**kw) == 2 and "bad argument" in err(), kw
        assert select(**kw) == 2 and "bad argument" in err(), kw
    assert select(refs=[refs[0], None, refs[2], refs[3]]) == 2 and "bad argument" in err()
    for kw in (dict(nf=-1), dict(nv=-1), dict(nv=1 << 31), dict(nf=1 << 31)):
        assert label(**kw) == 2 and "2^31" in err(), kw
        assert select(**kw) == 2 and "2^31" in err(), kw
        assert compact(**kw) == 2 and "2^31" in err(), kw
    for fn in (label, select, compact):
        assert fn(nf=3, nv=0) == 2 and "faces without vertices" in err()
    assert select(mn=-1) == 2 and "min_faces" in err()
    assert select(k=-1) == 2 and "keep_largest" in err()
    assert select(k=hip_ops.KEEP_LARGEST_MAX + 1) == 2 and "keep_largest must be in [0, 1024]" in err()
    assert [o.value for o in out] == [-7] * 4, "nothing is returned by a rejected call"
    for kw in (dict(ws=null), dict(f=null)):
        assert compact(**kw) == 2 and "bad argument" in err(), kw
    assert compact(kv=21) == 2 and "kept counts" in err()
    assert compact(kf=11) == 2 and "kept counts" in err()
    assert compact(kv=-1) == 2 and compact(kf=-1) == 2
    assert compact(ov=null) == 2 and "without its output" in err()
    assert compact(val=one) == 2 and "without its output" in err()
    assert compact(keys=one) == 2 and "without its output" in err()
    assert compact(of=null) == 2 and "null face output" in err()
    # the workspace: the parents, one keep bit and a third of a prefix byte per vertex and face, the round maxima
    assert lib.nm_mesh_components_workspace_bytes(-1, 0) == 0 and lib.nm_mesh_components_workspace_bytes(0, -1) == 0
    assert lib.nm_mesh_components_workspace_bytes(1 << 31, 0) == 0
    assert lib.nm_mesh_components_workspace_bytes(0, 0) >= 8 * (hip_ops.KEEP_LARGEST_MAX + 1)
    big = lib.nm_mesh_components_workspace_bytes(750_000, 1_500_000)
    assert 4 * 750_000 + (750_000 + 1_500_000) * 12 // 64 <= big <= 8 * 750_000
    assert lib.nm_abi_version() == 6


def test_wrappers_check_their_arguments_before_the_device():
    import torch
    from nerfmeshes_amd import _lib, hip_ops
    with pytest.raises(_lib.HipLibraryError, match="GPU memory"):
        hip_ops.mesh_components(torch.zeros(4, 3, dtype=torch.int32), 8)
    with pytest.raises(_lib.HipLibraryError, match="GPU memory"):
        hip_ops.mesh_filter_components(torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(8, 3))
    with pytest.raises(ValueError, match=">= 0"):
        hip_ops.mesh_filter_components(torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(8, 3), min_faces=-1)
    with pytest.raises(ValueError, match="at most 1024"):
        hip_ops.mesh_filter_components(torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(8, 3), keep_largest=1025)
