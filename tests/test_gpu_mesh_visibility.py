"""GPU: the hidden-face filter (nm_mesh_visibility_views / _select / _compact, hip_ops.mesh_cull_hidden, mesh_nerf
--cull-hidden-views).  Integer work and bits that only rise, so every comparison with the numpy restatement
(tests/mesh_visibility.py) is exact -- new_faces, the counts and the four output arrays: nested spheres, a shell with a window,
a soup full of depth ties, one face per reject reason, bad indices, the empty cases; both raster paths, run after run; the
rings and the views called again on one workspace; then the exporter end to end, 2 ranks against 1."""
import contextlib
import ctypes as C
import io
import json
import os

import numpy as np
import pytest
import torch

from tests import mesh_raster as MR
from tests import mesh_visibility as MV
from tests.test_gpu_mesh_raster import soup
from tests.test_mesh_raster import reject_mesh
from tests.test_mesh_visibility import NESTED, framed, nested, small_cases, vertex_normals, windowed_shell  # noqa: F401
from tests.gpu_support import assert_ranks_ok, export_mesh, launch_ranks, to_device as _dev, to_numpy as _np
from tests.gpu_support import ops, scene  # noqa: F401

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = ("verts", "faces", "normals", "face_index")


def _views(ops, camera):
    poses, size, focal, _ = camera
    return [ops.make_view(pose, size, size, focal) for pose in poses]


def _device(ops, verts, faces, normals, camera, rings, **kw):
    out = ops.mesh_cull_hidden(_dev(verts, F32).reshape(-1, 3), _dev(faces, np.int32).reshape(-1, 3),
                               None if normals is None else _dev(normals, F32).reshape(-1, 3), _views(ops, camera), float(camera[3]),
                               rings=rings, **kw)
    return tuple(_np(t) for t in out[:4]) + (out[4],)


def _same(got, want, tag):
    assert got[4] == want[4], f"{tag}: info {got[4]} != {want[4]}"
    for name, a, b in zip(NAMES, got, want):
        if b is None:
            assert a is None, f"{tag}: {name}"
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{tag}: {name} differ"


@pytest.mark.parametrize("case", NESTED, ids=lambda c: "views{}_size{}_rings{}".format(*c))
def test_the_nested_spheres(ops, nested, case):  # noqa: F811
    verts, faces, normals, camera, want = nested[case]
    _same(_device(ops, verts, faces, normals, camera, case[2]), want, f"nested {case}")
    assert want[4]["faces_kept"] == {(8, 48, 0): 923, (8, 48, 1): 1024, (24, 96, 0): 960}[case]


@pytest.fixture(scope="module")
def shell():
    verts, faces, _ = windowed_shell()
    return verts, faces, vertex_normals(verts), framed(verts, 8, 48)


@pytest.fixture(scope="module")
def soup_case():
    verts, faces = soup(n=1000, faces=3000)
    return verts, faces, vertex_normals(verts), framed(verts, 4, 64)


def test_the_windowed_shell_the_soup_and_one_face_per_reject_reason(ops, shell, soup_case):
    for rings in (0, 1):
        _same(_device(ops, *shell, rings), MV.cull_hidden(*shell[:3], *shell[3], rings), f"shell, {rings} rings")
    want = MV.cull_hidden(*soup_case[:3], *soup_case[3], 1)
    _same(_device(ops, *soup_case, 1), want, "soup")
    assert 500 < want[4]["faces_seen"] < want[4]["faces_kept"]
    verts, faces, pose = reject_mesh()
    camera = (pose[None, :3], 32, 40.0, F32(0.1))
    want = MV.cull_hidden(verts, faces, None, *camera, 0)
    _same(_device(ops, verts, faces, None, camera, 0, large_threshold=16), want, "one face per reason")
    assert want[4]["bad_faces"] == 2 and want[4]["faces_seen"] == 1 and want[3].tolist() == [0]


def test_small_bad_and_empty_inputs(ops):
    for name, (verts, faces, normals, camera, rings) in small_cases().items():
        _same(_device(ops, verts, faces, normals, camera, rings), MV.cull_hidden(verts, faces, normals, *camera, rings), name)
    with pytest.raises(ValueError):
        ops.mesh_cull_hidden(torch.rand(5, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int32, device="cuda"), None,
                             [ops.make_view(np.eye(4, dtype=F32), 9, 11, 10.0, ndc_near=1.0)], 0.1)
    with pytest.raises(ValueError):
        ops.mesh_cull_hidden(torch.rand(5, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int32, device="cuda"), None, [], 0.0)


def folded_strip(nv=65539, shown=40):
    """A triangle strip of nv - 2 faces over nv vertices (two per column) in the plane z = -1, seen by a camera at the origin
    (focal 64 on 64 x 64 pixels: the image spans x, y in [-0.5, 0.5)): its first `shown` columns run left to right through the
    upper half of the image, its last `shown` right to left through the lower half, and everything between lies off screen to
    the right.  Columns are 1.28 pixels wide and 0.64 tall, across one pixel row, so of the faces in view some win a pixel centre and some
    do not.
    -> (verts, faces, camera)"""
    j = np.arange(nv) // 2
    last = j[-1] + 1 - shown
    x = np.where(j < shown, -0.45 + 0.02 * j, np.where(j >= last, 0.45 - 0.02 * (j - last), 5.0 + 1e-4 * j))
    y = 0.2 - 0.39 * np.clip((j - shown) / float(last - shown), 0.0, 1.0) + 0.01 * (np.arange(nv) % 2)
    first = np.arange(nv - 2, dtype=np.int32)
    pose = np.eye(4, dtype=F32)[None, :3]
    return np.stack([x, y, np.full(nv, -1.0)], -1).astype(F32), np.stack([first, first + 1, first + 2], -1), (pose, 64, 64.0, F32(0.1))


def test_compaction_at_the_chunk_boundary_of_the_scan(ops):
    """65 537 faces over 65 539 vertices: 1025 words of face keep bits and as many of vertex bits, so the last face and the last
    vertices sit in the first word of the second chunk of the one-workgroup scan (csrc/compact.h) and their rows out need the
    carry that the first chunk hands over.  The strip's two ends are in view, so kept and dropped faces alternate in the first
    words and in the last, and everything between is dropped."""
    verts, faces, camera = folded_strip()
    assert len(faces) == 65537 and len(verts) == 65539 and (len(faces) + 63) // 64 == 1025
    want = MV.cull_hidden(verts, faces, None, *camera, 0)
    _same(_device(ops, verts, faces, None, camera, 0), want, "folded strip")
    kept, info = want[3], want[4]
    assert kept[-1] == 65536 and want[1][-1].max() == info["vertices_kept"] - 1, "the last face and its vertices are rows out"
    front, back = int((kept < 80).sum()), int((kept >= 65537 - 80).sum())    # 78 faces in view + the two that leave it
    assert 8 < front < 70 and 8 < back < 70 and front + back == info["faces_kept"] == info["faces_seen"], "both ends, in part"


def test_both_raster_paths_give_the_same_bytes_run_after_run(ops, shell, soup_case):
    for tag, case in (("shell", shell), ("soup", soup_case)):
        runs = [_device(ops, *case, 1, large_threshold=t) for t in (None, None, 0, 2 ** 30)]
        for other in runs[1:]:
            _same(other, runs[0], f"{tag}: another threshold or another run")


class Session:
    """the three C entries on one workspace, as a caller of the C ABI uses them"""

    def __init__(self, ops, verts, faces, normals, size):
        from nerfmeshes_amd import _lib
        self.ops, self.lib, self._lib = ops, _lib.load(), _lib
        self.verts, self.faces, self.normals = _dev(verts, F32), _dev(faces, np.int32), _dev(normals, F32)
        self.nv, self.nf = len(verts), len(faces)
        self.ws = torch.empty(int(self.lib.nm_mesh_visibility_workspace_bytes(self.nv, self.nf, size, size)), dtype=torch.uint8,
                              device="cuda")

    def views(self, views, near, clear):
        """-> (new_faces, the rasteriser's counts per view)"""
        ptr, ops = self.ops._ptr, self.ops
        new = torch.full((len(views),), -1, dtype=torch.int64, device="cuda")
        counts = torch.full((len(views), len(ops.RASTER_COUNTS)), -1, dtype=torch.int64, device="cuda")
        array = (self._lib.View * len(views))(*views)
        self._lib.check(self.lib.nm_mesh_visibility_views(array, len(views), ptr(self.verts), self.nv, ptr(self.faces), self.nf,
                                                          float(near), ops.RASTER_LARGE_THRESHOLD, clear, ptr(self.ws), ptr(new),
                                                          ptr(counts), ops._stream()), "nm_mesh_visibility_views")
        return new.tolist(), [dict(zip(ops.RASTER_COUNTS, row)) for row in counts.tolist()]

    def select(self, rings):
        """-> the four arrays after `rings` rings + (vertices kept, faces kept, faces seen, bad faces)"""
        ptr = self.ops._ptr
        out = [C.c_int64() for _ in range(4)]
        self._lib.check(self.lib.nm_mesh_visibility_select(ptr(self.faces), self.nf, self.nv, rings, ptr(self.ws),
                                                           *(C.byref(o) for o in out), self.ops._stream()), "nm_mesh_visibility_select")
        kv, kf = out[0].value, out[1].value
        v, n = torch.empty(kv, 3, device="cuda"), torch.empty(kv, 3, device="cuda")
        f, index = torch.empty(kf, 3, dtype=torch.int32, device="cuda"), torch.empty(kf, dtype=torch.int32, device="cuda")
        self._lib.check(self.lib.nm_mesh_visibility_compact(ptr(self.ws), ptr(self.faces), self.nf, self.nv, ptr(self.verts),
                                                            ptr(self.normals), kv, kf, ptr(v), ptr(f), ptr(n), ptr(index),
                                                            self.ops._stream()), "nm_mesh_visibility_compact")
        return tuple(_np(t) for t in (v, f, n, index)) + (tuple(o.value for o in out),)


def _restated(verts, faces, normals, seen, rings):
    keep_f, keep_v, bad = MV.grow(faces, len(verts), seen, rings)
    return MV.compact(verts, faces, normals, keep_f, keep_v) + ((int(keep_v.sum()), int(keep_f.sum()), int(seen.sum()), bad),)


def test_select_and_views_again_on_one_workspace(ops, shell):
    verts, faces, normals, camera = shell
    poses, size, focal, near = camera
    views = _views(ops, camera)
    seen, new_faces, counts = MV.seen_faces(verts, faces, poses, size, focal, near)
    session = Session(ops, verts, faces, normals, size)
    got_new, got_counts = session.views(views, near, 1)
    assert got_new == new_faces and got_counts == counts, "every view's new faces and the rasteriser's own counts"
    answers = [session.select(rings) for rings in (0, 2, 0)]
    for rings, got in zip((0, 2, 0), answers):
        want = _restated(verts, faces, normals, seen, rings)
        assert got[4] == want[4] and all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], want[:4])), f"{rings} rings"
    assert answers[1][4][1] > answers[0][4][1] and answers[1][4][2] == answers[0][4][2], "the seen bits stay as they were"
    first, _ = session.views(views[:3], near, 1)                     # clears: the first three views alone
    part = MV.seen_faces(verts, faces, poses[:3], size, focal, near)[0]
    assert first == new_faces[:3] and session.select(0)[4] == _restated(verts, faces, normals, part, 0)[4]
    later, _ = session.views(views[3:], near, 0)                     # accumulates
    assert first + later == new_faces, "two calls equal one call over the concatenated views"
    again = session.select(2)
    assert again[4] == answers[1][4] and all(a.tobytes() == b.tobytes() for a, b in zip(again[:4], answers[1][:4]))
    none, _ = session.views([], near, 0)
    assert none == [] and session.select(2)[4] == answers[1][4], "no view changes nothing"


def test_the_rasteriser_is_unchanged_afterwards(ops, nested):  # noqa: F811
    verts, faces, normals, camera, want = nested[8, 48, 0]
    _same(_device(ops, verts, faces, normals, camera, 0), want, "nested")
    pose, size, focal, near = camera[0][5], camera[1], camera[2], camera[3]
    raster = ops.mesh_rasterize(_dev(verts), _dev(faces), ops.make_view(pose, size, size, focal), float(near))
    restated = MR.rasterize(verts, faces, pose, size, size, focal, near)
    assert raster[3] == restated[3] and all(_np(a).tobytes() == b.tobytes() for a, b in zip(raster[:3], restated[:3]))


def _run(model, tmp_path, tag, *extra):
    d = tmp_path / tag
    d.mkdir(exist_ok=True)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        export_mesh(model, d, "--res", "64", "--limit", "1.2", *extra)
    return d, text.getvalue()


def test_end_to_end_through_the_exporter(scene, tmp_path):
    plain, plain_text = _run(scene, tmp_path, "plain")
    zero, zero_text = _run(scene, tmp_path, "zero", "--cull-hidden-views", "0")
    culled, text = _run(scene, tmp_path, "culled", "--cull-hidden-views", "12", "--cull-size", "128")
    whole = open(plain / "mesh.obj", "rb").read()
    assert open(zero / "mesh.obj", "rb").read() == whole, "--cull-hidden-views 0 gives the former OBJ byte for byte"
    assert zero_text.replace(str(zero), "") == plain_text.replace(str(plain), "") and not os.path.exists(zero / "mesh.visibility.json")
    lines = open(culled / "mesh.obj").read().splitlines()
    before = whole.decode().splitlines()
    count = lambda rows, key: sum(1 for row in rows if row.startswith(key + " "))   # noqa: E731
    assert 0 < count(lines, "f") < count(before, "f") and 0 < count(lines, "v") < count(before, "v")
    known = set(before)
    assert all(row in known for row in lines if row.startswith(("v ", "vn "))), "a kept vertex keeps its position, colour and normal"
    report = json.load(open(culled / "mesh.visibility.json"))
    assert report["faces_kept"] == count(lines, "f") and report["vertices_kept"] == count(lines, "v") == count(lines, "vn")
    assert report["faces"] == count(before, "f") and report["vertices"] == count(before, "v")
    assert report["views"] == 12 and report["size"] == 128 and report["rings"] == 1 and report["radius"] == 3.0
    assert len(report["new_faces"]) == 12 and sum(report["new_faces"]) == report["faces_seen"] <= report["faces_kept"]
    assert (f"Hidden-face filter: kept {report['faces_kept']} of {report['faces']} faces ({report['faces_seen']} seen), "
            f"{report['vertices_kept']} of {report['vertices']} vertices, 12 views of 128², ") in text
    print(text)


def test_two_ranks_sharing_one_gpu_equal_one_rank():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    world = 2
    r = launch_ranks(os.path.join("tests", "tools", "visibility_dist_worker.py"), world, timeout=900)
    assert_ranks_ok(r, f"VISIBILITY_DIST_OK world={world}")
