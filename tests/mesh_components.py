"""The mesh-component filter restated in numpy (the role tests/surface_filter.py and tests/ss_refine.py play for their
kernels): what nm_mesh_components / _select / _compact must give, integer for integer.

  connectivity  two vertices are connected when a triangle holds both
  label         a component's smallest vertex index (min-label propagation to a fixed point)
  size          its number of triangles (bincount of the faces' labels); a vertex in no triangle is a component of size 0
  selection     components with fewer than min_faces triangles go; of the rest the keep_largest with most triangles stay, by a
                stable sort on (-count, label); fewer than keep_largest left: all stay; 0 = no limit
  compaction    kept faces and vertices in their order, new = cumsum(keep_v) - 1, faces' = new[faces[keep_f]]
"""
import numpy as np


def labels(faces, num_vertices):
    """(V,) int32: min-label propagation over the triangles' edges to a fixed point, with pointer jumping between sweeps."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lab = np.arange(num_vertices, dtype=np.int64)
    if len(faces) == 0:
        return lab.astype(np.int32)
    assert faces.min() >= 0 and faces.max() < num_vertices
    while True:
        before = lab.copy()
        low = lab[faces].min(axis=1)                       # the smallest label on each triangle ...
        for k in range(3):
            np.minimum.at(lab, faces[:, k], low)           # ... reaches its three vertices
        while True:                                        # a label is a vertex: follow it to that vertex's label
            jumped = lab[lab]
            if np.array_equal(jumped, lab):
                break
            lab = jumped
        if np.array_equal(lab, before):
            return lab.astype(np.int32)


def face_counts(faces, lab):
    """(V,) int32: triangles per component at the component's label, 0 elsewhere."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.bincount(np.asarray(lab, dtype=np.int64)[faces[:, 0]], minlength=len(lab)).astype(np.int32)


def components(faces, num_vertices):
    lab = labels(faces, num_vertices)
    return lab, face_counts(faces, lab)


def select(lab, counts, min_faces=0, keep_largest=0):
    """(V,) bool over LABELS: True at the roots of the components that stay."""
    lab = np.asarray(lab, dtype=np.int64)
    roots = np.flatnonzero(lab == np.arange(len(lab)))
    roots = roots[counts[roots] >= min_faces]
    if keep_largest > 0:
        order = np.lexsort((roots, -counts[roots].astype(np.int64)))     # stable: count descending, then label ascending
        roots = roots[order[:keep_largest]]
    keep = np.zeros(len(lab), dtype=bool)
    keep[roots] = True
    return keep


def filter_components(verts, faces, normals, values=None, keys=None, min_faces=0, keep_largest=0, labelled=None):
    """-> (verts, faces, normals, values, keys, info), as hip_ops.mesh_filter_components.  labelled: `components(faces, V)` where
    the caller already has it."""
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    nv = len(verts)
    lab, counts = labelled if labelled is not None else components(faces, nv)
    keep_root = select(lab, counts, min_faces, keep_largest)
    keep_v = keep_root[lab]
    keep_f = keep_v[faces[:, 0]] if len(faces) else np.zeros(0, dtype=bool)
    new = np.cumsum(keep_v) - 1
    out_faces = new[faces[keep_f]].astype(np.int32).reshape(-1, 3)
    pick = lambda a: None if a is None else np.asarray(a)[keep_v]     # noqa: E731
    info = dict(components=int((lab == np.arange(nv)).sum()), components_kept=int(keep_root.sum()), faces=len(faces),
                faces_kept=int(keep_f.sum()), vertices=nv, vertices_kept=int(keep_v.sum()))
    return pick(verts), out_faces, pick(normals), pick(values), pick(keys), info


def scipy_components(faces, num_vertices):
    """(count, (V,) labels in scipy's own numbering) from scipy.sparse.csgraph, or None where scipy is not installed."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return None
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows = np.concatenate((faces[:, 0], faces[:, 1]))
    cols = np.concatenate((faces[:, 1], faces[:, 2]))
    graph = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(num_vertices, num_vertices))
    return connected_components(graph, directed=False)


def canonical(other, num_vertices):
    """any component numbering -> the smallest vertex index of each component"""
    other = np.asarray(other, dtype=np.int64)
    low = np.full(int(other.max()) + 1 if len(other) else 0, num_vertices, dtype=np.int64)
    np.minimum.at(low, other, np.arange(num_vertices))
    return low[other].astype(np.int32)
