"""Numpy restatement of the mesh cleaning (bf_marching_cubes_clean / bf_mesh_clean_host, DESIGN.md "Mesh cleaning: the definition") and of the PLY writer with
normals, independent of the product; the yardstick of tests/test_mesh_clean_cpu.py and tests/test_mesh_clean_gpu.py.

Definition, over an indexed mesh of nv vertices (position, colour) and nf faces of three vertex ids each:
  * vertices that share a face are adjacent; a component is a connected set of vertices, its label its lowest vertex id; a face belongs to the component of its
    vertices; a component's size is its number of faces; a vertex in no face is an isolated vertex, a component of size 0;
  * a component passes iff size >= max(1, min_faces); with `largest` only the passing component of greatest size stays, the lowest label among equal sizes;
  * output: the vertices of the kept components in increasing old id (positions and colours copied), the kept faces in their old order and winding, ids remapped;
  * normals, on the output mesh, binary32 with one rounding per operation: N_f = (P[b] - P[a]) x (P[c] - P[a]), not normalised; S_v starts at +0 and receives N_f
    once per corner of f that is v, in increasing corner number 3f + c; n_v = S_v / sqrt((S.x*S.x + S.y*S.y) + S.z*S.z) where that length is finite and > 0,
    (0, 0, 0) otherwise.

labels() is a vectorised fixed-point iteration (faces pull their three labels down to the lowest, then every label jumps to its label's label); labels_union_find()
is the plain sequential union-find, for small meshes.  The planted builders return (positions [nv,3] float32, colours [nv,3] float32, faces [nf,3] uint32); every
one takes T (the number of faces of its main part), a seed and the order of the vertex ids - labels are minima over ids, so the numbering is what stresses a
parallel labelling."""
import numpy as np

from tests import mesh_weld_ref

M = 7          # the threshold the `patches` family is planted around: patches of M - 1, M, M and M + 1 faces
ORDERS = ("ascending", "descending", "shuffled")
STAT_KEYS = ("numVerticesIn", "numFacesIn", "numVerticesOut", "numFacesOut", "numComponents", "numComponentsKept", "numIsolatedVertices", "largestComponentFaces")


# --------------------------------------------------------------------------- the definition
def labels(nv, faces):
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3).astype(np.int64)
    lab = np.arange(nv, dtype=np.int64)
    if len(f) == 0:
        return lab.astype(np.uint32)
    while True:
        new = lab.copy()
        np.minimum.at(new, f.reshape(-1), np.repeat(lab[f].min(axis=1), 3))
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, lab):
            return lab.astype(np.uint32)
        lab = new


def labels_union_find(nv, faces):
    """the sequential form, in plain Python"""
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(u, v):
        u, v = find(u), find(v)
        if u != v:
            parent[max(u, v)] = min(u, v)

    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        unite(a, b)
        unite(b, c)
    return np.array([find(v) for v in range(nv)], np.uint32)


def vertex_normals(pos, faces):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3).astype(np.int64)
    e1 = pos[f[:, 1]] - pos[f[:, 0]]
    e2 = pos[f[:, 2]] - pos[f[:, 0]]
    with np.errstate(all="ignore"):
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(np.float32)
        S = np.zeros((len(pos), 3), np.float32)
        np.add.at(S, f.reshape(-1), np.repeat(N, 3, axis=0))          # unbuffered: in increasing corner number
        L = np.sqrt((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])
        ok = np.isfinite(L) & (L > 0)
        n = np.zeros_like(S)
        n[ok] = S[ok] / L[ok, None]
    assert N.dtype == S.dtype == L.dtype == n.dtype == np.float32
    return n


def clean(pos, col, faces, min_faces=0, largest=False, normals=False):
    """-> (positions, colours, normals or None, faces, stats dict, labels of the input vertices)"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); col = np.ascontiguousarray(col, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    nv, nf = len(pos), len(faces)
    assert len(col) == nv and (nf == 0 or int(faces.max()) < nv)
    lab = labels(nv, faces).astype(np.int64)
    face_lab = lab[faces[:, 0].astype(np.int64)]
    size = np.bincount(face_lab, minlength=nv)[:nv] if nv else np.zeros(0, np.int64)
    root = lab == np.arange(nv)
    comps = np.nonzero(root & (size >= 1))[0]
    passing = comps[size[comps] >= max(1, int(min_faces))]
    if largest and len(passing):
        kept = passing[[int(np.argmax(size[passing]))]]          # argmax: the first of equal sizes, and `passing` is in increasing label
    else:
        kept = passing
    keep_root = np.zeros(nv, bool); keep_root[kept] = True
    keep_v = keep_root[lab] if nv else np.zeros(0, bool)
    keep_f = keep_root[face_lab] if nf else np.zeros(0, bool)
    new_id = np.cumsum(keep_v) - 1
    out_pos, out_col = pos[keep_v].copy(), col[keep_v].copy()
    out_faces = new_id[faces[keep_f].astype(np.int64)].astype(np.uint32).reshape(-1, 3)
    stats = dict(numVerticesIn=nv, numFacesIn=nf, numVerticesOut=int(keep_v.sum()), numFacesOut=int(keep_f.sum()), numComponents=len(comps), numComponentsKept=len(kept),
                 numIsolatedVertices=int((root & (size == 0)).sum()), largestComponentFaces=int(size[comps].max()) if len(comps) else 0)
    return out_pos, out_col, (vertex_normals(out_pos, out_faces) if normals else None), out_faces, stats, lab.astype(np.uint32)


def ply_bytes_normals(pos, normals, col, faces):
    """the file bf_write_ply_indexed_normals writes; normals None: bf_write_ply_indexed's"""
    if normals is None:
        return mesh_weld_ref.ply_bytes(pos, col, faces)
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); col = np.ascontiguousarray(col, np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3); faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    head = ("ply\nformat binary_little_endian 1.0\ncomment bundlefusion_amd marching cubes\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(pos), len(faces))).encode()
    v = np.zeros(len(pos), np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 4)]))
    v["p"] = pos; v["n"] = normals
    scaled = col * np.float32(255.0) + np.float32(0.5)
    v["c"][:, :3] = np.maximum(np.float32(0.0), np.minimum(np.float32(255.0), scaled)).astype(np.uint8)
    v["c"][:, 3] = 255
    f = np.zeros(len(faces), np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    f["n"] = 3; f["i"] = faces.view(np.int32)
    assert v.dtype.itemsize == 28 and f.dtype.itemsize == 13
    return head + v.tobytes() + f.tobytes()


# --------------------------------------------------------------------------- planted meshes
# A piece is (positions [n,3] float64, faces [k,3] int64) with ids of its own; _finish() joins pieces, numbers the vertices in the asked order - `first` / `last`
# name vertices that must carry the lowest / highest ids whatever the order - and gives every vertex a colour of its own.
def _grid_patch(k, rng, origin=(0.0, 0.0, 0.0)):
    """a connected patch of exactly k faces cut row by row from a triangulated grid, on a bumpy surface"""
    if k == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    w = max(1, int(np.sqrt(k / 2.0)))
    rows = -(-k // (2 * w))
    r, c = np.meshgrid(np.arange(rows), np.arange(w), indexing="ij")
    v00 = (r * (w + 1) + c).reshape(-1); v01 = v00 + 1; v10 = v00 + (w + 1); v11 = v10 + 1
    f = np.stack([np.stack([v00, v01, v11], 1), np.stack([v00, v11, v10], 1)], 1).reshape(-1, 3)[:k]
    used = np.unique(f)
    remap = np.full((rows + 1) * (w + 1), -1, np.int64); remap[used] = np.arange(len(used))
    gy, gx = np.divmod(used, w + 1)
    p = np.stack([gx * 0.01, gy * 0.01, 0.003 * np.sin(gx * 0.7) * np.cos(gy * 0.9)], 1) + rng.uniform(-0.002, 0.002, (len(used), 3)) + np.asarray(origin)
    return p, remap[f]


def _join(pieces):
    pos, faces, base = [], [], 0
    for p, f in pieces:
        pos.append(np.asarray(p, np.float64).reshape(-1, 3)); faces.append(np.asarray(f, np.int64).reshape(-1, 3) + base); base += len(pos[-1])
    return np.concatenate(pos) if pos else np.zeros((0, 3)), np.concatenate(faces) if faces else np.zeros((0, 3), np.int64)


def _finish(pos, faces, order, rng, first=(), last=()):
    assert order in ORDERS
    nv = len(pos)
    pinned = set(first) | set(last)
    free = np.array([v for v in range(nv) if v not in pinned], np.int64)
    if order == "descending":
        free = free[::-1]
    elif order == "shuffled":
        free = rng.permutation(free)
    sequence = np.concatenate([np.array(list(first), np.int64), free, np.array(list(last), np.int64)]).astype(np.int64)          # sequence[new id] = old id
    new_id = np.empty(nv, np.int64); new_id[sequence] = np.arange(nv)
    col = ((sequence.astype(np.float64)[:, None] * [0.618033988, 0.414213562, 0.732050807] + rng.uniform(0, 1e-3, (nv, 3))) % 1.0).astype(np.float32)
    return pos[sequence].astype(np.float32), col, new_id[faces].astype(np.uint32).reshape(-1, 3)


def _islands_piece(T, rng):
    p = rng.uniform(-1.0, 1.0, (T, 1, 3)) + rng.uniform(-0.02, 0.02, (T, 3, 3))
    return p.reshape(-1, 3), np.arange(3 * T, dtype=np.int64).reshape(-1, 3)


def _strip_piece(T, rng):
    n = T + 2 if T else 0
    i = np.arange(n)
    p = np.stack([i * 0.01, (i % 2) * 0.01, 0.004 * np.sin(i * 0.3)], 1) + rng.uniform(-0.002, 0.002, (n, 3))
    t = np.arange(T)
    f = np.stack([t, t + 1, t + 2], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]          # a consistent winding
    return p, f


def _fan_piece(T, rng):
    """T faces around a hub (vertex 0 of the piece), on a cone that winds round several times"""
    if T == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    a = np.arange(T + 1) * 0.37
    rim = np.stack([np.cos(a) * (1.0 + 0.01 * np.arange(T + 1) / (T + 1)), np.sin(a), 0.3 + 0.1 * np.sin(a * 0.5)], 1) + rng.uniform(-0.01, 0.01, (T + 1, 3))
    t = np.arange(T)
    return np.concatenate([[[0.0, 0.0, 0.0]], rim]), np.stack([np.zeros(T, np.int64), t + 1, t + 2], 1)


def islands(T, seed=0, order="ascending"):
    """T separate triangles: T components of size 1"""
    rng = np.random.default_rng(seed)
    return _finish(*_islands_piece(T, rng), order, rng)


def strip(T, seed=0, order="ascending"):
    """one triangle strip of T faces: the deepest parent chain"""
    rng = np.random.default_rng(seed)
    return _finish(*_strip_piece(T, rng), order, rng)


def fan(T, seed=0, order="ascending"):
    """T faces around one hub vertex that carries the highest id: degree T, the long normals segment"""
    rng = np.random.default_rng(seed)
    p, f = _fan_piece(T, rng)
    return _finish(p, f, order, rng, last=[0] if T else [])


def patches(T, seed=0, order="ascending"):
    """grid patches of M - 1, M, M and M + 1 faces - the threshold boundary at min_faces = M - and two large ones of T faces each: the tie for `largest`, which the
    patch with the lower label wins in every id order (for T <= M the small patches take part in it too)"""
    rng = np.random.default_rng(seed)
    sizes = [M - 1, T, M, M, T, M + 1]
    return _finish(*_join([_grid_patch(k, rng, origin=(0.0, 0.0, 0.5 * i)) for i, k in enumerate(sizes)]), order, rng)


def bridge(T, seed=0, order="ascending", through="face"):
    """two patches of T faces each, joined by a single face whose three vertices carry the three highest ids (through="face": one vertex of either patch and one
    of its own) or through one shared vertex only (through="vertex"): one component either way"""
    rng = np.random.default_rng(seed)
    pa, fa = _grid_patch(T, rng); pb, fb = _grid_patch(T, rng, origin=(0.0, 0.0, 1.0))
    if T == 0:
        pa = pb = np.array([[0.0, 0.0, 0.0]])
    if through == "vertex":
        pos, faces = _join([(pa, fa), (pb, fb)])
        shared, dup = len(pa) - 1, len(pa)                      # B's first vertex becomes A's last one
        faces[faces == dup] = shared
        faces[faces > dup] -= 1
        pos = np.delete(pos, dup, axis=0)
        return _finish(pos, faces, order, rng)
    pos, faces = _join([(pa, fa), (pb, fb), (np.array([[0.3, 0.3, 0.5]]), np.zeros((0, 3), np.int64))])
    a, b, x = len(pa) - 1, len(pa), len(pa) + len(pb)
    faces = np.concatenate([faces[:len(fa)], [[a, x, b]], faces[len(fa):]])          # in the middle of the face list
    return _finish(pos, faces, order, rng, last=[a, b, x])


def isolated(T, seed=0, order="ascending"):
    """a strip, islands and a patch, plus five vertices in no face, among them id 0 and id nv - 1"""
    rng = np.random.default_rng(seed)
    pos, faces = _join([_strip_piece(T // 2, rng), _islands_piece(T - T // 2, rng), _grid_patch(M, rng, origin=(0.0, 0.0, 2.0)), (rng.uniform(-1, 1, (5, 3)), np.zeros((0, 3), np.int64))])
    nv = len(pos)
    return _finish(pos, faces, order, rng, first=[nv - 5], last=[nv - 1])


def repeated(T, seed=0, order="ascending"):
    """patches and islands with faces of two or three equal ids mixed in: (v, v, w) inside a component, (v, v, w) across two components - which joins them -,
    (v, v, v) on a vertex of a component and on a vertex that has no other face"""
    rng = np.random.default_rng(seed)
    pos, faces = _join([_grid_patch(T, rng), _grid_patch(M, rng, origin=(0.0, 0.0, 1.0)), _islands_piece(4, rng), (rng.uniform(-1, 1, (2, 3)), np.zeros((0, 3), np.int64))])
    nv = len(pos)
    lone, other = nv - 2, nv - 1
    extra = [[lone, lone, lone], [nv - 3, nv - 3, nv - 4], [nv - 5, nv - 8, nv - 5]]          # the second inside an island; the third joins two islands
    if T:
        extra += [[0, 0, 0], [int(faces[0, 1]), int(faces[0, 0]), int(faces[0, 0])], [len(np.unique(faces[:T])) + 1, 0, 0]]          # the last joins the two patches
    k = max(1, len(faces) // max(1, len(extra)))
    out = faces
    for i, e in enumerate(extra):
        at = min(len(out), i * k + 1)
        out = np.concatenate([out[:at], [e], out[at:]])
    return _finish(pos, out, order, rng, last=[other])          # `other` stays isolated


def mixed(T, seed=0, order="ascending"):
    """all of it, side by side"""
    rng = np.random.default_rng(seed)
    q = T // 4
    parts = [_islands_piece(q, rng), _strip_piece(q, rng), _fan_piece(q, rng), _grid_patch(T - 3 * q, rng, origin=(0.0, 0.0, 1.0)), _grid_patch(M, rng, origin=(0.0, 0.0, 1.5)),
             _grid_patch(M - 1, rng, origin=(0.0, 0.0, 2.0)), _grid_patch(M, rng, origin=(0.0, 0.0, 2.5)), (rng.uniform(-1, 1, (4, 3)), np.zeros((0, 3), np.int64))]
    pos, faces = _join(parts)
    nv = len(pos)
    faces = np.concatenate([faces, [[nv - 6, nv - 6, nv - 7], [nv - 2, nv - 2, nv - 2]]])          # repeated ids: inside the last patch, and on a vertex of its own
    faces = faces[rng.permutation(len(faces))]
    return _finish(pos, faces, order, rng, first=[nv - 4], last=[nv - 1])


FAMILIES = ("islands", "strip", "fan", "patches", "bridge", "bridge_vertex", "isolated", "repeated", "mixed")


def build(family, T, seed=0, order="ascending"):
    if family == "bridge_vertex":
        return bridge(T, seed, order, through="vertex")
    return globals()[family](T, seed, order)
