"""Numpy restatement of the mesh simplification by vertex clustering (bf_marching_cubes_simplify / bf_mesh_simplify_host, DESIGN.md "Mesh simplification: the
definition"), independent of the product; the yardstick of tests/test_mesh_simplify_cpu.py and tests/test_mesh_simplify_gpu.py.

Definition, over an indexed mesh of nv vertices (position, colour; binary32) and nf faces of three vertex ids each, with a cell size c (binary32):
  * refused (ValueError here): c not finite or <= 0; a face id >= nv; a position or colour component that is not finite or has |x| >= 1024; a cell index with
    |k| >= 2^20;
  * cell of a vertex: per axis k = (int64)floor((double)p * (1.0 / (double)c)); the key is the three indices biased by 2^20, packed into 63 bits;
  * a cluster is the set of ALL input vertices with one key, its leader its lowest vertex id;
  * with q(x) = (int64)floor((double)x * 1048576.0 + 0.5), a cluster of n members has the int64 sums of q over its members' positions and colours; its
    representative is the member itself, bit for bit, where n == 1, and per component (float)((double)S / ((double)n * 1048576.0)) otherwise;
  * face ids are mapped to clusters; a face whose three clusters are not pairwise different is collapsed; among the others, faces with the same sorted triple keep
    the one with the lowest face index (the rest are duplicates); kept faces stay in face order with their winding;
  * output vertices are the clusters a kept face uses, in increasing leader id; faces are remapped to those ids; normals are mesh_clean_ref.vertex_normals of the
    output; the map holds per input vertex its output id, or 0xFFFFFFFF where its cluster is not in the output.

simplify() is vectorised; simplify_sequential() is the same definition as one dictionary loop in plain Python, for small meshes.  The planted builders return
(positions [nv,3] float32, colours [nv,3] float32, faces [nf,3] uint32, cell size, labels): `labels` [nv,3] int64 is the cell of every vertex as the CONSTRUCTION
knows it (integers the builder chose, not floats it computed), from which expected_stats() derives what the family plants; None for the generic families.  Every
builder takes T (its size), a seed and the order, which permutes the vertex and the face numbering."""
import numpy as np

from tests import mesh_clean_ref

ORDERS = ("ascending", "descending", "shuffled")
STAT_KEYS = ("numVerticesIn", "numFacesIn", "numClusters", "numVerticesOut", "numFacesOut", "numFacesCollapsed", "numFacesDuplicate", "largestCluster")
NONE = 0xFFFFFFFF
BIAS = 1 << 20


# --------------------------------------------------------------------------- the definition
def cell_indices(pos, cell_size):
    """[nv,3] float64: floor((double)p * (1.0 / (double)cellSize)), not yet converted to integers"""
    inv = np.float64(1.0) / np.float64(np.float32(cell_size))
    with np.errstate(all="ignore"):
        return np.floor(np.ascontiguousarray(pos, np.float32).reshape(-1, 3).astype(np.float64) * inv)


def quant(x):
    return np.floor(np.asarray(x, np.float32).astype(np.float64) * np.float64(1048576.0) + np.float64(0.5)).astype(np.int64)


def mean_of(S, n):
    """(float)((double)S / ((double)n * 1048576.0)): int64 -> binary64 rounds to nearest even, the multiply is exact, one division, one rounding to binary32"""
    return (np.asarray(S, np.int64).astype(np.float64) / (np.asarray(n, np.int64).astype(np.float64) * np.float64(1048576.0))).astype(np.float32)


def _checked(pos, col, faces, cell_size):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); col = np.ascontiguousarray(col, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    c = np.float32(cell_size)
    if not (np.isfinite(c) and c > 0):
        raise ValueError("cellSize")
    if len(col) != len(pos) or (len(faces) and int(faces.max()) >= len(pos)):
        raise ValueError("face id")
    for a in (pos, col):
        if not (np.isfinite(a).all() and (np.abs(a) < np.float32(1024.0)).all()):
            raise ValueError("value")
    k = cell_indices(pos, c)
    if not ((k > -float(BIAS)) & (k < float(BIAS))).all():
        raise ValueError("cell index")
    k = k.astype(np.int64) + BIAS
    return pos, col, faces, k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)


def _segment_sums(values, order, starts):
    """int64 sums of values[order] over the segments that begin at `starts`"""
    return np.add.reduceat(values[order], starts, axis=0) if len(starts) else np.zeros((0,) + values.shape[1:], np.int64)


def simplify(pos, col, faces, cell_size, normals=False):
    """-> (positions, colours, normals or None, faces, stats dict, map)"""
    pos, col, faces, keys = _checked(pos, col, faces, cell_size)
    nv, nf = len(pos), len(faces)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)          # first: the lowest vertex id of every key
    rank = np.empty(len(first), np.int64); rank[np.argsort(first)] = np.arange(len(first))          # clusters numbered in increasing leader id
    cid = rank[inverse.reshape(-1)] if nv else np.zeros(0, np.int64)
    nc = len(first)
    leader = np.sort(first)
    order = np.argsort(cid, kind="stable")
    n = np.bincount(cid, minlength=nc)
    starts = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64) if nc else np.zeros(0, np.int64)
    SP = _segment_sums(quant(pos), order, starts); SC = _segment_sums(quant(col), order, starts)
    rep_pos = mean_of(SP, n[:, None]) if nc else np.zeros((0, 3), np.float32)
    rep_col = mean_of(SC, n[:, None]) if nc else np.zeros((0, 3), np.float32)
    alone = n == 1
    rep_pos[alone] = pos[leader[alone]]; rep_col[alone] = col[leader[alone]]
    # faces
    fc = cid[faces.astype(np.int64)] if nf else np.zeros((0, 3), np.int64)
    gone = (fc[:, 0] == fc[:, 1]) | (fc[:, 1] == fc[:, 2]) | (fc[:, 0] == fc[:, 2])
    alive = np.nonzero(~gone)[0]
    if len(alive):
        _, firsts = np.unique(np.sort(fc[alive], axis=1), axis=0, return_index=True)      # the first of equal rows: the lowest face index
        kept = np.sort(alive[firsts])
    else:
        kept = np.zeros(0, np.int64)
    used = np.zeros(nc, bool); used[fc[kept].reshape(-1)] = True
    new_id = np.where(used, np.cumsum(used) - 1, NONE).astype(np.int64)
    out_pos, out_col = rep_pos[used].copy(), rep_col[used].copy()
    out_faces = new_id[fc[kept]].astype(np.uint32).reshape(-1, 3)
    stats = dict(numVerticesIn=nv, numFacesIn=nf, numClusters=nc, numVerticesOut=int(used.sum()), numFacesOut=len(kept), numFacesCollapsed=int(gone.sum()),
                 numFacesDuplicate=nf - len(kept) - int(gone.sum()), largestCluster=int(n.max()) if nc else 0)
    vmap = new_id[cid].astype(np.uint32) if nv else np.zeros(0, np.uint32)
    return out_pos, out_col, (mesh_clean_ref.vertex_normals(out_pos, out_faces) if normals else None), out_faces, stats, vmap


def simplify_sequential(pos, col, faces, cell_size, normals=False):
    """the same definition as one loop over the vertices and one over the faces, with dictionaries and Python integers"""
    pos, col, faces, keys = _checked(pos, col, faces, cell_size)
    qp, qc = quant(pos).tolist(), quant(col).tolist()
    cluster_of_key, cid, members, sums, leader = {}, [], [], [], []
    for v, key in enumerate(keys.tolist()):
        c = cluster_of_key.setdefault(key, len(cluster_of_key))
        if c == len(members):
            members.append(0); sums.append([0] * 6); leader.append(v)
        cid.append(c); members[c] += 1
        for d in range(3):
            sums[c][d] += qp[v][d]; sums[c][3 + d] += qc[v][d]
    seen, kept, used, gone = set(), [], set(), 0
    for f, (a, b, c) in enumerate(faces.tolist()):
        t = (cid[a], cid[b], cid[c])
        if len(set(t)) < 3:
            gone += 1
            continue
        s = tuple(sorted(t))
        if s in seen:
            continue
        seen.add(s); kept.append(f); used.update(t)
    new_id, out_pos, out_col = {}, [], []
    for c in range(len(members)):
        if c not in used:
            continue
        new_id[c] = len(new_id)
        if members[c] == 1:
            out_pos.append(pos[leader[c]]); out_col.append(col[leader[c]])
        else:
            out_pos.append(mean_of(sums[c][:3], members[c])); out_col.append(mean_of(sums[c][3:], members[c]))
    out_pos = np.array(out_pos, np.float32).reshape(-1, 3); out_col = np.array(out_col, np.float32).reshape(-1, 3)
    out_faces = np.array([[new_id[cid[v]] for v in faces[f].tolist()] for f in kept], np.uint32).reshape(-1, 3)
    stats = dict(numVerticesIn=len(pos), numFacesIn=len(faces), numClusters=len(members), numVerticesOut=len(new_id), numFacesOut=len(kept), numFacesCollapsed=gone,
                 numFacesDuplicate=len(faces) - len(kept) - gone, largestCluster=max(members) if members else 0)
    vmap = np.array([new_id.get(c, NONE) for c in cid], np.uint32)
    return out_pos, out_col, (mesh_clean_ref.vertex_normals(out_pos, out_faces) if normals else None), out_faces, stats, vmap


def expected_stats(labels, faces):
    """what a mesh plants, from the cells its builder chose: the stats the definition must give"""
    cluster, cid, members = {}, [], []
    for l in map(tuple, np.asarray(labels, np.int64).reshape(-1, 3).tolist()):
        c = cluster.setdefault(l, len(cluster))
        if c == len(members):
            members.append(0)
        cid.append(c); members[c] += 1
    seen, used, gone = set(), set(), 0
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        t = (cid[a], cid[b], cid[c])
        if len(set(t)) < 3:
            gone += 1
        elif tuple(sorted(t)) not in seen:
            seen.add(tuple(sorted(t))); used.update(t)
    nf = len(np.asarray(faces).reshape(-1, 3))
    return dict(numVerticesIn=len(cid), numFacesIn=nf, numClusters=len(members), numVerticesOut=len(used), numFacesOut=len(seen), numFacesCollapsed=gone,
                numFacesDuplicate=nf - len(seen) - gone, largestCluster=max(members) if members else 0)


# --------------------------------------------------------------------------- planted meshes
def _finish(pos, faces, labels, order, rng):
    """numbers vertices and faces in the asked order; every vertex gets a colour of its own in [0, 1)"""
    assert order in ORDERS
    pos = np.asarray(pos, np.float32).reshape(-1, 3); faces = np.asarray(faces, np.int64).reshape(-1, 3); labels = np.asarray(labels, np.int64).reshape(-1, 3)
    nv, nf = len(pos), len(faces)
    assert len(labels) == nv
    sv, sf = np.arange(nv), np.arange(nf)
    if order == "descending":
        sv, sf = sv[::-1], sf[::-1]
    elif order == "shuffled":
        sv, sf = rng.permutation(nv), rng.permutation(nf)
    new_id = np.empty(nv, np.int64); new_id[sv] = np.arange(nv)
    col = ((sv.astype(np.float64)[:, None] * [0.618033988, 0.414213562, 0.732050807] + rng.uniform(0, 1e-3, (nv, 3))) % 1.0).astype(np.float32)
    return pos[sv].copy(), col, new_id[faces[sf]].astype(np.uint32).reshape(-1, 3), labels[sv].copy()


def _lattice_faces(k):
    """exactly k faces cut row by row from a triangulated lattice: (integer lattice coordinates [n,2] of the vertices used, faces [k,3])"""
    if k == 0:
        return np.zeros((0, 2), np.int64), np.zeros((0, 3), np.int64)
    w = max(1, int(np.sqrt(k / 2.0)))
    rows = -(-k // (2 * w))
    r, c = np.meshgrid(np.arange(rows), np.arange(w), indexing="ij")
    v00 = (r * (w + 1) + c).reshape(-1); v01 = v00 + 1; v10 = v00 + (w + 1); v11 = v10 + 1
    f = np.stack([np.stack([v00, v01, v11], 1), np.stack([v00, v11, v10], 1)], 1).reshape(-1, 3)[:k]
    used = np.unique(f)
    remap = np.full((rows + 1) * (w + 1), -1, np.int64); remap[used] = np.arange(len(used))
    gy, gx = np.divmod(used, w + 1)
    return np.stack([gx, gy], 1), remap[f]


def _inside(cells, cell, rng, lo=0.2, hi=0.8):
    """a binary32 position well inside each of the integer cells [n,3]"""
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    return ((cells + rng.uniform(lo, hi, cells.shape)) * float(np.float32(cell))).astype(np.float32)


def _one_per_cell(T, rng, cell, origin=(0, 0, 0)):
    """T lattice faces with every vertex alone in a cell of its own"""
    g, f = _lattice_faces(T)
    cells = np.concatenate([g, np.zeros((len(g), 1), np.int64)], 1) + np.asarray(origin, np.int64)
    return _inside(cells, cell, rng), f, cells


def _done(finished, cell):
    pos, col, faces, labels = finished
    return pos, col, faces, cell, labels


def grid(T, seed=0, order="ascending"):
    """a patch of T faces with spacing cellSize / 3: 3 x 3 vertices merge per cell, the faces inside a cell and across one cell border collapse, the two faces where
    four cells meet stay; every fifth face is there a second time with its ids rotated, a duplicate wherever the face stays"""
    rng = np.random.default_rng(seed); cell = 0.03
    g, f = _lattice_faces(T)
    labels = np.concatenate([g // 3, np.zeros((len(g), 1), np.int64)], 1)
    pos = np.stack([(g[:, 0] + 0.5) * 0.01, (g[:, 1] + 0.5) * 0.01, 0.015 + 0.009 * np.sin(g[:, 0] * 0.7) * np.cos(g[:, 1] * 0.9)], 1).astype(np.float32)
    f = np.concatenate([f, f[::5][:, [1, 2, 0]]])
    return _done(_finish(pos, f, labels, order, rng), cell)


def straddle(T, seed=0, order="ascending"):
    """T faces over vertices whose coordinates are -0.25 cellSize, -0.0, +0.0 or +0.25 cellSize: floor, not truncation, decides the cell (-1 for the first, 0 for
    the other three - the two zeros share a cell)"""
    rng = np.random.default_rng(seed); cell = 0.0625
    values = np.array([-0.25 * cell, -0.0, 0.0, 0.25 * cell], np.float32); cells = np.array([-1, 0, 0, 0], np.int64)
    pick = rng.integers(0, 4, (3 * T, 3))
    if T >= 2:
        pick[:4, 0] = [0, 1, 2, 3]          # every value is there
    return _done(_finish(values[pick], np.arange(3 * T).reshape(-1, 3), cells[pick], order, rng), cell)


def boundary(T, seed=0, order="ascending"):
    """cellSize = 2^-6; T faces over vertices whose coordinates are exactly k * cellSize (cell k) or the binary32 number just below it (cell k - 1), k negative,
    zero and positive"""
    rng = np.random.default_rng(seed); cell = 2.0 ** -6
    k = rng.integers(-40, 41, (3 * T, 3)); below = rng.integers(0, 2, (3 * T, 3)).astype(bool)
    exact = (k * cell).astype(np.float32)
    pos = np.where(below, np.nextafter(exact, np.float32(-np.inf)), exact).astype(np.float32)
    return _done(_finish(pos, np.arange(3 * T).reshape(-1, 3), k - below, order, rng), cell)


def hub(T, seed=0, order="ascending"):
    """T vertices with distinct positions inside ONE cell, each with a face to two of eight vertices in cells of their own around it: the cluster size is T, and only
    eight different faces come out of it"""
    rng = np.random.default_rng(seed); cell = 0.05
    ring = np.array([[2, 0, 0], [2, 2, 0], [0, 2, 0], [-2, 2, 0], [-2, 0, 0], [-2, -2, 0], [0, -2, 0], [2, -2, 0]], np.int64)
    labels = np.concatenate([np.zeros((T, 3), np.int64), ring])
    i = np.arange(T)
    faces = np.stack([i, T + i % 8, T + (i + 1) % 8], 1)
    return _done(_finish(_inside(labels, cell, rng, 0.05, 0.95), faces, labels, order, rng), cell)


def sheets(T, seed=0, order="ascending"):
    """two sheets of T faces each, one vertex of either per cell, the second with the opposite winding: every face has its mirror image, and the one with the lower
    face index stays, with its winding"""
    rng = np.random.default_rng(seed); cell = 0.04
    pa, f, cells = _one_per_cell(T, rng, cell)
    pb = _inside(cells, cell, rng)
    return _done(_finish(np.concatenate([pa, pb]), np.concatenate([f, f[:, [0, 2, 1]] + len(pa)]), np.concatenate([cells, cells]), order, rng), cell)


def singles(T, seed=0, order="ascending"):
    """T faces, every vertex used and alone in its cell, at positions that do not survive the quantisation: the output is the input, bit for bit"""
    rng = np.random.default_rng(seed); cell = 0.05
    pos, f, cells = _one_per_cell(T, rng, cell)
    return _done(_finish(pos, f, cells, order, rng), cell)


def speck(T, seed=0, order="ascending"):
    """`singles` with a tetrahedron inside one cell of its own in the middle of the numbering: four collapsed faces, a cluster no face uses"""
    rng = np.random.default_rng(seed); cell = 0.05
    pos, f, cells = _one_per_cell(T, rng, cell)
    h = len(pos) // 2
    tcell = np.tile([[5, -7, 3]], (4, 1))
    pos = np.concatenate([pos[:h], _inside(tcell, cell, rng), pos[h:]]); cells = np.concatenate([cells[:h], tcell, cells[h:]])
    f = np.where(f >= h, f + 4, f)
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int64) + h
    f = np.concatenate([f[:len(f) // 2], tet, f[len(f) // 2:]])
    return _done(_finish(pos, f, cells, order, rng), cell)


def isolated(T, seed=0, order="ascending"):
    """`singles` plus one vertex no face uses inside the cell of every second vertex: it counts in n and in the mean"""
    rng = np.random.default_rng(seed); cell = 0.05
    pos, f, cells = _one_per_cell(T, rng, cell)
    extra = cells[::2]
    return _done(_finish(np.concatenate([pos, _inside(extra, cell, rng)]), f, np.concatenate([cells, extra]), order, rng), cell)


PLANTED = ("grid", "straddle", "boundary", "hub", "sheets", "singles", "speck", "isolated")
# the families of mesh_clean_ref.build as generic input (moved by +3 so that one cell of 8 m can hold all of it): a cell below the edge lengths, one about three
# edge lengths, one that swallows the mesh (one cluster: 0 vertices and 0 faces come out)
GENERIC_CELLS = {"fine": 0.0005, "coarse": 0.03, "swallow": 8.0}
FAMILIES = PLANTED + tuple("%s@%s" % (f, c) for f in mesh_clean_ref.FAMILIES for c in GENERIC_CELLS)


def build(family, T, seed=0, order="ascending"):
    """-> (positions, colours, faces, cell size, labels or None)"""
    if "@" in family:
        name, c = family.split("@")
        pos, col, faces = mesh_clean_ref.build(name, T, seed, order)
        return (pos + np.float32(3.0)).astype(np.float32), col, faces, GENERIC_CELLS[c], None
    return globals()[family](T, seed, order)


def ply_bytes(pos, normals, col, faces):
    return mesh_clean_ref.ply_bytes_normals(pos, normals, col, faces)
