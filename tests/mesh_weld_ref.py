"""Numpy restatement of the mesh weld (bf_marching_cubes_save_mesh / bf_marching_cubes_weld) and of the PLY writer, independent of the product; the yardstick of
tests/test_mesh_weld_cpu.py and tests/test_mesh_weld_gpu.py.

Definition (corner 3 * t + c = corner c of triangle t):
  * key of a corner: (int64)floor((double)p * (1.0 / 0.00001) + 0.5) per axis, in binary64, a multiply then an add;
  * the vertex of a key is its lowest-numbered corner; vertex ids count those representatives in increasing corner number (the order of first occurrence);
    position and colour are the representative's; corners of faces that are dropped still make vertices;
  * a face whose ids are not pairwise different is dropped; of the others with the same sorted id triple the one with the lowest triangle index is kept; kept faces
    stay in triangle order with their winding;
  * an optional 4x4 transform is applied to the welded positions, op by op in binary32: ((m0 * x + m1 * y) + m2 * z) + m3 * 1.

Two forms: weld() is vectorised (np.unique finds first occurrences and ranks them), weld_sequential() is the plain dictionary loop of the host code."""
import numpy as np

INV = 1.0 / 0.00001


def corner_keys(tris):
    p = np.ascontiguousarray(tris, np.float32).reshape(-1, 6)[:, :3].astype(np.float64)
    return np.floor(p * INV + 0.5).astype(np.int64)


def xform(T, pos):
    T = np.asarray(T, np.float32).reshape(4, 4)
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    out = np.empty_like(pos)
    for r in range(3):
        out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] * np.float32(1.0)
    return out


def _first_occurrence_ids(rows):
    """per row the rank of its value among the distinct values ordered by first occurrence; and the first-occurrence row of every rank"""
    _, first, inv = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(first), np.int64); rank[order] = np.arange(len(first))
    return rank[np.asarray(inv).reshape(-1)], first[order]


def weld(tris, transform=None):
    """(positions [nv,3] float32, colours [nv,3] float32, faces [nf,3] uint32) of triangles [T,3,6] float32"""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 6)
    if len(tris) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)
    corners = tris.reshape(-1, 6)
    vid, reps = _first_occurrence_ids(corner_keys(tris))
    pos, col = corners[reps, :3].copy(), corners[reps, 3:].copy()
    ids = vid.reshape(-1, 3)
    proper = np.nonzero((ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2]))[0]
    if len(proper):
        _, first = _first_occurrence_ids(np.sort(ids[proper], axis=1))
        faces = ids[proper[first]]
    else:
        faces = np.zeros((0, 3), np.int64)
    if transform is not None:
        pos = xform(transform, pos)
    return pos, col, faces.astype(np.uint32)


def weld_sequential(tris, transform=None):
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 6)
    grid, pos, col, faces, seen = {}, [], [], [], set()
    for t in tris:
        f = []
        for v in t:
            k = tuple(int(np.floor(np.float64(v[c]) * INV + 0.5)) for c in range(3))
            if k not in grid:
                grid[k] = len(pos); pos.append(v[:3]); col.append(v[3:])
            f.append(grid[k])
        if f[0] == f[1] or f[1] == f[2] or f[0] == f[2]:
            continue
        s = tuple(sorted(f))
        if s in seen:
            continue
        seen.add(s); faces.append(f)
    pos = np.array(pos, np.float32).reshape(-1, 3); col = np.array(col, np.float32).reshape(-1, 3)
    if transform is not None:
        pos = xform(transform, pos)
    return pos, col, np.array(faces, np.uint32).reshape(-1, 3)


def ply_bytes(pos, col, faces):
    """the file bf_write_ply_indexed writes"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); col = np.ascontiguousarray(col, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    head = ("ply\nformat binary_little_endian 1.0\ncomment bundlefusion_amd marching cubes\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n"
            % (len(pos), len(faces))).encode()
    v = np.zeros(len(pos), np.dtype([("p", "<f4", 3), ("c", "u1", 4)]))
    v["p"] = pos
    scaled = col * np.float32(255.0) + np.float32(0.5)                       # binary32, a multiply then an add
    v["c"][:, :3] = np.maximum(np.float32(0.0), np.minimum(np.float32(255.0), scaled)).astype(np.uint8)          # truncation
    v["c"][:, 3] = 255
    f = np.zeros(len(faces), np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    f["n"] = 3; f["i"] = faces.view(np.int32)
    assert v.dtype.itemsize == 16 and f.dtype.itemsize == 13
    return head + v.tobytes() + f.tobytes()


# --------------------------------------------------------------------------- planted soups
# A cell is an integer triple m; a corner "in" it sits at m * 1e-5 plus a jitter of at most 0.3 cells, which the rounding to binary32 (below 1e-7 for |x| < 1 m)
# cannot carry over the cell's edge at +-0.5.
def _in_cells(rng, cells):
    p = (cells.astype(np.float64) + rng.uniform(-0.3, 0.3, cells.shape)) * 1e-5
    return p.astype(np.float32)


def _soup(pos, rng):
    """triangles [T,3,6] from corner positions [3T,3]: every corner gets a colour of its own (so "which corner represents the vertex" shows)"""
    n = len(pos)
    col = ((np.arange(n, dtype=np.float64)[:, None] * [0.618033988, 0.414213562, 0.732050807] + rng.uniform(0, 1e-3, (n, 3))) % 1.0).astype(np.float32)
    return np.concatenate([pos, col], axis=1).reshape(-1, 3, 6)


def soup_one_cell(T, seed=0):
    """(a) every corner in one cell: 1 vertex, 0 faces"""
    rng = np.random.default_rng(seed)
    return _soup(_in_cells(rng, np.tile(np.array([[1234, -777, 40000]]), (3 * T, 1))), rng)


def soup_copies(T, seed=0):
    """(b) every triangle is the first one again, jittered inside its cells, rotated or reflected: 3 vertices, 1 face"""
    rng = np.random.default_rng(seed)
    base = np.array([[100, 200, 300], [4100, 250, 300], [130, 5200, -900]])
    perms = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]])
    pick = perms[rng.integers(0, 6, T)]
    if T:
        pick[0] = [0, 1, 2]
    return _soup(_in_cells(rng, base[pick].reshape(-1, 3)), rng)


def soup_pool(T, seed=0, cells=60):
    """(c) corners drawn from a pool of `cells` cells: every key is contended by 3T / cells corners spread over the whole corner range"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(-40000, 40000, (cells, 3))
    return _soup(_in_cells(rng, pool[rng.integers(0, cells, 3 * T)]), rng)


def soup_distinct(T, seed=0):
    """(d) all keys distinct: 3T vertices, T faces"""
    rng = np.random.default_rng(seed)
    n = 3 * T
    m = np.zeros((0, 3), np.int64)
    while len(m) < n:
        m = np.unique(np.concatenate([m, rng.integers(-60000, 60000, (n + 16, 3))]), axis=0)
    return _soup(_in_cells(rng, rng.permutation(m)[:n]), rng)


def soup_range(T, seed=0):
    """(e) coordinates over +-50 m, negative ones included, a third of the corners exact copies of pool points (binary32 is coarser than a cell out there)"""
    rng = np.random.default_rng(seed)
    n = 3 * T
    pos = rng.uniform(-50.0, 50.0, (n, 3)).astype(np.float32)
    pool = np.concatenate([rng.uniform(-50.0, 50.0, (40, 3)), [[50.0, -50.0, 49.99999], [-50.0, 50.0, -49.99999]]]).astype(np.float32)
    take = rng.random(n) < 1.0 / 3.0
    pos[take] = pool[rng.integers(0, len(pool), int(take.sum()))]
    return _soup(pos, rng)


def boundary_values():
    """(f) binary32 coordinates whose product with 1e5 is k + 0.5 in exact arithmetic - (2k + 1) / 200000 is a binary32 number exactly when it is j / 64, j odd -
    and their two binary32 neighbours on either side: which cell they fall in is decided by the rounding of the binary64 multiply and add"""
    j = np.arange(-199, 200, 2, dtype=np.float64)
    x = (j / 64.0).astype(np.float32)
    vals = [x]
    up, dn = x, x
    for _ in range(2):
        up = np.nextafter(up, np.float32(np.inf)); dn = np.nextafter(dn, np.float32(-np.inf))
        vals += [up, dn]
    return np.concatenate(vals).astype(np.float32)


def soup_boundaries(T, seed=0):
    rng = np.random.default_rng(seed)
    v = boundary_values()
    n = 3 * T
    pos = v[rng.integers(0, 3, (n, 3)) * 7]          # two axes from three values, so that corners meet ...
    axis = np.arange(n) % 3
    pos[np.arange(n), axis] = v[rng.integers(0, len(v), n)]          # ... and one axis from all of them: neighbours either side of an edge end up in one cell or in two
    return _soup(pos.astype(np.float32).reshape(-1, 3), rng)


def soup_mixed(T, seed=0):
    """copies, rotations and reflections of pool triangles next to triangles of their own: every rule at once"""
    rng = np.random.default_rng(seed)
    if T == 0:
        return np.zeros((0, 3, 6), np.float32)
    a = soup_pool(T, seed, cells=max(8, T // 7))[:, :, :3]
    src = rng.integers(0, T, T); dup = rng.random(T) < 0.3
    perms = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]])
    b = a[src[:, None], perms[rng.integers(0, 6, T)]]
    a = np.where(dup[:, None, None], b, a)
    own = rng.random(T) < 0.3
    a = np.where(own[:, None, None], soup_distinct(T, seed + 1)[:, :, :3], a)
    return _soup(a.reshape(-1, 3), rng)


TRANSFORM = np.array([[0.36, 0.48, -0.8, 0.1], [-0.8, 0.6, 0.0, -0.2], [0.48, 0.64, 0.6, 0.3], [0.0, 0.0, 0.0, 1.0]], np.float32)      # a rotation + translation; no entry but 0 and 1 is a binary32 number
