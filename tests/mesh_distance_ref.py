"""Numpy binary64 restatement of the mesh distance (DESIGN.md "Mesh distance: the definition"; include/bf_hip.h next to bf_marching_cubes_distance): Ericson's
closest point vectorised with np.where, a brute-force minimum over ALL faces of B with no grid, the sums in Python integers.  numpy's elementwise binary64
operations round once each and never contract, which is the definition's arithmetic, so the library is held to this as bits."""
import math
import struct

import numpy as np

NONE = 0xFFFFFFFF
BINS = 1024


def dot3(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross_norm2(a, b, c):
    u, v = b - a, c - a
    n = np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2], u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)
    return dot3(n, n)


def corners(pos, faces):
    """(a, b, c) binary64 [nf,3] and the degenerate mask"""
    pos = np.asarray(pos, np.float32).reshape(-1, 3).astype(np.float64); faces = np.asarray(faces, np.uint32).reshape(-1, 3).astype(np.int64)
    a, b, c = pos[faces[:, 0]], pos[faces[:, 1]], pos[faces[:, 2]]
    with np.errstate(all="ignore"):
        n2 = cross_norm2(a, b, c)
    return a, b, c, n2, ~((n2 > 0) & (n2 < np.inf))


def tri_dist2(p, a, b, c):
    """d2 of points p [N,1,3] to triangles a, b, c [1,M,3]: [N,M]"""
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot3(ab, ap), dot3(ac, ap), dot3(ab, bp), dot3(ac, bp), dot3(ab, cp), dot3(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = 1.0 / ((va + vb) + vc)
        q = (a + ab * (vb * den)[..., None]) + ac * (vc * den)[..., None]
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        q = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + t[..., None] * (c - b), q)
        t = d2 / (d2 - d6)
        q = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + t[..., None] * ac, q)
        q = np.where(((d6 >= 0) & (d5 <= d6))[..., None], c + 0 * p, q)
        t = d1 / (d1 - d3)
        q = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + t[..., None] * ab, q)
        q = np.where(((d3 >= 0) & (d4 <= d3))[..., None], b + 0 * p, q)
        q = np.where(((d1 <= 0) & (d2 <= 0))[..., None], a + 0 * p, q)
        r = p - q
        return dot3(r, r)


def samples(pos, faces, mode, spacing):
    """(points [N,3] binary64, weights [N], number of degenerate faces) of mesh A"""
    a, b, c, n2, deg = corners(pos, faces)
    if mode == 0:
        p = np.asarray(pos, np.float32).reshape(-1, 3).astype(np.float64)
        return p, np.ones(len(p)), int(deg.sum())
    spacing = float(np.float32(spacing))
    if spacing == 0.0:                                   # n = 1 everywhere: the loop below, all faces at once
        a, b, c, n2 = a[~deg], b[~deg], c[~deg], n2[~deg]
        u = 1.0 / 3.0
        return (a + u * (b - a)) + u * (c - a), (0.5 * np.sqrt(n2)) / 1.0, int(deg.sum())
    pts, wts = [], []
    for f in np.nonzero(~deg)[0]:
        e = [b[f] - a[f], c[f] - a[f], c[f] - b[f]]
        L = math.sqrt(max(float(dot3(x, x)) for x in e))
        n = 1 if spacing == 0.0 else max(1, int(math.ceil(L / spacing)))
        k = np.arange(n * n, dtype=np.int64)
        m = n * n - k
        r = np.ceil(np.sqrt(m.astype(np.float64))).astype(np.int64)
        r = np.where((r - 1) * (r - 1) >= m, r - 1, r); r = np.where(r * r < m, r + 1, r)
        j, t = n - r, k - (n * n - r * r)
        i, up = t // 2, np.where(t & 1, 2, 1)
        u = (3 * i + up).astype(np.float64) / float(3 * n); v = (3 * j + up).astype(np.float64) / float(3 * n)
        pts.append((a[f] + u[:, None] * (b[f] - a[f])) + v[:, None] * (c[f] - a[f]))
        wts.append(np.full(n * n, (0.5 * math.sqrt(float(n2[f]))) / float(n * n)))
    if not pts:
        return np.zeros((0, 3)), np.zeros(0), int(deg.sum())
    return np.concatenate(pts), np.concatenate(wts), int(deg.sum())


def scales(num_samples, mode, D):
    L = 0
    while (1 << L) < num_samples:
        L += 1
    e = -20
    while e < 6 and D > 2.0 ** e:
        e += 1
    kw = 62 - L - (6 if mode else 0)
    return kw, kw - e, kw - 2 * e


def q(x, k):
    return int(math.floor(x * 2.0 ** k + 0.5))


def stats_of(dist, weight, max_distance, mode, deg_a, deg_b):
    """the summary of per-sample results, in Python integers"""
    D = float(np.float32(max_distance))
    kw, kwd, kwd2 = scales(len(dist), mode, D)
    st = dict(numSamples=len(dist), numWithin=0, numBeyond=0, numDegenerateA=deg_a, numDegenerateB=deg_b, maxWithin=0.0, sumW=0, sumWD=0, sumWD2=0, sumWBeyond=0,
              scaleW=kw, scaleWD=kwd, scaleWD2=kwd2, max_distance=D)
    hist = [0] * BINS
    bin_scale = 1024.0 / D
    for d, w in zip(dist.tolist(), weight.tolist()):
        if d < math.inf:
            wd = w * d
            st["numWithin"] += 1; st["sumW"] += q(w, kw); st["sumWD"] += q(wd, kwd); st["sumWD2"] += q(wd * d, kwd2)
            st["maxWithin"] = max(st["maxWithin"], d)
            hist[min(BINS - 1, int(math.floor(d * bin_scale)))] += q(w, kw)
        else:
            st["numBeyond"] += 1; st["sumWBeyond"] += q(w, kw)
    assert all(abs(st[k]) < 2 ** 63 for k in ("sumW", "sumWD", "sumWD2", "sumWBeyond"))
    st["histogram"] = np.array(hist, np.int64)
    return st


def nearest(p, B, chunk=1 << 21):
    """(minimum d2, its lowest face index or NONE, number of degenerate faces) of binary64 points p [N,3] over all faces of B"""
    a, b, c, _, deg = corners(B[0], B[1])
    live = np.nonzero(~deg)[0]
    a, b, c = a[live][None], b[live][None], c[live][None]
    N = len(p)
    best = np.full(N, np.inf); face = np.full(N, NONE, np.uint32)
    step = max(1, chunk // max(1, len(live)))
    if len(live):
        for s in range(0, N, step):
            d2 = tri_dist2(p[s:s + step, None, :], a, b, c)
            k = np.argmin(d2, axis=1)                     # the first of equal minima: the lowest face index (live is increasing)
            best[s:s + step] = d2[np.arange(len(k)), k]; face[s:s + step] = live[k]
    return best, face, int(deg.sum())


def distance(A, B, max_distance, sample_spacing=0.0, sample_mode=0):
    """(distance, nearest face, weight, stats) of mesh A = (positions, faces) against the surface B: every sample against every face"""
    D = float(np.float32(max_distance))
    p, w, deg_a = samples(A[0], A[1], sample_mode, sample_spacing)
    best, face, deg_b = nearest(p, B)
    within = (face != NONE) & (best <= D * D)
    dist = np.where(within, np.sqrt(np.where(within, best, 0.0)), np.inf)
    face = np.where(within, face, NONE).astype(np.uint32)
    return dist, face, w, stats_of(dist, w, max_distance, sample_mode, deg_a, deg_b)


def same(got, want):
    """two (distance, face, weight, stats): distances and weights as uint64 bit patterns, faces, stats and histograms exactly"""
    for k, name in enumerate(("distance", "face", "weight")):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if g.shape != w.shape:
            return "%s: shapes %r %r" % (name, g.shape, w.shape)
        gb, wb = (g.view(np.uint64), w.view(np.uint64)) if g.dtype == np.float64 else (g, w)
        if not np.array_equal(gb, wb):
            i = int(np.nonzero(gb != wb)[0][0])
            return "%s differs at %d of %d: %r != %r (%d in all)" % (name, i, len(g), g[i], w[i], int((gb != wb).sum()))
    gs, ws = got[3], want[3]
    for key in ws:
        if key == "histogram":
            if not np.array_equal(gs[key], ws[key]):
                return "histogram differs"
        elif key == "maxWithin":
            if struct.pack("<d", gs[key]) != struct.pack("<d", ws[key]):
                return "maxWithin %r != %r" % (gs[key], ws[key])
        elif gs[key] != ws[key]:
            return "stats[%s]: %r != %r" % (key, gs[key], ws[key])
    return None


# ---- planted meshes
def soup(num_faces, seed, lo=-1.0, hi=1.0, edge=0.3):
    """a random triangle soup on both sides of zero: (positions [3 nf, 3] float32, faces [nf, 3] uint32); face ids shuffled over the vertices"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(lo, hi, (num_faces, 1, 3))
    pos = (centre + rng.uniform(-edge, edge, (num_faces, 3, 3))).reshape(-1, 3).astype(np.float32)
    perm = rng.permutation(3 * num_faces)
    inv = np.empty_like(perm); inv[perm] = np.arange(3 * num_faces)
    return pos[perm], inv.reshape(num_faces, 3).astype(np.uint32)


def sheet(n, size=1.0, z=0.0, x0=-0.5, y0=-0.5):
    """an n x n grid of squares cut into 2 n^2 triangles at height z"""
    g = np.arange(n + 1, dtype=np.float64) * (size / n)
    xs, ys = np.meshgrid(g + x0, g + y0, indexing="ij")
    pos = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, z)], 1).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = (i * (n + 1) + j).ravel()
    faces = np.concatenate([np.stack([v, v + n + 1, v + 1], 1), np.stack([v + 1, v + n + 1, v + n + 2], 1)]).astype(np.uint32)
    return pos, faces


def error_ply_bytes(pos, faces, dist, max_distance):
    """the file bf_write_ply_indexed_error writes"""
    pos = np.asarray(pos, np.float32).reshape(-1, 3); faces = np.asarray(faces, np.uint32).reshape(-1, 3)
    D = np.float32(max_distance)
    d = np.asarray(dist, np.float64)
    ok = d <= np.float64(D)
    with np.errstate(all="ignore"):
        t = (np.where(ok, d, 0.0) / np.float64(D)).astype(np.float32)
    s = np.float32(2) * t - np.float32(1)
    col = np.stack([np.maximum(np.float32(0), s), np.float32(1) - np.abs(s), np.maximum(np.float32(0), np.float32(1) - np.float32(2) * t)], 1).astype(np.float32)
    col[~ok] = (1.0, 0.0, 1.0)
    head = ("ply\nformat binary_little_endian 1.0\ncomment bundlefusion_amd marching cubes\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(pos), len(faces)))
    vrec = np.zeros(len(pos), np.dtype([("p", "<f4", 3), ("c", "u1", 4)]))
    vrec["p"] = pos
    vrec["c"][:, :3] = np.maximum(np.float32(0), np.minimum(np.float32(255), col * np.float32(255) + np.float32(0.5))).astype(np.uint8)
    vrec["c"][:, 3] = 255
    frec = np.zeros(len(faces), np.dtype([("n", "u1"), ("v", "<u4", 3)]))
    frec["n"] = 3; frec["v"] = faces
    return head.encode() + vrec.tobytes() + frec.tobytes()
