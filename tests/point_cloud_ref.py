"""The point cloud's definition (DESIGN.md 1 "Point cloud") restated in numpy, twice: `build` vectorised over all frames at once, `build_loop` as the sequential
per-pixel loop with a dictionary on the cell triple.  The library's host route, its device object and its file are compared with these as bits.

What the reference does (cited, not copied): SiftVisualization::saveToPointCloud (SiftVisualization.cpp:607-644) walks every skip-th frame, computePointCloud
(:527-561) skips a frame whose pose starts with -inf (:531), back-projects each pixel with depthToCamera (:498-503), takes getNormal's cross product of the
central differences (:505-525), drops black pixels (:543) and points at or beyond maxDepth, moves point and normal into the world (:556-560), and
pc.sparsifyUniform(0.005f, true) (:640) thins the union; RGBDSensor::recordPointCloud / saveRecordedPointCloud (RGBDSensor.cpp:528-616) do the same per frame.

All arithmetic is binary32, one rounding per operation; the cell is one binary64 multiply and a floor.
"""
import numpy as np

F = np.float32
KEPT, NO_POSITION, MAX_DEPTH, BORDER, NEIGHBOUR, NORMAL, COLOUR, WORLD, CELL_RANGE, POSE = range(10)
RULES = ("kept", "no position", "maxDepth", "border", "neighbour", "normal", "colour", "world", "cell range", "pose")


def cell_inverse(cell_size):
    """1.0 / (double)cellSize, or None for cellSize <= 0 (no thinning)"""
    c = float(F(cell_size))
    return 1.0 / c if c > 0.0 else None


def pose_invalid(T):
    t0 = F(np.asarray(T, F).reshape(-1)[0])
    return bool(np.isnan(t0) or t0 == F(-np.inf))


def _dot(r, a, b, c, d):
    return ((r[0] * a + r[1] * b) + r[2] * c) + r[3] * d


def frame_candidates(D, C, Kinv, T, cell_size, max_depth):
    """One frame, vectorised.  Returns (reason (h, w) int, P (h, w, 3) f32, N (h, w, 3) f32, rgba (h, w, 4) u8); reason == KEPT marks the candidates, any other
    value names the first rule of the definition, in its order, that drops the pixel."""
    D = np.asarray(D, F); C = np.asarray(C, np.uint8); K = np.asarray(Kinv, F).reshape(4, 4); T = np.asarray(T, F).reshape(4, 4)
    h, w = D.shape
    reason = np.zeros((h, w), np.int64)
    if pose_invalid(T):
        reason[:] = POSE
        return reason, np.zeros((h, w, 3), F), np.zeros((h, w, 3), F), np.zeros((h, w, 4), np.uint8)
    inv = cell_inverse(cell_size)
    with np.errstate(all="ignore"):
        has = np.isfinite(D) & (D > 0)
        d = np.where(has, D, F(0))
        x = np.arange(w, dtype=F)[None, :] * np.ones((h, 1), F); y = np.arange(h, dtype=F)[:, None] * np.ones((1, w), F)
        xd = x * d; yd = y * d
        one = np.ones_like(d)
        p = [_dot(K[i], xd, yd, d, one) for i in range(3)]
        interior = np.zeros((h, w), bool)
        if h >= 3 and w >= 3:
            interior[1:-1, 1:-1] = True
        xm = lambda a: np.roll(a, 1, axis=1); xp = lambda a: np.roll(a, -1, axis=1)          # value at (x-1, y) / (x+1, y); the wrap touches the border only
        ym = lambda a: np.roll(a, 1, axis=0); yp = lambda a: np.roll(a, -1, axis=0)
        nb = xm(has) & xp(has) & ym(has) & yp(has)
        a = [xp(q) - xm(q) for q in p]; b = [yp(q) - ym(q) for q in p]
        n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        l = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        ml = -l
        nn = [q / ml for q in n]
        P = [_dot(T[i], p[0], p[1], p[2], one) for i in range(3)]
        N = [(T[i, 0] * nn[0] + T[i, 1] * nn[1]) + T[i, 2] * nn[2] for i in range(3)]
        finite = np.isfinite(P[0]) & np.isfinite(P[1]) & np.isfinite(P[2])
        in_range = np.ones((h, w), bool)
        if inv is not None:
            for q in P:
                c = np.floor(np.where(finite, q, F(0)).astype(np.float64) * inv)
                in_range &= (c >= -2147483648.0) & (c <= 2147483647.0)
        black = (C[..., 0] == 0) & (C[..., 1] == 0) & (C[..., 2] == 0)
        # last rule first, so that the first rule that fails is the one that stays
        for code, bad in ((CELL_RANGE, ~in_range), (WORLD, ~finite), (COLOUR, black), (NORMAL, ~(np.isfinite(l) & (l > 0))), (NEIGHBOUR, ~nb), (BORDER, ~interior),
                          (MAX_DEPTH, ~(p[2] < F(max_depth))), (NO_POSITION, ~has)):
            reason[bad] = code
    rgba = C.copy(); rgba[..., 3] = 255
    return reason, np.stack(P, -1).astype(F), np.stack(N, -1).astype(F), rgba


def cells_of(P, cell_size):
    return np.floor(np.asarray(P, F).astype(np.float64) * cell_inverse(cell_size)).astype(np.int64)


def build(frames, Kinv, cell_size, max_depth):
    """frames: sequence of (depth, colour, pose).  Returns (positions (n, 3) f32, normals (n, 3) f32, colours (n, 4) u8, numCandidates)."""
    Ps, Ns, Cs = [np.zeros((0, 3), F)], [np.zeros((0, 3), F)], [np.zeros((0, 4), np.uint8)]
    for D, C, T in frames:
        reason, P, N, rgba = frame_candidates(D, C, Kinv, T, cell_size, max_depth)
        m = reason == KEPT                                   # boolean indexing keeps raster order
        Ps.append(P[m]); Ns.append(N[m]); Cs.append(rgba[m])
    P, N, C = np.concatenate(Ps), np.concatenate(Ns), np.concatenate(Cs)
    if cell_inverse(cell_size) is not None and len(P):
        _, first = np.unique(cells_of(P, cell_size), axis=0, return_index=True)          # the index of each cell's first occurrence: its lowest candidate number
        keep = np.sort(first)
        return P[keep], N[keep], C[keep], len(P)
    return P, N, C, len(P)


def build_loop(frames, Kinv, cell_size, max_depth):
    """the same as one sequential loop: frames in order, pixels in raster order, scalars only; the first candidate of a cell stays"""
    K = np.asarray(Kinv, F).reshape(4, 4)
    inv = cell_inverse(cell_size)
    md = F(max_depth)
    cells = {}
    out_p, out_n, out_c = [], [], []
    num_candidates = 0
    one = F(1)

    def dot(r, a, b, c, d):
        return F(F(F(F(r[0] * a) + F(r[1] * b)) + F(r[2] * c)) + F(r[3] * d))

    with np.errstate(all="ignore"):
        for D, C, T in frames:
            D = np.asarray(D, F); C = np.asarray(C, np.uint8); T = np.asarray(T, F).reshape(4, 4)
            if pose_invalid(T):
                continue
            h, w = D.shape

            def has(x, y):
                return bool(np.isfinite(D[y, x]) and D[y, x] > 0)

            def pos(x, y):
                d = D[y, x]
                xd = F(F(x) * d); yd = F(F(y) * d)
                return [dot(K[i], xd, yd, d, one) for i in range(3)]

            for y in range(1, h - 1):
                for x in range(1, w - 1):
                    if not (has(x, y) and has(x - 1, y) and has(x + 1, y) and has(x, y - 1) and has(x, y + 1)):
                        continue
                    p = pos(x, y)
                    if not p[2] < md:
                        continue
                    xm, xp, ym, yp = pos(x - 1, y), pos(x + 1, y), pos(x, y - 1), pos(x, y + 1)
                    a = [F(xp[i] - xm[i]) for i in range(3)]; b = [F(yp[i] - ym[i]) for i in range(3)]
                    n = [F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])), F(F(a[0] * b[1]) - F(a[1] * b[0]))]
                    l = F(np.sqrt(F(F(F(n[0] * n[0]) + F(n[1] * n[1])) + F(n[2] * n[2]))))
                    if not (np.isfinite(l) and l > 0):
                        continue
                    if C[y, x, 0] == 0 and C[y, x, 1] == 0 and C[y, x, 2] == 0:
                        continue
                    ml = F(-l)
                    nn = [F(q / ml) for q in n]
                    P = [dot(T[i], p[0], p[1], p[2], one) for i in range(3)]
                    if not all(np.isfinite(q) for q in P):
                        continue
                    if inv is not None:
                        cell = tuple(int(np.floor(float(q) * inv)) for q in P)
                        if not all(-2 ** 31 <= c <= 2 ** 31 - 1 for c in cell):
                            continue
                    N = [F(F(F(T[i, 0] * nn[0]) + F(T[i, 1] * nn[1])) + F(T[i, 2] * nn[2])) for i in range(3)]
                    num_candidates += 1
                    if inv is not None:
                        if cell in cells:
                            continue
                        cells[cell] = len(out_p)
                    out_p.append(P); out_n.append(N); out_c.append([C[y, x, 0], C[y, x, 1], C[y, x, 2], 255])
    return (np.array(out_p, F).reshape(-1, 3), np.array(out_n, F).reshape(-1, 3), np.array(out_c, np.uint8).reshape(-1, 4), num_candidates)


def ply_bytes(positions, normals, colours):
    """the file of bf_write_ply_points, assembled here: the header and one 28-byte record per point"""
    n = len(positions)
    head = ("ply\nformat binary_little_endian 1.0\ncomment bundlefusion_amd point cloud\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n" % n)
    rec = np.zeros(n, np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 4)]))
    assert rec.dtype.itemsize == 28
    rec["p"] = np.asarray(positions, F).reshape(n, 3); rec["n"] = np.asarray(normals, F).reshape(n, 3); rec["c"] = np.asarray(colours, np.uint8).reshape(n, 4)
    return head.encode() + rec.tobytes()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
