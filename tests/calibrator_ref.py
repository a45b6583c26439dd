"""The depth-registration operator's definition (DESIGN.md "Depth registration") restated in numpy: binary32 op by op in the vertex stage
(the library is built without contraction and with IEEE division, so the same sequence gives the same bits), integers in the raster stage.
Vectorised over triangles; every triangle walks a bounding box padded to the largest one of the image.

register(depth, Kc, KdInv, E, thresh_offset, thresh_lin) -> float32 (h, w): the depth seen from the colour camera, -inf where nothing was drawn.
quad_survives(depth, thresh_offset, thresh_lin) -> bool (h, w): the quad stage alone.
"""
import numpy as np

F = np.float32
Z_NEAR, Z_FAR = F(0.1), F(20.0)
UV_LIMIT = F(1048576.0)


def _corners(depth):
    """the four corner depths of every quad (x, y): (x,y) (x,y+1) (x+1,y) (x+1,y+1); outside the image reads 0"""
    h, w = depth.shape
    p = np.zeros((h + 1, w + 1), np.float32)
    p[:h, :w] = depth
    return p[:h, :w], p[1:, :w], p[:h, 1:], p[1:, 1:]


def _depth_ok(d):
    with np.errstate(invalid="ignore"):
        return (d > Z_NEAR) & (d < F(np.inf))


def quad_survives(depth, thresh_offset, thresh_lin):
    depth = np.ascontiguousarray(depth, np.float32)
    d0, d1, d2, d3 = _corners(depth)
    ok = _depth_ok(d0) & _depth_ok(d1) & _depth_ok(d2) & _depth_ok(d3)
    z = [np.where(ok, d, F(1.0)) for d in (d0, d1, d2, d3)]
    dmax = np.maximum(np.maximum(z[0], z[1]), np.maximum(z[2], z[3]))
    dmin = np.minimum(np.minimum(z[0], z[1]), np.minimum(z[2], z[3]))
    return ok & ~(dmax - dmin > F(thresh_offset) + F(thresh_lin) * (F(0.5) * (dmax + dmin)))


def _dot4(m, a, b, c, d):
    return ((m[0] * a + m[1] * b) + m[2] * c) + m[3] * d


def project_vertices(depth, Kc, KdInv, E):
    """every pixel as a mesh vertex -> (ok, U, V, z): position in 1/256 pixel and depth in the colour camera"""
    depth = np.ascontiguousarray(depth, np.float32)
    Kc, KdInv, E = (np.asarray(m, np.float32).reshape(4, 4) for m in (Kc, KdInv, E))
    h, w = depth.shape
    ok = _depth_ok(depth)
    d = np.where(ok, depth, F(1.0))
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    one = F(1.0)
    with np.errstate(all="ignore"):
        xd, yd = x * d, y * d
        px, py, pz = _dot4(KdInv[0], xd, yd, d, d), _dot4(KdInv[1], xd, yd, d, d), _dot4(KdInv[3], xd, yd, d, d)
        ex, ey, ez, ew = (_dot4(E[i], px, py, pz, one) for i in range(4))
        wx, wy, wz = ex / ew, ey / ew, ez / ew
        qx, qy, qz = (_dot4(Kc[i], wx, wy, wz, one) for i in range(3))
        u, v = qx / qz, qy / qz
        ok = ok & (qz > Z_NEAR) & (qz < Z_FAR) & (np.abs(u) < UV_LIMIT) & (np.abs(v) < UV_LIMIT)
        u, v = np.where(ok, u, F(0.0)), np.where(ok, v, F(0.0))
        U = np.floor(u * F(256.0) + F(0.5)).astype(np.int64)
        V = np.floor(v * F(256.0) + F(0.5)).astype(np.int64)
    for a in (xd, px, ex, wx, qx, u):
        assert a.dtype == np.float32
    return ok, U, V, np.where(ok, qz, F(0.0)).astype(np.float32)


def _edge(aU, aV, bU, bV, pU, pV):
    return (bU - aU) * (pV - aV) - (bV - aV) * (pU - aU)


def _top_left(aU, aV, bU, bV):
    dU, dV = bU - aU, bV - aV
    return (dV < 0) | ((dV == 0) & (dU > 0))


def _raster(out, w, h, tri):
    """tri: three (U, V, z) tuples of 1-D arrays, positive orientation expected.  out: float32 (h*w), minimum kept."""
    (aU, aV, az), (bU, bV, bz), (cU, cV, cz) = tri
    if aU.size == 0:
        return
    area2 = _edge(aU, aV, bU, bV, cU, cV)
    keep = area2 > 0
    aU, aV, az, bU, bV, bz, cU, cV, cz = (t[keep] for t in (aU, aV, az, bU, bV, bz, cU, cV, cz))
    if aU.size == 0:
        return
    i0 = np.maximum(-((-np.minimum(np.minimum(aU, bU), cU)) // 256), 0)          # ceil
    i1 = np.minimum(np.maximum(np.maximum(aU, bU), cU) // 256, w - 1)            # floor
    j0 = np.maximum(-((-np.minimum(np.minimum(aV, bV), cV)) // 256), 0)
    j1 = np.minimum(np.maximum(np.maximum(aV, bV), cV) // 256, h - 1)
    keep = (i1 >= i0) & (j1 >= j0)
    aU, aV, az, bU, bV, bz, cU, cV, cz, i0, i1, j0, j1 = (t[keep] for t in (aU, aV, az, bU, bV, bz, cU, cV, cz, i0, i1, j0, j1))
    if aU.size == 0:
        return
    nx, ny = int((i1 - i0).max()) + 1, int((j1 - j0).max()) + 1
    tl0, tl1, tl2 = _top_left(bU, bV, cU, cV), _top_left(cU, cV, aU, aV), _top_left(aU, aV, bU, bV)
    for dj in range(ny):
        for di in range(nx):
            i, j = i0 + di, j0 + dj
            inside = (i <= i1) & (j <= j1)
            pU, pV = i * 256, j * 256
            e0, e1, e2 = _edge(bU, bV, cU, cV, pU, pV), _edge(cU, cV, aU, aV, pU, pV), _edge(aU, aV, bU, bV, pU, pV)
            cov = inside & ((e0 > 0) | ((e0 == 0) & tl0)) & ((e1 > 0) | ((e1 == 0) & tl1)) & ((e2 > 0) | ((e2 == 0) & tl2))
            if not cov.any():
                continue
            f0, f1, f2 = e0[cov].astype(np.float32), e1[cov].astype(np.float32), e2[cov].astype(np.float32)
            val = ((f0 * az[cov] + f1 * bz[cov]) + f2 * cz[cov]) / ((f0 + f1) + f2)
            assert val.dtype == np.float32
            np.minimum.at(out, (j[cov] * w + i[cov]), val)


def register(depth, Kc, KdInv, E, thresh_offset, thresh_lin):
    depth = np.ascontiguousarray(depth, np.float32)
    h, w = depth.shape
    quad = quad_survives(depth, thresh_offset, thresh_lin)
    ok, U, V, z = project_vertices(depth, Kc, KdInv, E)

    def pad(a, fill):
        p = np.full((h + 1, w + 1), fill, a.dtype)
        p[:h, :w] = a
        return p
    okp, Up, Vp, zp = pad(ok, False), pad(U, 0), pad(V, 0), pad(z, F(0.0))

    def vert(dx, dy, sel):
        return okp[dy:dy + h, dx:dx + w][sel], (Up[dy:dy + h, dx:dx + w][sel], Vp[dy:dy + h, dx:dx + w][sel], zp[dy:dy + h, dx:dx + w][sel])
    out = np.full(h * w, np.inf, np.float32)
    # (x, y+1) (x, y) (x+1, y+1)   and   (x+1, y+1) (x, y) (x+1, y)
    for tri in (((0, 1), (0, 0), (1, 1)), ((1, 1), (0, 0), (1, 0))):
        oks, vs = zip(*(vert(dx, dy, quad) for dx, dy in tri))
        good = oks[0] & oks[1] & oks[2]
        _raster(out, w, h, tuple(tuple(t[good] for t in v) for v in vs))
    out[out == np.inf] = -np.inf
    return out.reshape(h, w)
