"""The definition of the mesh recolouring (DESIGN.md "Mesh colour from the key frames: the definition"; include/bf_hip.h) restated in numpy, twice: `recolour`
evaluates the six rules of every (vertex, frame) pair vectorised over the vertices and then walks the frames in the order given; `recolour_loop` is the sequential
per-vertex, per-frame loop on binary32 scalars.  Both return (colours [nv,3] float32, views [nv] uint32, stats dict, codes [nv,K] uint8).  Arithmetic is binary32,
one rounding per operation: every intermediate below is a float32 array or scalar.

A frame is (depth [h,w] float32, colour [h,w,4] uint8, meshToCamera [4,4] float32, cameraCentre [3] float32, skipped); params is a dict with the fields of
bf_mesh_recolour_params; the codes of a skipped frame's pairs stay SKIPPED."""
import numpy as np

from tests import mesh_simplify_ref

VIEW, NORMAL, RANGE, IMAGE, FACING, OCCLUDED, COLOUR = range(7)
SKIPPED = 255
SIGN = np.float32(1.0)          # BF_RECOLOUR_NORMAL_SIGN
STAT_KEYS = ("numVertices", "numRecoloured", "numUnseen", "numFramesUsed", "numFramesSkipped", "maxViews")
F = np.float32


def params(depthMin=0.25, depthMax=8.0, depthTolerance=0.0625, depthToleranceLin=0.0, minCos=0.25, mode=0):
    return dict(depthMin=depthMin, depthMax=depthMax, depthTolerance=depthTolerance, depthToleranceLin=depthToleranceLin, minCos=minCos, mode=mode)


def _finite(x):
    return np.isfinite(x)


def _stats(nv, recoloured, frames, views):
    used = sum(1 for f in frames if not f[4])
    return dict(numVertices=int(nv), numRecoloured=int(recoloured), numUnseen=int(nv - recoloured), numFramesUsed=used, numFramesSkipped=len(frames) - used,
                maxViews=int(views.max()) if nv else 0)


def _frame_pairs(P, N, ok, frame, w, h, K, p):
    """codes, weights and samples of all vertices against one frame"""
    D, C, W, o = (np.ascontiguousarray(frame[0], F), np.ascontiguousarray(frame[1], np.uint8), np.asarray(frame[2], F).reshape(4, 4), np.asarray(frame[3], F).reshape(3))
    fx, fy, cx, cy = F(K[0][0]), F(K[1][1]), F(K[0][2]), F(K[1][2])
    n = len(P)
    px, py, pz = P[:, 0], P[:, 1], P[:, 2]

    def dot(r):
        return ((r[0] * px + r[1] * py) + r[2] * pz) + r[3] * F(1)

    code = np.full(n, VIEW, np.uint8)
    alive = ok.copy()
    code[~ok] = NORMAL

    def gate(passed, name):
        nonlocal alive
        failed = alive & ~passed
        code[failed] = name
        alive = alive & passed

    p0, p1, z = dot(W[0]), dot(W[1]), dot(W[2])
    gate((z >= F(p["depthMin"])) & (z <= F(p["depthMax"])), RANGE)
    u = (p0 * fx) / z + cx
    v = (p1 * fy) / z + cy
    gate((u >= 0) & (u < F(w - 1)) & (v >= 0) & (v < F(h - 1)), IMAGE)
    x0 = np.where(alive, u, 0).astype(np.int32)
    y0 = np.where(alive, v, 0).astype(np.int32)
    a = u - x0.astype(F)
    b = v - y0.astype(F)
    cxv, cyv, czv = o[0] - px, o[1] - py, o[2] - pz
    l = np.sqrt((cxv * cxv + cyv * cyv) + czv * czv)
    gate(_finite(l) & (l > 0), FACING)
    cosv = SIGN * (((N[:, 0] * cxv + N[:, 1] * cyv) + N[:, 2] * czv) / l)
    gate(cosv >= F(p["minCos"]), FACING)
    tol = F(p["depthTolerance"]) + F(p["depthToleranceLin"]) * z
    texels = [(x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)]
    visible = np.ones(n, bool)
    for tx, ty in texels:
        d = D[ty, tx]
        visible &= _finite(d) & (d > 0) & (np.abs(d - z) <= tol)
    gate(visible, OCCLUDED)
    cols = [C[ty, tx, :3] for tx, ty in texels]
    coloured = np.ones(n, bool)
    for c in cols:
        coloured &= ~((c[:, 0] == 0) & (c[:, 1] == 0) & (c[:, 2] == 0))
    gate(coloured, COLOUR)
    wgt = (cosv * cosv) / (z * z)
    c00, c10, c01, c11 = [c.astype(F) for c in cols]
    top = c00 + a[:, None] * (c10 - c00)
    bot = c01 + a[:, None] * (c11 - c01)
    val = top + b[:, None] * (bot - top)
    return code, wgt.astype(F), val.astype(F)


def _vertex_ok(P, N):
    return _finite(P).all(1) & _finite(N).all(1) & ((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2] > 0)


def recolour(pos, nrm, col, frames, w, h, K, p):
    P = np.ascontiguousarray(pos, F).reshape(-1, 3); N = np.ascontiguousarray(nrm, F).reshape(-1, 3); C0 = np.ascontiguousarray(col, F).reshape(-1, 3)
    n, mode = len(P), int(p["mode"])
    codes = np.full((n, len(frames)), SKIPPED, np.uint8)
    S = np.zeros((n, 3), F); SW = np.zeros(n, F); views = np.zeros(n, np.uint32)
    with np.errstate(all="ignore"):
        ok = _vertex_ok(P, N)
        for k, frame in enumerate(frames):
            if frame[4]:
                continue
            code, wgt, val = _frame_pairs(P, N, ok, frame, w, h, K, p)
            codes[:, k] = code
            view = code == VIEW
            if mode == 0:
                S = np.where(view[:, None], S + wgt[:, None] * val, S)
                SW = np.where(view, SW + wgt, SW)
            else:
                take = view & ((views == 0) | (wgt > SW))
                S = np.where(take[:, None], val, S)
                SW = np.where(take, wgt, SW)
            views = views + view.astype(np.uint32)
        if mode == 0:
            done = (views > 0) & _finite(SW) & (SW > 0)
            new = (S / SW[:, None]) / F(255)
        else:
            done = views > 0
            new = S / F(255)
    out = C0.copy()
    out[done] = new[done].astype(F)
    return out, views, _stats(n, done.sum(), frames, views), codes


def _pair_loop(P, N, frame, w, h, K, p):
    """one pair on binary32 scalars: (code, wgt, val)"""
    D, C, W, o = frame[0], frame[1], np.asarray(frame[2], F).reshape(4, 4), np.asarray(frame[3], F).reshape(3)
    fx, fy, cx, cy = F(K[0][0]), F(K[1][1]), F(K[0][2]), F(K[1][2])

    def dot(r):
        return ((r[0] * P[0] + r[1] * P[1]) + r[2] * P[2]) + r[3] * F(1)

    p0, p1, z = dot(W[0]), dot(W[1]), dot(W[2])
    if not (z >= F(p["depthMin"]) and z <= F(p["depthMax"])):
        return RANGE, None, None
    u = (p0 * fx) / z + cx
    v = (p1 * fy) / z + cy
    if not (u >= 0 and u < F(w - 1) and v >= 0 and v < F(h - 1)):
        return IMAGE, None, None
    x0, y0 = int(u), int(v)
    a, b = u - F(x0), v - F(y0)
    c = (o[0] - P[0], o[1] - P[1], o[2] - P[2])
    l = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    if not (np.isfinite(l) and l > 0):
        return FACING, None, None
    cosv = SIGN * (((N[0] * c[0] + N[1] * c[1]) + N[2] * c[2]) / l)
    if not cosv >= F(p["minCos"]):
        return FACING, None, None
    tol = F(p["depthTolerance"]) + F(p["depthToleranceLin"]) * z
    texels = [(x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)]
    for tx, ty in texels:
        d = F(D[ty, tx])
        if not (np.isfinite(d) and d > 0 and np.abs(d - z) <= tol):
            return OCCLUDED, None, None
    cols = [C[ty, tx] for tx, ty in texels]
    for t in cols:
        if t[0] == 0 and t[1] == 0 and t[2] == 0:
            return COLOUR, None, None
    wgt = (cosv * cosv) / (z * z)
    val = []
    for ch in range(3):
        c00, c10, c01, c11 = [F(t[ch]) for t in cols]
        top = c00 + a * (c10 - c00)
        bot = c01 + a * (c11 - c01)
        val.append(top + b * (bot - top))
    return VIEW, wgt, val


def recolour_loop(pos, nrm, col, frames, w, h, K, p):
    P = np.ascontiguousarray(pos, F).reshape(-1, 3); N = np.ascontiguousarray(nrm, F).reshape(-1, 3); C0 = np.ascontiguousarray(col, F).reshape(-1, 3)
    n, mode = len(P), int(p["mode"])
    codes = np.full((n, len(frames)), SKIPPED, np.uint8)
    out = C0.copy(); views = np.zeros(n, np.uint32)
    recoloured = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            Pi, Ni = P[i], N[i]
            ok = bool(np.isfinite(Pi).all() and np.isfinite(Ni).all() and (Ni[0] * Ni[0] + Ni[1] * Ni[1]) + Ni[2] * Ni[2] > 0)
            S = [F(0), F(0), F(0)]; SW = F(0); nviews = 0
            for k, frame in enumerate(frames):
                if frame[4]:
                    continue
                code, wgt, val = _pair_loop(Pi, Ni, frame, w, h, K, p) if ok else (NORMAL, None, None)
                codes[i, k] = code
                if code != VIEW:
                    continue
                if mode == 0:
                    S = [S[c] + wgt * val[c] for c in range(3)]
                    SW = SW + wgt
                elif nviews == 0 or wgt > SW:
                    S, SW = list(val), wgt
                nviews += 1
            views[i] = nviews
            if nviews == 0 or (mode == 0 and not (np.isfinite(SW) and SW > 0)):
                continue
            recoloured += 1
            out[i] = [(S[c] / SW) / F(255) if mode == 0 else S[c] / F(255) for c in range(3)]
    return out, views, _stats(n, recoloured, frames, views), codes


def mul44(a, b):
    """bf_device.h's product in binary32: r[i][j] = ((a[i][0] b[0][j] + a[i][1] b[1][j]) + a[i][2] b[2][j]) + a[i][3] b[3][j]"""
    a = np.asarray(a, F).reshape(4, 4); b = np.asarray(b, F).reshape(4, 4)
    with np.errstate(all="ignore"):
        return ((a[:, 0:1] * b[0:1, :] + a[:, 1:2] * b[1:2, :]) + a[:, 2:3] * b[2:3, :]) + a[:, 3:4] * b[3:4, :]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    """None where (colours, views, stats[, codes]) agree as bits, otherwise what differs"""
    if got[0].shape != want[0].shape or not np.array_equal(bits(got[0]), bits(want[0])):
        bad = np.argwhere(bits(got[0]) != bits(want[0])) if got[0].shape == want[0].shape else []
        return "colours differ at %s" % (bad[:4].tolist(),)
    if not np.array_equal(got[1], want[1]):
        return "views differ: %s vs %s" % (got[1][:8], want[1][:8])
    if got[2] != want[2]:
        return "stats differ: %s vs %s" % (got[2], want[2])
    if len(got) > 3 and len(want) > 3 and not np.array_equal(got[3], want[3]):
        return "codes differ at %s" % (np.argwhere(got[3] != want[3])[:4].tolist(),)
    return None


def ply_bytes(pos, nrm, col, faces):
    return mesh_simplify_ref.ply_bytes(pos, nrm, col, faces)
