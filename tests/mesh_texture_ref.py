"""The definition of the mesh texture (DESIGN.md "Mesh texture: the definition"; include/bf_hip.h) restated in numpy, vectorised over the faces (the choice) and
over the texels (the fill).  `texture` returns a dict: atlas [H,A,4] uint8, faceFrame [nf] int32, faceUV [nf,6] float32, stats, and for the tests that prove what a
planted case is named for: codes [nf,3,K] uint8 (the recolouring's rule code of every (face corner, frame) pair; SKIPPED for a skipped frame, NORMAL for a degenerate
face), weights [nf,3,K] float32 (a view's weight), why [H,A] uint8 (where each texel came from, the WHY_* below).  Arithmetic is binary32, one rounding per
operation: every intermediate below is a float32 array.  The pair rules are tests/mesh_recolour_ref.py's, the face's normal in place of the vertex's.

A frame is (depth [h,w] float32, colour [h,w,4] uint8, meshToCamera [4,4] float32, cameraCentre [3] float32, skipped); params is a dict with the fields of
bf_mesh_texture_params."""
import numpy as np

from tests import mesh_recolour_ref as R

F = np.float32
STAT_KEYS = ("numFaces", "numFacesTextured", "numFacesUntextured", "numFramesUsed", "numFramesSkipped", "atlasWidth", "atlasHeight", "numTexelsFromFrames",
             "numTexelsFromVertices", "numTexelsUnused")
# where a texel came from: unused; the frame; then the fallbacks - the face has no frame, z not finite or <= 0, outside the image, a black colour texel, a face
# with an index out of range
WHY_UNUSED, WHY_FRAME, WHY_NO_FRAME, WHY_Z, WHY_IMAGE, WHY_BLACK, WHY_INDEX = range(7)
MAX_HEIGHT = 32768


def params(depthMin=0.25, depthMax=8.0, depthTolerance=0.0625, depthToleranceLin=0.0, minCos=0.25, patchSize=8, atlasWidth=64):
    return dict(depthMin=depthMin, depthMax=depthMax, depthTolerance=depthTolerance, depthToleranceLin=depthToleranceLin, minCos=minCos, patchSize=patchSize, atlasWidth=atlasWidth)


def layout(nf, S, A):
    """(m, cellsPerRow, H)"""
    assert 4 <= S <= 64 and S <= A <= 16384
    cpr = A // S
    cells = (nf + 1) // 2
    return S - 3, cpr, S * (-(-cells // cpr))


def owner(S):
    """[S,S] indexed [j, i]: the half that owns texel (i, j) of a cell"""
    j, i = np.mgrid[0:S, 0:S]
    return (i + j > S - 1).astype(np.int64)


def corners(S):
    """[2,3,2]: per half the texels (ci, cj) of a, b, c"""
    m = S - 3
    half0 = np.array([(0, 0), (m, 0), (0, m)], np.int64)
    return np.stack([half0, S - 1 - half0])


def face_uv(nf, S, A):
    m, cpr, H = layout(nf, S, A)
    f = np.arange(nf, dtype=np.int64)
    q, t = f >> 1, f & 1
    X, Y = (q % cpr) * S, (q // cpr) * S
    c = corners(S)[t]                                                    # [nf,3,2]
    out = np.zeros((nf, 6), F)
    with np.errstate(all="ignore"):
        out[:, 0::2] = ((X[:, None] + c[:, :, 0]).astype(F) + F(0.5)) / F(A)
        out[:, 1::2] = F(1.0) - ((Y[:, None] + c[:, :, 1]).astype(F) + F(0.5)) / F(H)
    return out


def _gather(arr, idx, nv):
    """rows of arr at idx, zeros where idx is out of range"""
    padded = np.vstack([np.ascontiguousarray(arr, F).reshape(-1, 3), np.zeros((1, 3), F)])
    return padded[np.where(idx < nv, idx, nv)]


def select(pos, faces, frames, w, h, K, p):
    """(faceFrame, codes, weights)"""
    P = np.ascontiguousarray(pos, F).reshape(-1, 3)
    Fc = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3).astype(np.int64)
    nv, nf, nk = len(P), len(Fc), len(frames)
    codes = np.full((nf, 3, nk), R.SKIPPED, np.uint8)
    weights = np.full((nf, 3, nk), np.nan, F)
    best = np.full(nf, -1, np.int32)
    if nf == 0:
        return best, codes, weights
    with np.errstate(all="ignore"):
        bad = (Fc >= nv).any(1)
        Pc = [_gather(P, Fc[:, e], nv) for e in range(3)]
        e1, e2 = Pc[1] - Pc[0], Pc[2] - Pc[0]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = ~bad & np.isfinite(Pc[0]).all(1) & np.isfinite(Pc[1]).all(1) & np.isfinite(Pc[2]).all(1) & np.isfinite(length) & (length > 0)
        N = n / length[:, None]
        best_w = np.zeros(nf, F)
        for k, frame in enumerate(frames):
            if frame[4]:
                continue
            viewed = np.ones(nf, bool)
            for e in range(3):
                code, wgt, _ = R._frame_pairs(Pc[e], N, ok, frame, w, h, K, p)
                codes[:, e, k] = code
                weights[:, e, k] = np.where(code == R.VIEW, wgt, F(np.nan))
                viewed &= code == R.VIEW
            wgt = np.fmin(np.fmin(weights[:, 0, k], weights[:, 1, k]), weights[:, 2, k])
            take = viewed & ((best < 0) | (wgt > best_w))
            best = np.where(take, np.int32(k), best)
            best_w = np.where(take, wgt, best_w)
    return best, codes, weights


def _bytes(val):
    with np.errstate(all="ignore"):
        return (np.fmin(np.fmax(val, F(0.0)), F(255.0)) + F(0.5)).astype(np.int32).astype(np.uint8)


def fill(pos, col, faces, face_frame, frames, w, h, K, S, A):
    """(atlas [H,A,4] uint8, why [H,A] uint8)"""
    P = np.ascontiguousarray(pos, F).reshape(-1, 3); C0 = np.ascontiguousarray(col, F).reshape(-1, 3)
    Fc = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3).astype(np.int64)
    nv, nf = len(P), len(Fc)
    m, cpr, H = layout(nf, S, A)
    atlas = np.zeros((H, A, 4), np.uint8); why = np.full((H, A), WHY_UNUSED, np.uint8)
    if H == 0:
        return atlas, why
    ys, xs = np.mgrid[0:H, 0:A]
    i, j = xs % S, ys % S
    t = (i + j > S - 1).astype(np.int64)
    f = 2 * ((ys // S) * cpr + xs // S) + t
    used = (xs < cpr * S) & (f < nf)
    ys, xs, i, j, t, f = ys[used], xs[used], i[used], j[used], t[used], f[used]
    n = len(f)
    fx, fy, cx, cy = F(K[0][0]), F(K[1][1]), F(K[0][2]), F(K[1][2])
    with np.errstate(all="ignore"):
        idx = Fc[f]
        bad = (idx >= nv).any(1)
        s = np.where(t == 1, S - 1 - i, i).astype(F) / F(m)
        r = np.where(t == 1, S - 1 - j, j).astype(F) / F(m)
        wb, wc, wa = s, r, (F(1.0) - s) - r
        Pa, Pb, Pc = (_gather(P, idx[:, e], nv) for e in range(3))
        Ca, Cb, Cc = (_gather(C0, idx[:, e], nv) for e in range(3))
        Pt = (wa[:, None] * Pa + wb[:, None] * Pb) + wc[:, None] * Pc
        val = ((wa[:, None] * Ca + wb[:, None] * Cb) + wc[:, None] * Cc) * F(255.0)
        reason = np.full(n, WHY_NO_FRAME, np.uint8)
        k = np.ascontiguousarray(face_frame, np.int32)[f]
        for kk in np.unique(k[(k >= 0) & ~bad]):
            D, C, W, o = frames[kk][:4]
            W = np.asarray(W, F).reshape(4, 4); C = np.ascontiguousarray(C, np.uint8)
            sel = np.flatnonzero((k == kk) & ~bad)
            px, py, pz = Pt[sel, 0], Pt[sel, 1], Pt[sel, 2]

            def dot(row):
                return ((row[0] * px + row[1] * py) + row[2] * pz) + row[3] * F(1)

            p0, p1, z = dot(W[0]), dot(W[1]), dot(W[2])
            why_k = np.full(len(sel), WHY_FRAME, np.uint8)
            alive = np.isfinite(z) & (z > 0)
            why_k[~alive] = WHY_Z
            u = (p0 * fx) / z + cx
            v = (p1 * fy) / z + cy
            inside = (u >= 0) & (u < F(w - 1)) & (v >= 0) & (v < F(h - 1))
            why_k[alive & ~inside] = WHY_IMAGE
            alive &= inside
            x0 = np.where(alive, u, 0).astype(np.int32); y0 = np.where(alive, v, 0).astype(np.int32)
            a = u - x0.astype(F); b = v - y0.astype(F)
            tex = [C[y0, x0, :3], C[y0, x0 + 1, :3], C[y0 + 1, x0, :3], C[y0 + 1, x0 + 1, :3]]
            black = np.zeros(len(sel), bool)
            for c in tex:
                black |= (c == 0).all(1)
            why_k[alive & black] = WHY_BLACK
            alive &= ~black
            c00, c10, c01, c11 = [c.astype(F) for c in tex]
            top = c00 + a[:, None] * (c10 - c00)
            bot = c01 + a[:, None] * (c11 - c01)
            sample = top + b[:, None] * (bot - top)
            val[sel[alive]] = sample[alive]
            reason[sel] = why_k
        reason[bad] = WHY_INDEX
        rgb = _bytes(val)
        rgb[bad] = 0
    atlas[ys, xs, :3] = rgb
    atlas[ys, xs, 3] = 255
    why[ys, xs] = reason
    return atlas, why


def texture(pos, col, faces, frames, w, h, K, p):
    S, A = int(p["patchSize"]), int(p["atlasWidth"])
    nf = len(np.asarray(faces).reshape(-1, 3))
    face_frame, codes, weights = select(pos, faces, frames, w, h, K, p)
    atlas, why = fill(pos, col, faces, face_frame, frames, w, h, K, S, A)
    used = sum(1 for f in frames if not f[4])
    textured = int((face_frame >= 0).sum())
    stats = dict(numFaces=nf, numFacesTextured=textured, numFacesUntextured=nf - textured, numFramesUsed=used, numFramesSkipped=len(frames) - used, atlasWidth=A,
                 atlasHeight=atlas.shape[0], numTexelsFromFrames=int((why == WHY_FRAME).sum()), numTexelsFromVertices=int((why >= WHY_NO_FRAME).sum()),
                 numTexelsUnused=int((why == WHY_UNUSED).sum()))
    return dict(atlas=atlas, faceFrame=face_frame, faceUV=face_uv(nf, S, A), stats=stats, codes=codes, weights=weights, why=why)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    """None where (atlas, faceFrame, faceUV, stats) agree - bytes, integers, bits - with the restatement's dict, otherwise what differs"""
    atlas, ff, uv, st = got
    if not np.array_equal(ff, want["faceFrame"]):
        return "face frames differ at %s: %s vs %s" % (np.flatnonzero(ff != want["faceFrame"])[:4].tolist() if ff.shape == want["faceFrame"].shape else "?", ff[:8], want["faceFrame"][:8])
    if uv.shape != want["faceUV"].shape or not np.array_equal(bits(uv), bits(want["faceUV"])):
        return "texture coordinates differ"
    if atlas.shape != want["atlas"].shape:
        return "atlas shapes differ: %s vs %s" % (atlas.shape, want["atlas"].shape)
    if not np.array_equal(atlas, want["atlas"]):
        bad = np.argwhere((atlas != want["atlas"]).any(2))
        y, x = bad[0]
        return "%d texels differ, the first at (x %d, y %d): %s vs %s (why %d)" % (len(bad), x, y, atlas[y, x], want["atlas"][y, x], want["why"][y, x])
    if st != want["stats"]:
        return "stats differ: %s vs %s" % (st, want["stats"])
    return None


def ply_bytes(texture_name, pos, nrm, col, faces, uv):
    """the file bf_write_ply_textured writes"""
    plain = R.ply_bytes(pos, nrm, col, faces)
    head, body = plain.split(b"end_header\n", 1)
    line = b"comment bundlefusion_amd marching cubes\n"
    assert head.count(line) == 1 and head.endswith(b"property list uchar int vertex_indices\n")
    head = head.replace(line, line + b"comment TextureFile " + str(texture_name).encode() + b"\n") + b"property list uchar float texcoord\nend_header\n"
    nf = len(np.asarray(faces).reshape(-1, 3))
    vertex_bytes = len(body) - 13 * nf
    f = np.zeros(nf, np.dtype([("n", "u1"), ("i", "<i4", 3), ("k", "u1"), ("uv", "<f4", 6)]))
    assert f.dtype.itemsize == 38
    f["n"] = 3; f["i"] = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3).view(np.int32); f["k"] = 6; f["uv"] = np.ascontiguousarray(uv, F).reshape(-1, 6)
    return head + body[:vertex_bytes] + f.tobytes()
