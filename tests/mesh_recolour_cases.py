"""Planted meshes and frames for the mesh recolouring tests (tests/test_mesh_recolour_cpu.py, tests/test_mesh_recolour_gpu.py).  Every case is a dict
    name, family, pos, nrm, col ([nv,3] float32), frames [(depth (h, w) f32, colour (h, w, 4) u8, meshToCamera (4, 4) f32, cameraCentre (3,) f32, skipped)],
    w, h, K (4, 4) f32, params (tests/mesh_recolour_ref.params), codes: the rule codes the case's family is named for (the CPU test proves each occurs)
and, where the family is about one value, `expect`: what the CPU test asserts of the restatement's result.

Intrinsics, poses and depths are powers of two and small integers: a projection that should land on a pixel centre or on the image border lands exactly there,
`|d - z|` that should equal the tolerance does, and a cosine that should equal minCos does.  The plain camera sits at the origin and looks along +z; a vertex
that faces it has the normal (0, 0, -1) (the normals point to the side of the camera: BF_RECOLOUR_NORMAL_SIGN = +1)."""
import numpy as np

from bundlefusion_amd import capi
from tests import mesh_recolour_ref as R

F = np.float32
NINF, PINF, NAN = F(-np.inf), F(np.inf), F(np.nan)
I4 = np.eye(4, dtype=F)
ROT_Z90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)
TOWARDS = (0.0, 0.0, -1.0)


def below(x):
    return np.nextafter(F(x), F(-np.inf))


def above(x):
    return np.nextafter(F(x), F(np.inf))


def intr(fx, cx, cy, fy=None):
    K = np.eye(4, dtype=F)
    K[0, 0] = fx; K[1, 1] = fx if fy is None else fy; K[0, 2] = cx; K[1, 2] = cy
    return K


def pose(tx=0.0, ty=0.0, tz=0.0, rot=None):
    T = np.eye(4, dtype=F)
    if rot is not None:
        T[:3, :3] = rot
    T[:3, 3] = [tx, ty, tz]
    return T


def colours(h, w, rng):
    return rng.integers(1, 256, (h, w, 4)).astype(np.uint8)          # never black


def flat(h, w, d=1.0):
    return np.full((h, w), d, F)


def frame(D, C, M=I4):
    """a frame from its camera-to-mesh pose, through the library's own bf_mesh_recolour_frame_from_pose"""
    W, o, skipped = capi.mesh_recolour_frame_from_pose(M)
    return (np.ascontiguousarray(D, F), np.ascontiguousarray(C, np.uint8), W, o, skipped)


def _mesh(points, normals=None, seed=0):
    pos = np.asarray(points, F).reshape(-1, 3)
    nrm = np.tile(np.asarray(TOWARDS, F), (len(pos), 1)) if normals is None else np.asarray(normals, F).reshape(-1, 3)
    col = np.random.default_rng(1000 + seed).uniform(0, 1, (len(pos), 3)).astype(F)
    return pos, nrm, col


def _case(name, family, mesh, frames, w, h, K, p, codes, expect=None):
    pos, nrm, col = mesh
    return dict(name=name, family=family, pos=pos, nrm=nrm, col=col, frames=frames, w=w, h=h, K=K, params=p, codes=tuple(codes), expect=expect)


def image_cases():
    """u and v exactly 0 (kept), exactly w-1 / h-1 (rejected), the float just below (kept) and just below 0 (rejected): u = 4 X, v = 4 Y at z = 1"""
    rng = np.random.default_rng(21)
    w, h = 8, 6
    pts = [(0, 0, 1), (7 / 4, 0, 1), (below(7) / F(4), 0, 1), (-2.0 ** -30, 0, 1), (0, 5 / 4, 1), (0, below(5) / F(4), 1), (0, -2.0 ** -30, 1), (1.0, 0.5, 1)]
    views = [1, 0, 1, 0, 0, 1, 0, 1]
    return [_case("image_border", "image", _mesh(pts, seed=1), [frame(flat(h, w), colours(h, w, rng))], w, h, intr(4, 0, 0), R.params(minCos=0.25), (R.IMAGE, R.VIEW),
                  dict(views=views))]


def range_cases():
    """z equal to depthMin and to depthMax (kept), one float outside each (rejected), behind the camera; the tolerance is wide open"""
    rng = np.random.default_rng(22)
    w, h = 8, 6
    pts = [(0, 0, 0.25), (0, 0, below(0.25)), (0, 0, 8), (0, 0, above(8)), (0, 0, -1), (0, 0, 1)]
    return [_case("range_border", "range", _mesh(pts, seed=2), [frame(flat(h, w), colours(h, w, rng))], w, h, intr(4, 3, 2), R.params(depthTolerance=16.0), (R.RANGE, R.VIEW),
                  dict(views=[1, 0, 1, 0, 0, 1]))]


def occlusion_cases():
    """tol = 2^-4 + 2^-4 * 2 = 0.1875 at z = 2; the vertex projects onto pixel (3, 2) of a 10 x 8 frame, its texels are (3,2) (4,2) (3,3) (4,3)"""
    rng = np.random.default_rng(23)
    w, h = 10, 8
    K = intr(4, 3, 2)
    p = R.params(depthTolerance=2.0 ** -4, depthToleranceLin=2.0 ** -4)
    texels = [(3, 2), (4, 2), (3, 3), (4, 3)]
    out = []
    edge, kept = [], []
    for k, (d, keep) in enumerate([(F(2.1875), 1), (above(2.1875), 0), (F(1.8125), 1), (below(1.8125), 0)]):
        for x, y in texels:
            D = flat(h, w, 2.0); D[y, x] = d
            edge.append(frame(D, colours(h, w, rng))); kept.append(keep)
    out.append(_case("occlusion_tolerance", "occlusion", _mesh([(0, 0, 2)], seed=3), edge, w, h, K, p, (R.OCCLUDED, R.VIEW), dict(frame_views=kept)))
    special, kept = [], []
    for v in (NINF, PINF, NAN, F(0), F(-2)):
        for x, y in texels:
            D = flat(h, w, 2.0); D[y, x] = v
            special.append(frame(D, colours(h, w, rng))); kept.append(0)
    special.append(frame(flat(h, w, 2.0), colours(h, w, rng))); kept.append(1)
    out.append(_case("occlusion_specials", "occlusion", _mesh([(0, 0, 2)], seed=4), special, w, h, K, p, (R.OCCLUDED, R.VIEW), dict(frame_views=kept)))
    return out


def black_cases():
    rng = np.random.default_rng(24)
    w, h = 8, 6
    frames, kept = [], []
    for x, y in [(3, 2), (4, 2), (3, 3), (4, 3)]:
        C = colours(h, w, rng); C[y, x] = (0, 0, 0, 255)          # the fourth byte is not colour
        frames.append(frame(flat(h, w), C)); kept.append(0)
        C = colours(h, w, rng); C[y, x] = (0, 0, 1, 0)            # not black
        frames.append(frame(flat(h, w), C)); kept.append(1)
    return [_case("black_texels", "black", _mesh([(0, 0, 1)], seed=5), frames, w, h, intr(4, 3, 2), R.params(), (R.COLOUR, R.VIEW), dict(frame_views=kept))]


def facing_cases():
    """P = (0.75, 0, 1) seen from the origin: c = (-0.75, 0, -1), l = 1.25, and with N = (0, 0, -0.625) the cosine is 0.625 / 1.25 = 0.5 exactly"""
    rng = np.random.default_rng(25)
    w, h = 12, 8
    K = intr(4, 3, 2)
    out = []
    for name, min_cos, views in (("facing_equal", F(0.5), 1), ("facing_one_float_below", above(0.5), 0)):
        out.append(_case(name, "facing", _mesh([(0.75, 0, 1)], [(0, 0, -0.625)], seed=6), [frame(flat(h, w), colours(h, w, rng))], w, h, K, R.params(minCos=min_cos),
                         (R.VIEW,) if views else (R.FACING,), dict(views=[views])))
    # a zero normal, a NaN normal, an infinite position; a back-facing normal; a vertex at the camera centre (z = 0: the range gate has it first); behind the camera
    pts = [(0, 0, 1), (0, 0, 1), (PINF, 0, 1), (0, 0, 1), (0, 0, 0), (0, 0, -1), (0, 0, 1)]
    nrm = [(0, 0, 0), (NAN, 0, -1), TOWARDS, (0, 0, 1), TOWARDS, TOWARDS, TOWARDS]
    out.append(_case("facing_degenerate", "facing", _mesh(pts, nrm, seed=7), [frame(flat(h, w), colours(h, w, rng))], w, h, K, R.params(), (R.NORMAL, R.FACING, R.RANGE, R.VIEW),
                     dict(views=[0, 0, 0, 0, 0, 0, 1], first_codes=[R.NORMAL, R.NORMAL, R.NORMAL, R.FACING, R.RANGE, R.RANGE, R.VIEW])))
    # the camera centre given as the vertex itself while mesh-to-camera still puts the vertex in range (a table no pose produces): l = 0
    f = frame(flat(h, w), colours(h, w, rng))
    f = (f[0], f[1], f[2], np.array([0, 0, 1], F), False)
    out.append(_case("facing_zero_length", "facing", _mesh([(0, 0, 1)], seed=8), [f], w, h, K, R.params(), (R.FACING,), dict(views=[0])))
    return out


def pose_cases():
    """M[0] = -inf and NaN (the reference's invalid pose), a singular pose: skipped, no error; a valid rotated and translated pose between them"""
    rng = np.random.default_rng(26)
    w, h = 8, 6
    bad = []
    for v in (NINF, NAN):
        M = pose(); M[0, 0] = v
        bad.append(M)
    M = np.full((4, 4), NINF, F); bad.append(M)
    M = pose(); M[2, :] = M[1, :]; bad.append(M)                       # singular: two equal rows
    bad.append(np.zeros((4, 4), F))
    good = pose(tx=1.0, ty=2.0, tz=-1.0, rot=ROT_Z90)                  # camera at (1, 2, -1), its x axis along the mesh's y
    frames = [frame(flat(h, w, 2.0), colours(h, w, rng), M) for M in bad[:2]] + [frame(flat(h, w, 2.0), colours(h, w, rng), good)] + \
             [frame(flat(h, w, 2.0), colours(h, w, rng), M) for M in bad[2:]]
    # camera coordinates (0.5, 0.25, 2) -> mesh: R (x, y, z) + t = (-0.25 + 1, 0.5 + 2, 2 - 1)
    return [_case("poses", "poses", _mesh([(0.75, 2.5, 1.0), (1.0, 2.0, 1.0)], seed=9), frames, w, h, intr(4, 3, 2), R.params(), (R.VIEW,),
                  dict(views=[1, 1], skipped=[1, 1, 0, 1, 1, 1]))]


def order_cases():
    """the same vertices seen from 0.25 m, 8 m, 1 m and 3 m along the axis: weights of 16, 1/64, 1 and 1/9 per unit cosine - the sum depends on the order"""
    rng = np.random.default_rng(27)
    w, h = 24, 18
    pts = [(0.013 * i, 0.007 * i - 0.02, 0.003 * i) for i in range(9)]
    frames = [frame(flat(h, w, z), colours(h, w, rng), pose(tz=-z)) for z in (0.25, 8.0, 1.0, 3.0)]
    out = [_case("order_weights", "order", _mesh(pts, seed=10), frames, w, h, intr(16, 12, 9), R.params(depthMax=16.0, depthTolerance=1.0, minCos=0.125), (R.VIEW,), dict(permute=True))]
    # best view: frames 0 and 1 are the same camera with other colours (equal weights: the earlier stays), frame 2 is farther, frame 3 is nearer (it wins)
    tie = [frame(flat(h, w, 1.0), colours(h, w, rng), pose(tz=-1.0)), frame(flat(h, w, 1.0), colours(h, w, rng), pose(tz=-1.0)), frame(flat(h, w, 2.0), colours(h, w, rng), pose(tz=-2.0))]
    out.append(_case("order_tie", "order", _mesh(pts, seed=11), tie, w, h, intr(16, 12, 9), R.params(depthMax=16.0, depthTolerance=1.0, minCos=0.125), (R.VIEW,), dict(best=0)))
    out.append(_case("order_nearer_wins", "order", _mesh(pts, seed=12), tie + [frame(flat(h, w, 0.5), colours(h, w, rng), pose(tz=-0.5))], w, h, intr(16, 12, 9),
                     R.params(depthMax=16.0, depthTolerance=1.0, minCos=0.125), (R.VIEW,), dict(best=3)))
    return out


def unseen_cases():
    """vertices no frame sees keep their colour bit for bit: NaN, -0, a denormal and an infinity among the colours"""
    rng = np.random.default_rng(28)
    w, h = 8, 6
    pts = [(100, 0, 1), (0, 0, 100), (0, 0, 1), (0, 100, 1), (0, 0, -5)]
    pos, nrm, col = _mesh(pts, seed=13)
    col[0] = (NAN, F(-0.0), F(1e-42)); col[1] = (PINF, F(2.5), F(-1)); col[3] = np.array([0x7FC12345, 0xFFC00001, 0x00000001], np.uint32).view(F)
    return [_case("unseen", "unseen", (pos, nrm, col), [frame(flat(h, w), colours(h, w, rng)) for _ in range(3)], w, h, intr(4, 3, 2), R.params(), (R.VIEW, R.IMAGE, R.RANGE),
                  dict(views=[0, 0, 3, 0, 0]))]


def empty_cases():
    rng = np.random.default_rng(29)
    w, h = 8, 6
    e = np.zeros((0, 3), F)
    return [_case("no_frames", "empty", _mesh([(0, 0, 1), (1, 0, 1)], seed=14), [], w, h, intr(4, 3, 2), R.params(), (), dict(views=[0, 0])),
            _case("no_vertices", "empty", (e, e, e), [frame(flat(h, w), colours(h, w, rng))], w, h, intr(4, 3, 2), R.params(), (), dict(views=[]))]


def meaning_case():
    """one vertex, one frame: the camera at (2, 1, 0) looks along +z, the vertex (2, 1, 2) lies on its axis at z = 2 and projects exactly onto pixel (cx, cy) = (5, 1);
    cosv = 1 and the weight 1/4 is a power of two, so both modes give the pixel's bytes over 255 exactly.  The test states the expected value by hand."""
    rng = np.random.default_rng(30)
    w, h = 8, 6
    C = colours(h, w, rng); C[1, 5] = (200, 100, 50, 7)
    return _case("meaning", "meaning", _mesh([(2, 1, 2)], seed=15), [frame(flat(h, w, 2.0), C, pose(tx=2.0, ty=1.0))], w, h, intr(4, 5, 1), R.params(), (R.VIEW,), dict(views=[1]))


FAMILIES = {"image": image_cases, "range": range_cases, "occlusion": occlusion_cases, "black": black_cases, "facing": facing_cases, "poses": pose_cases, "order": order_cases,
            "unseen": unseen_cases, "empty": empty_cases, "meaning": lambda: [meaning_case()]}


def all_cases():
    return [c for f in FAMILIES.values() for c in f()]


# --------------------------------------------------------------------------- the random case
RANDOM_SEED = 5
RANDOM_W, RANDOM_H = 64, 48


def _rot_y(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def _rot_x(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def random_case(seed=RANDOM_SEED, n=5000, num_frames=7):
    """a noisy unit sphere of n vertices with outward normals and num_frames cameras 8 m from its centre looking at it (64 x 48, the sphere slightly taller than
    the image); depths rendered from the exact sphere, then invalid depths and black pixels sprinkled in, a few broken vertices"""
    rng = np.random.default_rng(seed)
    w, h = RANDOM_W, RANDOM_H
    K = intr(192.0, 31.5, 23.5)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = (d * (1.0 + rng.uniform(-0.01, 0.01, (n, 1)))).astype(F)
    nrm = d.astype(F)
    col = rng.uniform(0, 1, (n, 3)).astype(F)
    nrm[rng.choice(n, 12, replace=False)] = 0
    pos[rng.choice(n, 4, replace=False), 0] = NAN
    ys, xs = np.mgrid[0:h, 0:w]
    dirs = np.stack([(xs - 31.5) / 192.0, (ys - 23.5) / 192.0, np.ones((h, w))], -1)
    frames = []
    for k in range(num_frames):
        Rm = _rot_y(2 * np.pi * k / num_frames + 0.1) @ _rot_x(0.15 * np.sin(1.7 * k))
        t = Rm @ np.array([0, 0, -8.0])
        M = np.eye(4); M[:3, :3] = Rm; M[:3, 3] = t
        # ray o + s * dir (camera coordinates; the centre is at (0, 0, 8)): |s dir - c|^2 = 1
        cc = np.array([0, 0, 8.0])
        a = (dirs * dirs).sum(-1); b = -2 * (dirs @ cc); c0 = cc @ cc - 1.0
        disc = b * b - 4 * a * c0
        s = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)
        D = s.astype(F)                                    # dir.z = 1: the depth is s; 0 beside the sphere
        C = colours(h, w, rng)
        bad = rng.uniform(size=(h, w))
        D[bad < 0.004] = NAN; D[(bad >= 0.004) & (bad < 0.008)] = 0; D[(bad >= 0.008) & (bad < 0.010)] = PINF; D[(bad >= 0.010) & (bad < 0.012)] = -1
        C[rng.uniform(size=(h, w)) < 0.012, :3] = 0
        frames.append(frame(D, C, M.astype(F)))
    p = R.params(depthMin=0.5, depthMax=8.05, depthTolerance=0.05, depthToleranceLin=0.01, minCos=0.1)
    return _case("random_sphere", "random", (pos, nrm, col), frames, w, h, K, p, range(7))
