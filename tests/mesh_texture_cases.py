"""Planted meshes and frames for the mesh texture tests (tests/test_mesh_texture_cpu.py, tests/test_mesh_texture_gpu.py), built with the helpers of
tests/mesh_recolour_cases.py.  Every case is a dict
    name, family, pos, col ([nv,3] float32), faces ([nf,3] uint32), frames [(depth, colour, meshToCamera, cameraCentre, skipped)], w, h, K, params
    (tests/mesh_texture_ref.params), expect: what the CPU test asserts of the restatement's result, so that the case tests what it is named for.

Intrinsics, poses and depths are powers of two and small integers (as in the recolouring's cases): with K = intr(4, 3, 2) a point (X, Y, 1) seen from the origin
lands on pixel (4 X + 3, 4 Y + 2) exactly.  A face that the plain camera views is wound so that e1 x e2 points at the camera (-z)."""
import numpy as np

from tests import mesh_recolour_cases as RC
from tests import mesh_recolour_ref as R
from tests import mesh_texture_ref as T

F = np.float32
NAN = F(np.nan)
K43 = RC.intr(4, 3, 2)
# the plain face: pixels (3, 2), (3, 3), (4, 2) of a frame seen from the origin
PLAIN = [(0, 0, 1), (0, 0.25, 1), (0.25, 0, 1)]
ROTATIONS = [(0, 1, 2), (1, 2, 0), (2, 0, 1)]


def _case(name, family, points, faces, frames, w, h, p, expect=None, col=None, K=K43, seed=0):
    pos = np.asarray(points, F).reshape(-1, 3)
    if col is None:
        col = np.random.default_rng(2000 + seed).uniform(0, 1, (len(pos), 3)).astype(F)
    return dict(name=name, family=family, pos=pos, col=np.asarray(col, F).reshape(-1, 3), faces=np.asarray(faces, np.uint32).reshape(-1, 3), frames=frames, w=w, h=h, K=K, params=p,
                expect=expect or {})


def _plain_frame(w, h, rng, d=1.0):
    return RC.frame(RC.flat(h, w, d), RC.colours(h, w, rng))


# --------------------------------------------------------------------------- the face choice
def one_corner_cases():
    """vertices 0 1 2 are the plain face, which the frame views (face 3); vertex 3 replaces vertex 2 and fails exactly one rule; faces 0 1 2 are the three rotations
    of (0, 1, 3), so the failing corner is c, b, a in turn"""
    out = []
    faces = [(0, 1, 3), (1, 3, 0), (3, 0, 1), (0, 1, 2)]
    failing = [2, 1, 0]
    rng = np.random.default_rng(41)
    # RANGE: one float beyond depthMax = 1
    w, h = 8, 6
    out.append(_case("corner_range", "corner", PLAIN + [(0.25, 0, RC.above(1.0))], faces, [_plain_frame(w, h, rng)], w, h, T.params(depthMax=1.0), dict(rule=R.RANGE, failing=failing), seed=1))
    # IMAGE: u = 7 = w - 1
    out.append(_case("corner_image", "corner", PLAIN + [(1.0, 0, 1)], faces, [_plain_frame(w, h, rng)], w, h, T.params(), dict(rule=R.IMAGE, failing=failing), seed=2))
    # FACING: the same vertex in a frame wide enough for it; its cosine is 1 / sqrt(2) < 0.75, the others' are 1 and 0.97
    w, h = 10, 8
    out.append(_case("corner_facing", "corner", PLAIN + [(1.0, 0, 1)], faces, [_plain_frame(w, h, rng)], w, h, T.params(minCos=0.75), dict(rule=R.FACING, failing=failing), seed=3))
    # OCCLUDED / COLOUR: vertex 3 = (0.5, 0, 1) lands on pixel (5, 2); texel (6, 3) is in its footprint alone
    w, h = 8, 6
    D = RC.flat(h, w); D[3, 6] = 2.0
    out.append(_case("corner_occluded", "corner", PLAIN + [(0.5, 0, 1)], faces, [RC.frame(D, RC.colours(h, w, rng))], w, h, T.params(), dict(rule=R.OCCLUDED, failing=failing), seed=4))
    C = RC.colours(h, w, rng); C[3, 6] = (0, 0, 0, 9)
    out.append(_case("corner_colour", "corner", PLAIN + [(0.5, 0, 1)], faces, [RC.frame(RC.flat(h, w), C)], w, h, T.params(), dict(rule=R.COLOUR, failing=failing), seed=5))
    return out


def _weights_from(points, w, h, p, centres):
    """the weight of the face (0, 1, 2) seen from every camera centre (tx, tz), looking along +z"""
    C = RC.colours(h, w, np.random.default_rng(0))
    frames = [RC.frame(RC.flat(h, w, 1.0), C, RC.pose(tx=float(tx), tz=float(tz))) for tx, tz in centres]
    _, codes, weights = T.select(np.asarray(points, F), np.array([[0, 1, 2]], np.uint32), frames, w, h, K43, p)
    assert (codes == R.VIEW).all()
    return np.fmin(np.fmin(weights[0, 0], weights[0, 1]), weights[0, 2])


def weight_cases():
    rng = np.random.default_rng(42)
    w, h = 8, 6
    p = T.params(depthTolerance=0.5)
    out = []
    # two frames of one camera: equal weights, the earlier stays; a third, farther away, changes nothing
    tie = [_plain_frame(w, h, rng), _plain_frame(w, h, rng), RC.frame(RC.flat(h, w, 2.0), RC.colours(h, w, rng), RC.pose(tz=-1.0))]
    out.append(_case("weight_tie", "weight", PLAIN, [(0, 1, 2)], tie, w, h, T.params(), dict(face_frame=[0], equal=(0, 1)), seed=6))
    # two cameras whose weights are one float apart: found among camera centres a few 2^-23 m sideways of and behind the origin
    centres = [(i * 2.0 ** -23, -j * 2.0 ** -23) for i in range(8) for j in range(32)]
    b = _weights_from(PLAIN, w, h, p, centres).view(np.uint32).astype(np.int64)
    order = np.argsort(b, kind="stable")
    at = np.flatnonzero(np.diff(b[order]) == 1)[0]
    less, more = centres[order[at]], centres[order[at + 1]]
    fr = lambda c: RC.frame(RC.flat(h, w, 1.0), RC.colours(h, w, rng), RC.pose(tx=float(c[0]), tz=float(c[1])))
    out.append(_case("weight_one_ulp_later_wins", "weight", PLAIN, [(0, 1, 2)], [fr(less), fr(more)], w, h, p, dict(face_frame=[1], ulp=(1, 0)), seed=7))
    out.append(_case("weight_one_ulp_earlier_stays", "weight", PLAIN, [(0, 1, 2)], [fr(more), fr(less)], w, h, p, dict(face_frame=[0], ulp=(0, 1)), seed=8))
    # the least of the three corners decides: seen from the origin the far corner (0.75, 0, 1) has the least weight, 0.64; seen from (0.5, 0, 0) the least is
    # 0.76, so the second frame wins although the corner (0, 0, 1) alone would keep the first (1 against 0.8).  The rotations put the far corner at c, b, a.
    w, h = 10, 8
    pts = [(0, 0, 1), (0, 0.25, 1), (0.75, 0, 1)]
    two = [_plain_frame(w, h, rng), RC.frame(RC.flat(h, w), RC.colours(h, w, rng), RC.pose(tx=0.5))]
    out.append(_case("weight_least_corner", "weight", pts, ROTATIONS, two, w, h, T.params(), dict(face_frame=[1, 1, 1], least_in_frame0=[2, 1, 0]), seed=9))
    # a skipped frame before the winner: the index counts it
    bad = RC.pose(); bad[0, 0] = RC.NINF
    skipped = [RC.frame(RC.flat(6, 8), RC.colours(6, 8, rng), bad), _plain_frame(8, 6, rng)]
    out.append(_case("weight_skipped_before", "weight", PLAIN, [(0, 1, 2)], skipped, 8, 6, T.params(), dict(face_frame=[1], skipped=[1, 0]), seed=10))
    return out


def degenerate_cases():
    """a zero-area face (two equal corners; three on a line), a NaN position, an index == nv and one far beyond; the plain face last"""
    rng = np.random.default_rng(43)
    w, h = 8, 6
    pts = PLAIN + [(0, 0.5, 1), (NAN, 0, 1)]
    faces = [(0, 0, 1), (0, 1, 3), (0, 1, 4), (0, 1, 5), (0xFFFFFFFF, 1, 2), (0, 1, 2)]
    return [_case("degenerate_faces", "degenerate", pts, faces, [_plain_frame(w, h, rng)], w, h, T.params(), dict(face_frame=[-1, -1, -1, -1, -1, 0], why_index=[3, 4]), seed=11)]


# --------------------------------------------------------------------------- the fill
def fill_cases():
    rng = np.random.default_rng(44)
    out = []
    # the corner texels of both halves land on their vertices' pixels: (3,2) (3,3) (4,2) and, the second face, (4,3) (4,2) (3,3)
    w, h = 8, 6
    pts = PLAIN + [(0.25, 0.25, 1)]
    out.append(_case("fill_corners_on_pixels", "fill", pts, [(0, 1, 2), (3, 2, 1)], [_plain_frame(w, h, rng)], w, h, T.params(),
                     dict(face_frame=[0, 0], corner_pixels=[[(3, 2), (3, 3), (4, 2)], [(4, 3), (4, 2), (3, 3)]]), seed=12))
    # corners at pixels (3, 2), (3, 4.5), (6.5, 2): the gutter beyond the long side leaves the 8 x 6 image and falls back
    pts = [(0, 0, 1), (0, 0.625, 1), (0.875, 0, 1)]
    out.append(_case("fill_gutter_leaves_the_image", "fill", pts, [(0, 1, 2)], [_plain_frame(w, h, rng)], w, h, T.params(), dict(face_frame=[0], why=[T.WHY_FRAME, T.WHY_IMAGE]), seed=13))
    # a black pixel inside the face, away from the corners' footprints: corners at (1, 1), (1, 4), (6, 1) of a 10 x 8 frame, pixel (3, 2) black
    w, h = 10, 8
    C = RC.colours(h, w, rng); C[2, 3] = (0, 0, 0, 200)
    pts = [(-0.5, -0.25, 1), (-0.5, 0.5, 1), (0.75, -0.25, 1)]
    out.append(_case("fill_black_texel", "fill", pts, [(0, 1, 2)], [RC.frame(RC.flat(h, w), C)], w, h, T.params(minCos=0.125), dict(face_frame=[0], why=[T.WHY_FRAME, T.WHY_BLACK]), seed=14))
    # a steep face, a and b at z = 2, c at z = 1: with S = 4 (m = 1) the gutter reaches r = 3, wa = -2, where z = -2 * 2 + 3 * 1 = -1
    w, h = 8, 6
    pts = [(0, 0, 2), (0, 0.25, 2), (0.125, 0, 1)]
    out.append(_case("fill_z_not_positive", "fill", pts, [(0, 1, 2)], [_plain_frame(w, h, rng)], w, h, T.params(depthTolerance=4.0, minCos=0.0625, patchSize=4, atlasWidth=16),
                     dict(face_frame=[0], why=[T.WHY_FRAME, T.WHY_Z]), seed=15))
    # the fallback's bytes: colours outside [0, 1], infinite and NaN, no frame at all
    col = [(2.0, -1.0, 0.5), (NAN, 0.25, RC.PINF), (0.0, RC.NINF, 1.0)]
    out.append(_case("fill_fallback_colours", "fill", PLAIN, [(0, 1, 2)], [], w, h, T.params(), dict(face_frame=[-1], why=[T.WHY_NO_FRAME], bytes_seen=[0, 255]), col=col, seed=16))
    return out


def empty_cases():
    rng = np.random.default_rng(45)
    w, h = 8, 6
    bad = RC.pose(); bad[0, 0] = NAN
    none = np.zeros((0, 3), np.uint32)
    return [_case("no_frames", "empty", PLAIN, [(0, 1, 2)], [], w, h, T.params(), dict(face_frame=[-1]), seed=17),
            _case("all_skipped", "empty", PLAIN, [(0, 1, 2)], [RC.frame(RC.flat(h, w), RC.colours(h, w, rng), bad)] * 2, w, h, T.params(), dict(face_frame=[-1], skipped=[1, 1]), seed=18),
            _case("no_faces", "empty", PLAIN, none, [_plain_frame(w, h, rng)], w, h, T.params(), dict(face_frame=[]), seed=19),
            _case("no_vertices", "empty", np.zeros((0, 3), F), none, [_plain_frame(w, h, rng)], w, h, T.params(), dict(face_frame=[]), seed=20)]


FAMILIES = {"corner": one_corner_cases, "weight": weight_cases, "degenerate": degenerate_cases, "fill": fill_cases, "empty": empty_cases}


def all_cases():
    return [c for f in FAMILIES.values() for c in f()]


# --------------------------------------------------------------------------- the sphere
SPHERE_FRAMES = 3


def sphere_case(rings=32, segments=32, seed=5):
    """a unit sphere of rings x segments quads, two faces each (about 2000 for 32 x 32; those at the poles have no area), wound outwards, seen by the three
    64 x 48 cameras of the recolouring's random case with its sprinkled invalid depths and black pixels; a few broken faces"""
    rng = np.random.default_rng(seed)
    base = RC.random_case(seed=seed, n=16, num_frames=SPHERE_FRAMES)
    th = np.linspace(0.0, np.pi, rings + 1); ph = np.linspace(0.0, 2 * np.pi, segments, endpoint=False)
    d = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones_like(ph)), np.outer(np.sin(th), np.sin(ph))], -1).reshape(-1, 3)
    pos = (d * (1.0 + rng.uniform(-0.005, 0.005, (len(d), 1)))).astype(F)
    vid = lambda r, s: r * segments + (s % segments)
    faces = []
    for r in range(rings):
        for s in range(segments):
            a, b, c, e = vid(r, s), vid(r + 1, s), vid(r + 1, s + 1), vid(r, s + 1)
            faces += [(a, b, c), (a, c, e)]
    faces = np.array(faces, np.int64)
    P = pos.astype(np.float64)
    n = np.cross(P[faces[:, 1]] - P[faces[:, 0]], P[faces[:, 2]] - P[faces[:, 0]])
    inward = (n * P[faces].mean(1)).sum(1) < 0
    faces[inward] = faces[inward][:, [0, 2, 1]]
    faces = faces.astype(np.uint32)
    faces[rng.choice(len(faces), 5, replace=False), 1] = len(pos)
    pos[rng.choice(len(pos), 3, replace=False), 2] = NAN
    col = rng.uniform(-0.1, 1.1, (len(pos), 3)).astype(F)
    p = T.params(depthMin=0.5, depthMax=8.05, depthTolerance=0.05, depthToleranceLin=0.01, minCos=0.1, patchSize=8, atlasWidth=256)
    return dict(name="sphere", family="sphere", pos=pos, col=col, faces=faces, frames=base["frames"], w=base["w"], h=base["h"], K=base["K"], params=p, expect={})


def resized(case, nf, frames=None, **params):
    """the case with its faces repeated or cut to nf, other params, the first `frames` frames"""
    idx = np.arange(nf) % len(case["faces"])
    return dict(case, faces=case["faces"][idx], params=dict(case["params"], **params), frames=case["frames"] if frames is None else case["frames"][:frames])
