"""Planted frames for the point-cloud tests (tests/test_point_cloud_cpu.py, tests/test_point_cloud_gpu.py).  Every case is a dict
    name, family, frames [(depth (h, w) f32, colour (h, w, 4) u8, pose (4, 4) f32)], Kinv (4, 4) f32, cell, max_depth, rules
`rules`: the rule codes of tests/point_cloud_ref.py that the case's family is named for; the CPU test proves that each drops a pixel and that pixels are kept.

Inverse intrinsics, poses and depths are powers of two and small integers, cellSize is 2^-7: positions and cell boundaries are exactly representable, so a
boundary point sits ON the boundary and the families test what they say."""
import numpy as np

from tests import point_cloud_ref as R

F = np.float32
CELL = 2.0 ** -7
MAX_DEPTH = 3.5
NINF, PINF, NAN = F(-np.inf), F(np.inf), F(np.nan)


def kinv(sx, sy=None, ox=0.0, oy=0.0):
    """p = (sx * x * d + ox * d, sy * y * d + oy * d, d)"""
    K = np.eye(4, dtype=F)
    K[0, 0] = sx; K[1, 1] = sx if sy is None else sy; K[0, 2] = ox; K[1, 2] = oy
    return K


def pose(tx=0.0, ty=0.0, tz=0.0, rot=None):
    T = np.eye(4, dtype=F)
    if rot is not None:
        T[:3, :3] = rot
    T[:3, 3] = [tx, ty, tz]
    return T


ROT_Z90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)


def colours(h, w, rng):
    c = rng.integers(1, 256, (h, w, 4)).astype(np.uint8)          # never black
    return c


def flat(h, w, d=1.0):
    return np.full((h, w), d, F)


def _case(name, family, frames, K, rules, cell=CELL, max_depth=MAX_DEPTH):
    return dict(name=name, family=family, frames=frames, Kinv=K, cell=cell, max_depth=max_depth, rules=tuple(rules))


def gate_cases():
    rng = np.random.default_rng(11)
    out = []
    K = kinv(2.0 ** -6)
    # depth -inf, +inf, NaN, 0, negative: at the centre pixel of a 7x7 frame and at each of its four neighbours in turn
    frames = []
    for v in (NINF, PINF, NAN, F(0), F(-1)):
        for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
            D = flat(7, 7) + (rng.integers(0, 4, (7, 7)) * 2.0 ** -9).astype(F)
            D[3 + dy, 3 + dx] = v
            frames.append((D, colours(7, 7, rng), pose(tx=0.25 * len(frames))))
    out.append(_case("depth_specials", "depth", frames, K, (R.NO_POSITION, R.NEIGHBOUR)))
    # p.z just below, equal to and just above maxDepth: at a pixel (dropped from `equal` on) - its neighbours stay, maxDepth does not apply to neighbours
    md = F(2.0)
    D = flat(7, 11, 1.5)
    D[3, 2] = np.nextafter(md, F(0)); D[3, 5] = md; D[3, 8] = np.nextafter(md, F(4))
    out.append(_case("max_depth", "maxDepth", [(D, colours(7, 11, rng), pose())], K, (R.MAX_DEPTH,), max_depth=2.0))
    out[-1]["expect"] = [(0, 3, 2, R.KEPT), (0, 3, 5, R.MAX_DEPTH), (0, 3, 8, R.MAX_DEPTH)] + [(0, 3 + dy, x + dx, R.KEPT) for x in (5, 8) for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1))]
    # the image border
    out.append(_case("border", "border", [(flat(5, 6), colours(5, 6, rng), pose())], K, (R.BORDER,)))
    # a zero cross product: rows 0 and 1 of Kinv are zero, every position is (0, 0, d); the family's other case is the same frame with a camera
    K0 = np.eye(4, dtype=F); K0[0, 0] = 0; K0[1, 1] = 0
    Dz = flat(6, 7) + (rng.integers(0, 8, (6, 7)) * 2.0 ** -8).astype(F)
    Cz = colours(6, 7, rng)
    out.append(_case("zero_cross", "normal", [(Dz, Cz, pose())], K0, (R.NORMAL,)))
    out.append(_case("nonzero_cross", "normal", [(Dz, Cz, pose())], K, ()))
    # colour (0, 0, 0, X) dropped, (0, 0, 1, X) kept
    C = colours(6, 7, rng)
    C[2, 2] = [0, 0, 0, 77]; C[2, 4] = [0, 0, 1, 0]; C[3, 3] = [0, 1, 0, 0]; C[3, 5] = [1, 0, 0, 0]
    out.append(_case("black", "colour", [(flat(6, 7), C, pose())], K, (R.COLOUR,)))
    out[-1]["expect"] = [(0, 2, 2, R.COLOUR), (0, 2, 4, R.KEPT), (0, 3, 3, R.KEPT), (0, 3, 5, R.KEPT)]
    # poses: T[0] = -inf (the reference's invalid pose), T[0] = NaN, a translation that is +inf, and translations of +-2^24 = +-2^31 cells: +2^31 does not fit
    # an int32 (dropped), -2^31 does (kept: the float sum rounds back onto -2^24)
    Tm = np.full((4, 4), NINF, F)
    Tn = pose(); Tn[0, 0] = NAN
    frames = [(flat(5, 6), colours(5, 6, rng), T) for T in (pose(tx=0.5), Tm, Tn, pose(ty=np.inf), pose(tx=2.0 ** 24), pose(tx=-2.0 ** 24), pose(tz=2.0 ** 24), pose(tx=1.0, rot=ROT_Z90))]
    out.append(_case("poses", "pose", frames, K, (R.POSE, R.WORLD, R.CELL_RANGE)))
    return out


def thinning_cases():
    rng = np.random.default_rng(23)
    out = []
    # one cell wanted by every candidate of three frames: positions x * d * 2^-14 < 2^-10, z in [1, 1 + 2^-7), translations of a few 2^-12; every candidate has
    # its own position, normal and colour
    Ks = kinv(2.0 ** -14)
    frames = []
    for f in range(3):
        D = (1.0 + rng.integers(0, 48, (6, 8)) * 2.0 ** -13).astype(F)
        frames.append((D, colours(6, 8, rng), pose(tx=f * 2.0 ** -12, ty=(2 - f) * 2.0 ** -12, tz=f * 2.0 ** -12)))
    out.append(_case("one_cell", "one cell", frames, Ks, ()))
    # some 60 cells contended from all over three frames
    Kp = kinv(2.0 ** -10)
    frames = []
    for f in range(3):
        D = (1.0 + rng.integers(0, 7 * 16, (18, 24)) * 2.0 ** -11).astype(F)
        frames.append((D, colours(18, 24, rng), pose(tx=f * 2.0 ** -9)))
    out.append(_case("pool", "pool", frames, Kp, ()))
    # all cells distinct: two cells per pixel step, the second frame shifted by half a metre
    Kd = kinv(2.0 ** -6)
    out.append(_case("distinct", "distinct", [(flat(6, 8), colours(6, 8, rng), pose()), (flat(6, 8), colours(6, 8, rng), pose(tx=0.5))], Kd, ()))
    # points exactly on cell boundaries and in the middle of cells on both sides of 0: p = ((x - 4) / 256, (y - 3) / 256, 1); the second frame one cell lower in x
    Kb = kinv(2.0 ** -8, ox=-4 * 2.0 ** -8, oy=-3 * 2.0 ** -8)
    out.append(_case("boundaries", "boundaries", [(flat(8, 10), colours(8, 10, rng), pose(tz=-1.0)), (flat(8, 10), colours(8, 10, rng), pose(tx=-CELL, tz=-1.0))], Kb, ()))
    # cellSize <= 0: every candidate is a point
    for cell in (0.0, -1.0):
        out.append(_case("no_thinning_%g" % cell, "no thinning", out[0]["frames"], Ks, (), cell=cell))
    return out


def all_cases():
    return gate_cases() + thinning_cases()


def random_frame(w, h, seed, scale=2.0 ** -6, spread=0.5):
    """a frame of the given size with every kind of pixel sprinkled in: invalid depths, depths beyond maxDepth, black pixels; cells contended (spread small) or not"""
    rng = np.random.default_rng(seed)
    D = (1.0 + rng.integers(0, 256, (h, w)) * (spread / 256.0)).astype(F)
    r = rng.random((h, w))
    D[r < 0.03] = NINF; D[(r >= 0.03) & (r < 0.04)] = NAN; D[(r >= 0.04) & (r < 0.05)] = 0; D[(r >= 0.05) & (r < 0.06)] = 4.0; D[(r >= 0.06) & (r < 0.065)] = PINF
    C = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    C[rng.random((h, w)) < 0.03, :3] = 0
    return D, C


def distinct_frame(w, h, seed):
    """every interior pixel a candidate in a cell of its own: p = (x / 64, y / 64, 1 + k / 128) - two cells per pixel step"""
    rng = np.random.default_rng(seed)
    D = (1.0 + rng.integers(0, 2, (h, w)) * 2.0 ** -12).astype(F)
    return D, colours(h, w, rng)
