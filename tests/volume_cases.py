"""Planted volumes for the two consumers of the voxel hash (csrc/mesh.hip, csrc/raycast.hip, the look-up of csrc/bf_volume.h), shared by
tests/test_volume_consumers_edge_cpu.py (the oracle pinned to the reference's own kernels on these volumes, and the proof that the volumes
hold the cases they are named after) and tests/test_volume_consumers_edge_gpu.py (the HIP kernels held to the oracle bit for bit).

A volume is ALLOCATED by integrating synthetic frames (160x120 or smaller, 20 mm voxels, exact contract): table, heap and block pointers are
then bit-equal on the device and in the oracle.  It is PLANTED by overwriting whole 512-voxel blocks, addressed by block key and looked up
in each scene's own hash: the same 12-byte records go into the oracle's voxel array, the compiled reference's and the device's.

Marching cubes (plant_mc).  A cell at voxel p reads the 3x3x3 voxels around p: each of its 8 corner values is the mean of a 2x2x2
sub-cube.  Cells at the local coordinates (1|4)^3 of a block have disjoint neighbourhoods inside the block, so 8 cells per block get any
wanted corner values by the least-norm solution of the 8x27 system (numpy.linalg.pinv):
  (a) cases    all 256 cube cases, targets +-(0.3..0.8) voxel, in 32 blocks;
  (b) interp   corners within / beyond 1e-5 of the iso value, |d1 - d2| below / above 1e-5, +0.0 / -0.0 corners, voxels of -0.0 and
               +-1e-40 (denormal), and cells whose largest opposite-sign pair sum or largest |d| straddles GATE_THRESHOLDS (the first
               gate alone drops some, the second gate alone drops some, their neighbours just inside both are kept);
  (c) weights  27 cells, the k-th with weight 0 at the k-th voxel of its neighbourhood and nowhere else; and `full` blocks (every weight 1,
               a plane through the block) chosen among the blocks with the fewest allocated neighbours: their face, edge and corner cells
               read blocks that are absent - or, in the tight hash, were dropped by a full bucket;
  (d) box      box_on_cells: corners that are the float32 positions of two emitting cells, both bounds inclusive.
Every planted voxel has its own colour, bytes 0 and 255 among them, fourth byte never 0.

Ray cast.  (e) plant_holes: in every block of the volume a seeded 2 % of the observed voxels lose their weight, the others move by up to
3 mm and get random colours.  (f) near_camera_pose: 50 mm voxels and a pose inside the allocated band, so that the frustum list holds blocks
with corners on both sides of camera z = 0 and blocks across each of the four image borders (near_camera_facts states it in numpy).

Measured on the oracle (tests/test_volume_consumers_edge_cpu.py prints these on every run and asserts the conditions on them):
  natural volume (roomy hash): 351 blocks, 62918 cells with all 27 weights, 15116 triangles (the float64 recomputation predicts exactly that), 4 emitting cases;
    tight hash (80 buckets): 291 blocks, 126 insertions dropped, 22 chained entries, 11898 triangles.
  planted, roomy: 19889 triangles (recomputation 19895: cells with a corner value within float32 rounding of 0), all 256 case indices among the 54513 cells that pass
    the gates, 252 of them emit (edge masks 0 and 255 emit nothing, in the reference too).  tight: 16936 triangles (recomputation 16944), 256 / 252 as well.
  (b) 32 cells: under GATE_THRESHOLDS gate 1 alone drops 2, gate 2 alone 2, 26 emit; 11 have a corner within 1e-5 of 0 and 6 one just beyond.  Over the whole volume
    these thresholds drop 2 / 13894 cells by gate 1 / gate 2 alone and keep 40614.
  (c) restoring the 27 weights adds 487 triangles (20376 against 19889); cells emptied only by an absent block: 1502 on a face, 464 on an edge, 55 at a corner
    (tight: 3978 / 2029 / 225, of which 2676 / 1752 / 212 read one of the 60 keys that full buckets dropped); 86 emitting cells have a voxel coordinate 0 and
    read voxel -1 of block -1, 4440 have a negative coordinate.
  (d) roomy: 1314 triangles in the box, 105 with the bounds one float32 step inside; every one of the six bounds holds between 10 and 597 emitting cells.
  (e) 160x120 from frame 20: 17645 hits on the natural volume, 11963 planted (1762 weights set to 0).  Against the same planted sdf and colours with every weight
    kept (17643 hits): 5680 pixels lose or move their hit, 1998 keep their depth bits and get another analytic-gradient normal (the partial sums of a gradient tap
    that fails).  TIGHT_GATES: m_thresSampleDist alone keeps 6092 of the 11963 hits, m_thresDist alone 5609, both 2108.
  (f) 8 blocks in the frustum list, 1 with corners on both sides of camera z = 0; 1 / 2 / 1 / 4 blocks wholly in front across the left / right / top / bottom border;
    all 19200 pixels covered, 3877 hit.
  hits per image size 1x1 / 7x5 / 67x9 / 65x41 / 160x120: (e) 1 / 20 / 384 / 1669 / 11963, (f) 1 / 6 / 120 / 533 / 3877 (1x1 from pose_for_size: from the
    volume's own pose its single ray, through the principal point, passes the surface by).
  splat_poses: all 32 have blocks in their frustum list (1 to 27) and cover pixels; 10 of them have a block with corners on both sides of camera z = 0.
"""
import numpy as np

from bundlefusion_amd import synth
from bundlefusion_amd.capi import default_hash_params, camera_params, FREE_ENTRY, VOX_PER_BLOCK, VOXEL_DTYPE, _h2d

W, H, VOXEL = 160, 120, 0.02
ROOMY = dict(num_buckets=20011, num_sdf_blocks=4000)
TIGHT = dict(num_buckets=80, num_sdf_blocks=4000)             # load factor > 1: overflow chains, and keys dropped by full buckets
CHAINED = dict(num_buckets=170, num_sdf_blocks=4000)          # overflow chains and no drops: WHICH keys a full bucket drops depends on the order of arrival, so the
#                                                                compiled reference (a serial emulation) keeps another key set than the oracle under TIGHT, the same under CHAINED
DEFAULT_THRESHOLDS = (10.0 * VOXEL, 10.0 * VOXEL)
GATE_THRESHOLDS = (0.10, 0.07)                                 # thresh != thresh2: the planted gate cells straddle these

# corner (sx, sy, sz) -> bit of the case index (MarchingCubesSDFUtil.h: 1 = d010, 2 = d110, 4 = d100, 8 = d000, 16 = d011, 32 = d111, 64 = d101, 128 = d001)
CORNER_BIT = {(0, 1, 0): 1, (1, 1, 0): 2, (1, 0, 0): 4, (0, 0, 0): 8, (0, 1, 1): 16, (1, 1, 1): 32, (1, 0, 1): 64, (0, 0, 1): 128}
CORNERS = sorted(CORNER_BIT)                                   # a fixed order of the 8 corners for target vectors
CELLS = [(x, y, z) for z in (1, 4) for y in (1, 4) for x in (1, 4)]      # local coordinates of the 8 planted cells of a block


def room_frames(ks=(0, 20, 40), w=W, h=H):
    frames = [synth.scene_room(k, w, h) for k in ks]
    K = frames[0][3]
    return frames, camera_params(w, h, K["fx"], K["fy"], K["mx"], K["my"])


def hash_map(scene):
    h = scene.hash()
    return {tuple(int(v) for v in e["pos"]): int(e["ptr"]) for e in h[h["ptr"] != FREE_ENTRY]}


class Planted:
    """One volume in up to three scenes: the oracle's, the compiled reference's (ref_api given) and the device's (gpu given)."""

    def __init__(self, oracle, p, frames, cam, ref_api=None, gpu=None):
        self.p, self.cam = p, cam
        self.osc = oracle.OracleScene(p)
        self.rsc = ref_api.RefScene(p) if ref_api is not None else None
        self.gs = None
        if gpu is not None:
            import torch
            self.gs = gpu.capi.SceneRepHashSDF(p)
            self.gs.set_arith("exact")
            self.d_vox = self.gs.hash_data().d_SDFBlocks        # (asked for before the first operator, see tests/test_volume_chain_gpu.py)
        for d, c, T, _ in frames:
            self.osc.integrate(T, d, c, cam, threads=16)
            if self.rsc is not None:
                self.rsc.integrate(T, d, c, cam)
            if self.gs is not None:
                self.gs.integrate(T, torch.from_numpy(np.ascontiguousarray(d)).cuda(), torch.from_numpy(np.ascontiguousarray(c)).cuda(), cam)
        if self.gs is not None:
            torch.cuda.synchronize()

    def write(self, blocks):
        """blocks: {block key: VOXEL_DTYPE[512]} -> every scene, through its own hash"""
        for sc in (self.osc, self.rsc):
            if sc is None:
                continue
            m, vox = hash_map(sc), sc.voxels()
            for key, rec in blocks.items():
                vox[m[key]:m[key] + VOX_PER_BLOCK] = rec
        if self.gs is not None:
            m = hash_map(self.osc)
            for key, rec in blocks.items():
                _h2d(self.d_vox + m[key] * 12, np.ascontiguousarray(rec))

    def compactify(self, T):
        for sc in (self.osc, self.rsc, self.gs):
            if sc is not None:
                sc.compactify(T, self.cam)


def build(oracle, hash_kw=ROOMY, voxel=VOXEL, ks=(0, 20, 40), w=W, h=H, ref_api=None, gpu=None):
    frames, cam = room_frames(ks, w, h)
    p = default_hash_params(voxel_size=voxel, **hash_kw)
    return Planted(oracle, p, frames, cam, ref_api, gpu), frames


# ------------------------------------------------------------------------------------------------ marching cubes: planting
def _system():
    """A[corner, voxel of the 3x3x3 neighbourhood (z, y, x)] = 1/8 where the corner's 2x2x2 sub-cube holds the voxel"""
    A = np.zeros((8, 27))
    for r, (sx, sy, sz) in enumerate(CORNERS):
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    A[r, ((sz + dz) * 3 + sy + dy) * 3 + sx + dx] = 0.125
    return A


_PINV = np.linalg.pinv(_system())


def neighbourhood_for(targets):
    """least-norm 3x3x3 voxel values [z, y, x] (float32) whose 2x2x2 means are the 8 corner targets (order: CORNERS)"""
    return (_PINV @ np.asarray(targets, np.float64)).astype(np.float32).reshape(3, 3, 3)


def case_targets(ci, rng):
    return [(-1.0 if ci & CORNER_BIT[c] else 1.0) * rng.uniform(0.3, 0.8) * VOXEL for c in CORNERS]


def _by_corner(default, **named):
    """target vector: `default` everywhere, d010=..., d111=... by name"""
    t = [default] * 8
    for name, v in named.items():
        t[CORNERS.index((int(name[1]), int(name[2]), int(name[3])))] = v
    return t


def interp_targets():
    """(b): (name, 8 corner targets)"""
    out = []
    for e in (2e-6, 8e-6, 1.2e-5, 3e-5):                # either side of vertexInterp's 1e-5 bounds
        out.append(("d1 near iso %g" % e, _by_corner(0.01, d000=-e)))
        out.append(("d2 near iso %g" % e, _by_corner(-0.01, d100=e, d110=0.01, d101=0.01, d111=0.01)))
        out.append(("d1 - d2 small %g" % e, _by_corner(0.01, d000=-e, d100=e, d010=e, d001=e)))
    out.append(("+0.0 corner", _by_corner(-0.01, d111=0.0)))
    out.append(("all corners 0", _by_corner(0.0)))
    t, t2 = GATE_THRESHOLDS
    for s in (1.0, -1.0):
        out.append(("gate 1 drops", _by_corner(s * 0.05, d000=s * 0.06, d111=-s * 0.045)))        # 0.105 > thresh, every |d| <= thresh2
        out.append(("gate 1 keeps", _by_corner(s * 0.05, d000=s * 0.05, d111=-s * 0.045)))        # 0.095
        out.append(("gate 2 drops", _by_corner(s * 0.02, d000=s * 0.075, d111=-s * 0.02)))        # 0.095 <= thresh, 0.075 > thresh2
        out.append(("gate 2 keeps", _by_corner(s * 0.02, d000=s * 0.065, d111=-s * 0.02)))
    assert 0.06 + 0.045 > t > 0.05 + 0.045 and 0.075 > t2 > 0.065
    return out


def raw_neighbourhoods():
    """(b): voxel values planted directly: negative zero and denormals (a kernel that flushes them reads a different case index)"""
    a = np.full((3, 3, 3), np.float32(1e-40)); a[:, :, 0] = np.float32(-3e-40)
    b = np.full((3, 3, 3), np.float32(-0.0))
    c = np.full((3, 3, 3), np.float32(-0.0)); c[:, 0, :] = np.float32(-1e-40); c[2] = np.float32(1e-40)
    return [("denormals", a), ("negative zero", b), ("negative zero and denormals", c)]


def _colour(i):
    return (i & 255, (i >> 8) & 255, 255 - (i * 7) % 256, 1 + i % 255)


def _empty_block():
    return np.zeros(VOX_PER_BLOCK, VOXEL_DTYPE)


def _put(rec, cell, nb, weight=None):
    """writes a 3x3x3 neighbourhood (sdf [z,y,x]; weight 1 or the given [z,y,x] array) around the local cell"""
    r = rec.reshape(8, 8, 8)
    cx, cy, cz = cell
    r["sdf"][cz - 1:cz + 2, cy - 1:cy + 2, cx - 1:cx + 2] = nb
    r["weight"][cz - 1:cz + 2, cy - 1:cy + 2, cx - 1:cx + 2] = 1.0 if weight is None else weight


def full_block(j):
    """a block with every weight 1 and a plane (the j-th of six) through it"""
    rec = _empty_block().reshape(8, 8, 8)
    z, y, x = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    n = np.array([[1, 0.43, 0.21], [0.31, 1, -0.53], [-0.23, 0.61, 1], [1, 0.97, 1.03], [1, -1.07, 0.11], [0.053, 0.11, 1]][j])      # (no corner mean lands on 0)
    rec["sdf"] = (0.4 * VOXEL * (n[0] * (x - 3.5) + n[1] * (y - 3.5) + n[2] * (z - 3.5) + 0.0371)).astype(np.float32)
    rec["weight"] = 1.0
    rec["color"] = np.arange(2048, dtype=np.uint32).astype(np.uint8).reshape(8, 8, 8, 4) | 1
    return rec.reshape(-1)


def neighbour_count(keys):
    ks = set(keys)
    return {k: sum((k[0] + dx, k[1] + dy, k[2] + dz) in ks for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)) - 1 for k in ks}


def plant_mc(osc, seed=1, weights_valid=False, families=("cases", "interp", "weights", "full")):
    """-> ({key: records}, info).  Blocks are chosen from the oracle's hash alone.  weights_valid: family (c)'s 27 cells keep weight 1 (the
    volume WITHOUT that plant).  info: family -> [(key, local cell, name)]."""
    rng = np.random.default_rng(seed)
    keys = sorted(hash_map(osc))
    nc = neighbour_count(keys)
    full_keys = sorted(keys, key=lambda k: (nc[k], k))[:6]
    rest = [k for k in keys if k not in set(full_keys)]
    step = len(rest) // 40
    assert step >= 1, "the volume has too few blocks (%d)" % len(keys)
    pool = [rest[i * step] for i in range(40)]
    cells = []                                                                        # (family, name, neighbourhood sdf, weights or None)
    for ci in range(256):
        cells.append(("cases", "case %d" % ci, neighbourhood_for(case_targets(ci, rng)), None))
    for name, t in interp_targets():
        cells.append(("interp", name, neighbourhood_for(t), None))
    for name, nb in raw_neighbourhoods():
        cells.append(("interp", name, nb, None))
    while len(cells) % 8:
        cells.append(("interp", "filler", neighbourhood_for(case_targets(1, rng)), None))
    for k in range(27):
        w = np.ones(27, np.float32)
        if not weights_valid:
            w[k] = 0.0
        cells.append(("weights", "weight 0 at voxel %d" % k, neighbourhood_for(case_targets(1 + 9 * k, rng)), w.reshape(3, 3, 3)))
    blocks, info = {}, {f: [] for f in ("cases", "interp", "weights", "full")}
    colour = 0
    for i, (family, name, nb, w) in enumerate(cells):
        key = pool[i // 8]
        if family not in families:
            continue
        rec = blocks.setdefault(key, _empty_block())
        _put(rec, CELLS[i % 8], nb, w)
        info[family].append((key, CELLS[i % 8], name))
    if "full" in families:
        for j, key in enumerate(full_keys):
            rec = full_block(j)
            blocks[key] = rec
            info["full"].append((key, None, "full block with %d neighbours" % nc[key]))
    for key in sorted(blocks):
        for v in range(VOX_PER_BLOCK):
            blocks[key]["color"][v] = _colour(colour); colour += 1
    return blocks, info


# ------------------------------------------------------------------------------------------------ marching cubes: float64 recomputation
def _dense(hash_np, vox_np):
    """the volume as dense arrays [z, y, x] with one block of margin: sdf (float64), weight != 0, voxel belongs to an allocated block; and the
    block coordinate of the array's origin"""
    occ = hash_np[hash_np["ptr"] != FREE_ENTRY]
    pos = occ["pos"].astype(np.int64)
    lo = pos.min(0) - 1
    nb = pos.max(0) - lo + 2
    b = pos - lo
    v = vox_np.reshape(-1, VOX_PER_BLOCK)[occ["ptr"] // VOX_PER_BLOCK]
    sdf = np.zeros((nb[2], 8, nb[1], 8, nb[0], 8)); wt = np.zeros(sdf.shape, bool); own = np.zeros(sdf.shape, bool)
    sdf[b[:, 2], :, b[:, 1], :, b[:, 0], :] = v["sdf"].reshape(-1, 8, 8, 8)
    wt[b[:, 2], :, b[:, 1], :, b[:, 0], :] = v["weight"].reshape(-1, 8, 8, 8) != 0
    own[b[:, 2], :, b[:, 1], :, b[:, 0], :] = True
    shape = (nb[2] * 8, nb[1] * 8, nb[0] * 8)
    return sdf.reshape(shape), wt.reshape(shape), own.reshape(shape), lo


def absent_neighbour_cells(hash_np, vox_np, among=None):
    """(c): cells of allocated blocks that are empty ONLY because part of their 3x3x3 neighbourhood lies in a block the hash does not hold
    (every voxel of it that the hash does hold has weight) -> their number by how many axes they sit on the block boundary: {1: on a face,
    2: on an edge, 3: at a corner}.  among: count only cells that read a block of this set of keys (the keys a full bucket dropped)."""
    sdf, wt, own, lo = _dense(hash_np, vox_np)
    if among is not None:
        hit = np.zeros((own.shape[0] // 8, own.shape[1] // 8, own.shape[2] // 8), bool)
        for k in among:
            c = np.array(k) - lo
            if (c >= 0).all() and c[2] < hit.shape[0] and c[1] < hit.shape[1] and c[0] < hit.shape[2]:
                hit[c[2], c[1], c[0]] = True
        hit = np.repeat(np.repeat(np.repeat(hit, 8, 0), 8, 1), 8, 2) & ~own
    ok = own.copy(); reads_absent = np.zeros(own.shape, bool)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                sh = lambda a: np.roll(a, (-dz, -dy, -dx), (0, 1, 2))
                ok &= sh(wt) | ~sh(own)
                reads_absent |= sh(hit) if among is not None else ~sh(own)
    z, y, x = np.nonzero(ok & reads_absent)
    axes = sum(((c % 8 == 0) | (c % 8 == 7)).astype(int) for c in (x, y, z))
    return {k: int((axes == k).sum()) for k in (1, 2, 3)}


def mc_predict(hash_np, vox_np, voxel, thresh, thresh2, edge_table, tri_table, box=None):
    """Every cell of every allocated block, recomputed in float64 numpy with corner weights of exactly 1/8 (the kernels' float32 weights
    differ from 1/8 by rounding, so a cell whose gate sum lies within that of a threshold may be decided the other way).
    -> dict of arrays over the cells whose 27 voxels all have weight: pos [n,3] (voxel coordinates), ci, gate1 / gate2 (True = dropped by
    it), ntri (0 where dropped), and the scalar `cells` (number of valid cells)."""
    sdf, wt, own, lo = _dense(hash_np, vox_np)
    ok = own.copy()
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok &= np.roll(wt, (-dz, -dy, -dx), (0, 1, 2))                      # (the margin keeps the wrap-around out of allocated cells)
    z, y, x = np.nonzero(ok)
    d = np.zeros((len(z), 8))
    for r, (sx, sy, sz) in enumerate(CORNERS):
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    d[:, r] += 0.125 * sdf[z - 1 + sz + dz, y - 1 + sy + dy, x - 1 + sx + dx]
    ci = np.zeros(len(z), np.int64)
    for r, c in enumerate(CORNERS):
        ci += np.where(d[:, r] < 0, CORNER_BIT[c], 0)
    a, bb = d[:, :, None], d[:, None, :]
    pair = np.where(a * bb < 0, np.abs(a) + np.abs(bb), np.abs(a - bb))
    gate1 = (pair > thresh).any(axis=(1, 2))
    gate2 = (np.abs(d) > thresh2).any(axis=1)
    p = np.stack([x + lo[0] * 8, y + lo[1] * 8, z + lo[2] * 8], 1)
    keep = ~gate1 & ~gate2
    if box is not None:
        wp = p.astype(np.float32) * np.float32(voxel)
        keep &= ((wp >= np.float32(box[0])) & (wp <= np.float32(box[1]))).all(axis=1)
    e = np.asarray(edge_table).astype(np.int64)[ci]
    ntri = (np.asarray(tri_table).reshape(256, 16)[ci] >= 0).sum(axis=1) // 3
    ntri = np.where(keep & (e != 0) & (e != 255), ntri, 0)
    return dict(pos=p, ci=ci, d=d, gate1=gate1, gate2=gate2, ntri=ntri, cells=len(z))


def box_on_cells(pred, voxel, half=12):
    """(d): a box of about 2 * half voxels around the median emitting cell, then tightened to the emitting cells it holds: each of its six
    bounds is the float32 position of an emitting cell inside it.  -> ((min corner, max corner) in metres, (lo, hi) in voxel coordinates)"""
    em = pred["pos"][pred["ntri"] > 0]
    c = em[np.lexsort(em.T[::-1])][len(em) // 2]
    inside = em[(np.abs(em - c) <= half).all(axis=1)]
    lo, hi = inside.min(axis=0), inside.max(axis=0)
    f = lambda v: [float(np.float32(x) * np.float32(voxel)) for x in v]
    return (f(lo), f(hi)), (lo, hi)


def shrink_box(box):
    """the same box one float32 step smaller on every side: what an exclusive bound would extract"""
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    dn = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))
    return [up(v) for v in box[0]], [dn(v) for v in box[1]]


# ------------------------------------------------------------------------------------------------ ray cast
def plant_holes(osc, seed=5, fraction=0.02, move=0.003):
    """(e) -> {key: records} for every block of the volume"""
    rng = np.random.default_rng(seed)
    m, vox = hash_map(osc), osc.voxels()
    blocks = {}
    for key in sorted(m):
        rec = vox[m[key]:m[key] + VOX_PER_BLOCK].copy()
        seen = rec["weight"] > 0
        rec["sdf"] = np.where(seen, rec["sdf"] + rng.uniform(-move, move, VOX_PER_BLOCK).astype(np.float32), rec["sdf"]).astype(np.float32)
        rec["weight"] = np.where(seen & (rng.random(VOX_PER_BLOCK) < fraction), np.float32(0), rec["weight"])
        rec["color"] = rng.integers(0, 256, (VOX_PER_BLOCK, 4), dtype=np.uint8)
        blocks[key] = rec
    return blocks


def ray_params(K, w, h, use_gradients=1, increment=0.8 * 0.06, thres_sample=None, thres_dist=None, max_vertices=6 * 20000, src=(W, H), dmin=0.1, dmax=4.0):
    """RayCastParams for a w x h image, intrinsics scaled from the src size as tests/test_ref_pin_cpu.py does; the thresholds default to
    the application's 50.5 / 50 increments (which never fire on a truncated sdf)"""
    from bundlefusion_amd.capi import RayCastParams
    rp = RayCastParams()
    rp.m_width, rp.m_height = w, h
    rp.fx, rp.fy = K["fx"] * w / src[0], K["fy"] * h / src[1]
    rp.mx, rp.my = K["mx"] * (w - 1) / (src[0] - 1), K["my"] * (h - 1) / (src[1] - 1)
    rp.m_minDepth, rp.m_maxDepth = dmin, dmax
    rp.m_rayIncrement = increment
    rp.m_thresSampleDist = 50.5 * increment if thres_sample is None else thres_sample
    rp.m_thresDist = 50.0 * increment if thres_dist is None else thres_dist
    rp.m_useGradients = use_gradients
    rp.m_maxNumVertices = max_vertices
    return rp


def with_view(oracle, rp, T):
    Tinv = oracle.inverse44(np.asarray(T, np.float32))
    rp.m_viewMatrix[:] = [float(v) for v in Tinv.reshape(16)]
    rp.m_viewMatrixInverse[:] = [float(v) for v in np.asarray(T, np.float32).reshape(16)]
    return rp


TIGHT_GATES = dict(thres_sample=0.045, thres_dist=0.03)        # about the sdf step between two samples of a ray / half of it: each gate removes about half of the hits
SECOND_INCREMENT = 0.031

NEAR_VOXEL = 0.05
NEAR_ADVANCE, NEAR_YAW, NEAR_PITCH = 0.5, -0.6, 0.35          # frame 20's pose moved along its viewing direction into the allocated band, then turned


def near_camera_pose(frames):
    cy, sy, cx, sx = np.cos(NEAR_YAW), np.sin(NEAR_YAW), np.cos(NEAR_PITCH), np.sin(NEAR_PITCH)
    T = frames[1][2].astype(np.float64).copy()
    T[:3, 3] += NEAR_ADVANCE * T[:3, 2]
    T[:3, :3] = T[:3, :3] @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return T.astype(np.float32)


SINGLE_RAY_YAW = 0.3                                           # the central ray of both views passes the surface by; turned by this much it hits


def pose_for_size(T, size):
    """the pose a w x h image is rendered from: T, but for 1x1 (one ray, through the principal point) T turned about the camera's y axis until that ray hits"""
    if tuple(size) != (1, 1):
        return np.asarray(T, np.float32)
    c, s_ = np.cos(SINGLE_RAY_YAW), np.sin(SINGLE_RAY_YAW)
    T1 = np.asarray(T, np.float64).copy()
    T1[:3, :3] = T1[:3, :3] @ np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
    return T1.astype(np.float32)


def near_camera_facts(osc, cam, rp, voxel):
    """(f) from the inputs alone, float64: over the blocks of the oracle's frustum list, how many have corners on both sides of camera
    z = 0, and how many lie wholly in front of the camera with a screen rectangle across the left / right / top / bottom image border"""
    view = np.array(list(rp.m_viewMatrix), np.float64).reshape(4, 4)
    pos = osc.compactified()["pos"].astype(np.float64)
    mn = pos * 8 * voxel - voxel / 2
    facts = dict(blocks=len(pos), straddle_z=0, left=0, right=0, top=0, bottom=0)
    for b in mn:
        c = np.array([[b[0] + (i & 1) * 8 * voxel, b[1] + ((i >> 1) & 1) * 8 * voxel, b[2] + ((i >> 2) & 1) * 8 * voxel, 1.0] for i in range(8)]) @ view.T
        z = c[:, 2]
        if z.min() <= 0 < z.max():
            facts["straddle_z"] += 1
        if z.min() > 0:
            px = c[:, 0] * rp.fx / z + rp.mx + 0.5; py = c[:, 1] * rp.fy / z + rp.my + 0.5      # (to within the splat's viewport scaling)
            facts["left"] += px.min() < 0 < px.max(); facts["right"] += px.min() < rp.m_width < px.max()
            facts["top"] += py.min() < 0 < py.max(); facts["bottom"] += py.min() < rp.m_height < py.max()
    return facts


def _look_at(eye, target, roll):
    """camera-to-world with +z from eye towards target, rolled about the viewing direction"""
    f = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 1.0, 0.0]) if abs(f[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    r = np.cross(up, f); r /= np.linalg.norm(r)
    d = np.cross(f, r)
    c, s_ = np.cos(roll), np.sin(roll)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = c * r + s_ * d, -s_ * r + c * d, f, eye
    return T


def splat_poses(osc, frames, voxel, n=32, seed=11):
    """(the splat) n camera-to-world poses, every one with blocks in its frustum list: the near-camera pose; views from INSIDE the allocated region (the
    camera at the centre of an allocated block, looking at the centre of an allocated neighbour); views from a fraction of a block in front of a
    block's centre, looking past it (corners behind the camera); and poses along and off the stream"""
    rng = np.random.default_rng(seed)
    keys = sorted(hash_map(osc))
    ks = set(keys)
    pairs = [(k, (k[0] + dx, k[1] + dy, k[2] + dz)) for k in keys for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
             if (dx, dy, dz) != (0, 0, 0) and (k[0] + dx, k[1] + dy, k[2] + dz) in ks]
    centre = lambda k: (np.array(k, np.float64) * 8 + 3.5) * voxel
    poses = [near_camera_pose(frames)]
    while len(poses) < n:
        kind = len(poses) % 4
        if kind in (1, 3):
            a, b = pairs[int(rng.integers(len(pairs)))]
            T = _look_at(centre(a), centre(b), rng.uniform(0, 2 * np.pi))
        elif kind == 2:
            b = centre(keys[int(rng.integers(len(keys)))])
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            dist = rng.uniform(2.3, 3.5) * voxel                                        # the block's centre 0.29 to 0.44 of a block ahead: inside the frustum test's
            u = np.cross(d, rng.normal(size=3)); u /= np.linalg.norm(u)                 # depth range (>= 0.1 m at 50 mm voxels), its near corners behind the camera
            T = _look_at(b - dist * d, b + dist * np.tan(rng.uniform(0, 0.3)) * u, rng.uniform(0, 2 * np.pi))
        else:
            base = frames[int(rng.integers(len(frames)))][2].astype(np.float64)
            T = base.copy()
            T[:3, 3] = base[:3, 3] + rng.uniform(0.0, 0.4) * base[:3, 2] + rng.normal(0, 0.05, 3)
        poses.append(T.astype(np.float32))
    return poses
