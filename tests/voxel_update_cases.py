"""Planted voxel states under flat frames, for the four voxel-update kernels (k_update_col / k_update_apx in csrc/tsdf.hip, k_update_batch_col /
k_update_batch_apx in csrc/tsdf_batch.h).  Shared by tests/test_voxel_update_cases_cpu.py (the oracle held to the float64 restatement of
tests/voxel_update_ref.py, and the proof that the volumes hold the cases they are named after) and tests/test_voxel_update_cases_gpu.py.

A frame is ONE depth and ONE colour: a voxel's sample, sdf = D - z_cam, does not depend on the pixel its projection falls into, so no voxel has to be
excluded near a pixel boundary; validity and weights must agree exactly between the contracts.  Variety comes from the voxel STATE: a volume is allocated
by integrating the frames A and B at the identity (64 x 48 pixels, 5003 buckets, 2000 blocks), then every allocated block is overwritten
(tests/volume_cases.Planted.write) with states that a sequence of operators could have produced: integer weights with alpha 255, or the all-zero voxel.

  weights   WEIGHTS (0 .. 65535, around 255 / 1024 / 1593 / 2000), under a weight cap those up to the cap, the cap and the cap - 1;
  sdf       uniform in the truncation band; +0.0 / -0.0; +-1e-40 (denormal) / +-1e-20; and CANCELLING voxels whose float32 product sdf * w equals the
            sample s (de-integration numerator sdf * w - s = 0) or -s (integration numerator 0) of frame A at the identity, at w = 2 and at a large w.
            Frame A's depth is the z of slice K0, so s = 0 there: the tiny sdf classes give numerators of 0 and below 2^-60 (divStored's literal division);
  colour    random bytes 0 .. 254; the bytes 0, 1, 127, 128, 254; and TIES: (o, w) with w = 3 or 5 whose de-integration quotient (o w - c) / (w - 1) under
            frame A's colour is an exact half-integer, drawn mostly from the ties next to 0 (negative ones among them) and next to 254.5 (both sides).
Frames: A, B, C (three depths about 1.5 voxels apart, colour bytes 0 and 255 among them); NOCOL (no colour image), NEGINF (depth -inf), ZERO (depth 0);
E_BELOW / E_ON / E_ABOVE: depths found by search at which one slice has |sdf| exactly one float32 step below / on / one step above
m_truncation + m_truncScale D (under the identity z_cam is the stored float32 z and D - z is exact, so the bound is decided on known bits);
MAXD / MAXD_BELOW (configuration `narrow`): D = m_maxIntegrationDistance and one float32 step below it, over blocks that A and B allocated.
Poses: the identity, a translation, a rotation of 3 degrees about an oblique axis (no edge frame is used under it).

Measured on the oracle (tests/test_voxel_update_cases_cpu.py prints these on every run and asserts FACTS on them):
  default: 190 blocks (120 without the edge depths); ("de" / "in", A, identity) updates 21467 voxels, 740 to 2966 per planted weight, all 8 z-slices in every class;
    1926 de-integration numerators are 0 (246 of them -0.0), 288 non-zero below 2^-60, 1939 integration numerators are 0; every cancelling voxel was found
    (1981 at w = 2, 1168 at w = 1024 / 1593 / 65535); 13014 colour channels on a tie (2345 negative, 2512 in (0, 5), 2301 in (249.5, 254.5), 2167 from 254.5 up).
  caps: at weight_max 1 / 2 / 4 / 255, 10416 / 9181 / 2764 / 1523 voxels at the cap change sdf under an integration and keep the weight; a de-integration
    leaves them at cap - 1.  fine: 210 blocks, 69471 voxels updated; coarse: 44 blocks, 4096 (138 or more per weight); narrow: 72 blocks, 17125.
  edge depths (default): 1.1428571 leaves slice 53 one step inside the bound (2655 voxels updated), 0.92156863 puts slice 50 ON it and 1.1836735 slice 55 one step
    beyond (0 updated, 2255 / 2961 in the next slice inwards); narrow: D = m_maxIntegrationDistance updates 0 voxels, one step below 15516.
  emptied: 48 of 190 blocks are emptied by one de-integration and collected.  Image bounds: no projection within 1.66e-3 px (identity), 1.78e-3 (translation),
    4.66e-3 (rotation, coarse).  Oracle to float64: sdf within 6.8e-7 x truncation (identity, translation), 4.5e-6 (rotation at 2 m), colours all equal.
"""
import numpy as np

from bundlefusion_amd import synth
from bundlefusion_amd.capi import default_hash_params, camera_params, FREE_ENTRY, VOX_PER_BLOCK, VOXEL_DTYPE

from tests import voxel_update_ref as ref
from tests.volume_cases import Planted, hash_map

W, H = 64, 48
HASH = dict(num_buckets=5003, num_sdf_blocks=2000)
BATCH_MAX = 12

WEIGHTS = [0, 1, 2, 3, 4, 5, 9, 254, 255, 256, 1023, 1024, 1592, 1593, 1999, 2000, 2001, 65535]
LARGE_CANCEL = [1024, 1593, 65535]

# name -> (hash parameters, slice K0 whose z is frame A's depth)
CONFIGS = {
    "default": (dict(voxel_size=0.02), 51),
    "cap1": (dict(voxel_size=0.02, weight_max=1), 51),
    "cap2": (dict(voxel_size=0.02, weight_max=2), 51),
    "cap4": (dict(voxel_size=0.02, weight_max=4), 51),
    "cap255": (dict(voxel_size=0.02, weight_max=255), 51),
    "fine": (dict(voxel_size=0.004), 50),
    "coarse": (dict(voxel_size=0.05), 40),
    "narrow": (dict(voxel_size=0.02, truncation=0.03, trunc_scale=0.04, max_integration_distance=1.07), 51),
}

COL_A, COL_B, COL_C, COL_E = (0, 255, 100, 255), (255, 0, 37, 255), (17, 128, 254, 255), (90, 10, 200, 255)

IDENT = np.eye(4, dtype=np.float32)
# With the principal point at the image centre the lattice puts whole columns of voxels ON an image bound (4 mm voxels: x = -30 voxels at z = 53 voxels projects
# to hx = -1 to within 1e-6 px).  Moved by this much no voxel of any configuration comes within 1e-3 px of a bound under any pose (asserted in the CPU file).
PRINCIPAL_SHIFT = (0.37, -0.29)


def _pose(axis, deg, t):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T[:3, 3] = t
    return T.astype(np.float32)


T_TR = _pose((0, 0, 1), 0.0, (0.013, -0.007, 0.011))
T_ROT = _pose((0.27, 1.0, 0.29), 3.21, (0.017, -0.015, 0.009))          # found by search: see scripts_for
POSES = {"identity": IDENT, "translation": T_TR, "rotation": T_ROT}


def poses_for(cfg):
    return [n for n in POSES if n != "rotation" or cfg == "coarse"]

# (kind, frame, T0, T1): "in" integrate(T0), "de" de-integrate(T0), "re" de-integrate(T0) + integrate(T1) of the same frame, fused
SCRIPTS = {
    "integrate": [("in", "A", IDENT, None)],
    "deintegrate": [("de", "A", IDENT, None)],
    "reintegrate": [("re", "A", IDENT, T_TR)],
    "reintegrate_rot": [("re", "A", IDENT, T_ROT)],
    "mixed": [("in", "B", IDENT, None), ("de", "A", IDENT, None), ("re", "B", IDENT, T_TR), ("in", "NOCOL", IDENT, None), ("de", "C", T_TR, None),
              ("in", "A", T_TR, None), ("re", "B", T_TR, IDENT)],
    "mixed_rot": [("in", "B", T_ROT, None), ("de", "A", IDENT, None), ("re", "B", T_ROT, T_TR), ("in", "NOCOL", T_ROT, None), ("de", "C", T_ROT, None),
                  ("in", "A", T_ROT, None), ("re", "B", T_TR, T_ROT)],
    "edge_below": [("de", "E_BELOW", IDENT, None), ("in", "E_BELOW", IDENT, None)],
    "edge_on": [("de", "E_ON", IDENT, None), ("in", "E_ON", IDENT, None)],
    "edge_above": [("de", "E_ABOVE", IDENT, None), ("in", "E_ABOVE", IDENT, None)],
    "nothing": [("in", "NOCOL", IDENT, None), ("de", "NOCOL", IDENT, None), ("in", "NEGINF", IDENT, None), ("de", "NEGINF", IDENT, None),
                ("in", "ZERO", IDENT, None), ("de", "ZERO", IDENT, None), ("re", "NOCOL", IDENT, T_TR)],
    "maxdist": [("in", "MAXD", IDENT, None), ("de", "MAXD", IDENT, None), ("in", "MAXD_BELOW", IDENT, None), ("de", "MAXD_BELOW", IDENT, None)],
}
CORE = ("integrate", "deintegrate", "mixed")


ROTATED = ("reintegrate_rot", "mixed_rot")


def scripts_for(cfg):
    """Every configuration runs the core scripts; the default one all but `maxdist`, which needs the short integration range of `narrow`, and the rotated ones.
    Under a rotation the projections of the lattice are in general position: about one voxel in 10^4 falls within 1e-3 px of an image bound, so only `coarse`,
    whose volume has 2 x 10^4 voxels, runs the rotated scripts, under a rotation chosen so that none does."""
    if cfg == "default":
        return [s for s in SCRIPTS if s != "maxdist" and s not in ROTATED]
    if cfg == "coarse":
        return list(CORE) + list(ROTATED)
    if cfg == "narrow":
        return list(CORE) + ["edge_below", "edge_on", "edge_above", "maxdist"]
    return list(CORE)


def camera():
    K = synth.intrinsics(W, H)
    return camera_params(W, H, K["fx"], K["fy"], K["mx"] + PRINCIPAL_SHIFT[0], K["my"] + PRINCIPAL_SHIFT[1])


def params(cfg):
    return default_hash_params(**HASH, **CONFIGS[cfg][0])


def slice_z(p, k):
    """float32 world z of the voxels with z coordinate k (virtualVoxelPosToWorld)"""
    return np.float32(k) * np.float32(p.m_virtualVoxelSize)


def _step(v, n):
    """the float32 n steps above (n < 0: below) the positive float32 v"""
    return (np.float32(v).view(np.int32) + np.int32(n)).view(np.float32)


def trunc32(p, D):
    return np.float32(p.m_truncation) + np.float32(p.m_truncScale) * np.float32(D)


def edge_depths(p, k0, reach=30):
    """-> {-1, 0, 1: (D, k)}: a float32 depth at which the slice k has |D - z_k|, exact in float32, one step below / on / one step above the truncation
    bound of D.  A slice crosses the bound at one depth in front of it and one behind it, and D - z_k moves in steps of a float32 step of D there, several steps
    of the bound: whether a crossing lands ON the bound is a property of the lattice.  All slices within `reach` of K0 are searched, the nearest wins."""
    t0, ts = float(np.float32(p.m_truncation)), float(np.float32(p.m_truncScale))
    out = {}
    for k in sorted(range(max(2, k0 - reach), k0 + reach + 1), key=lambda k: abs(k - k0)):
        z = slice_z(p, k)
        for sg in (1.0, -1.0):
            Dc = np.float32((float(z) + sg * t0) / (1.0 - sg * ts))
            D = (Dc.view(np.int32) + np.arange(-40, 41, dtype=np.int32)).view(np.float32)
            sdf = np.abs(D - z)                               # Sterbenz: exact
            diff = sdf.view(np.int32).astype(np.int64) - trunc32(p, D).view(np.int32).astype(np.int64)
            for side in (-1, 0, 1):
                j = np.nonzero(diff == side)[0]
                if len(j) and side not in out:
                    out[side] = (D[j[0]], k)
    assert set(out) == {-1, 0, 1}, "no depth puts a slice on the truncation bound"
    return out


def frames(cfg):
    """name -> (depth [H, W] float32, colour [H, W, 4] uint8 or None)"""
    p = params(cfg)
    k0 = CONFIGS[cfg][1]
    vs = np.float32(p.m_virtualVoxelSize)
    D0 = slice_z(p, k0)
    flat = lambda D, c: (np.full((H, W), D, np.float32), None if c is None else np.tile(np.array(c, np.uint8), (H, W, 1)))
    e = edge_depths(p, k0)
    f = {"A": flat(D0, COL_A), "B": flat(D0 + np.float32(1.5) * vs, COL_B), "C": flat(D0 - np.float32(0.75) * vs, COL_C),
         "NOCOL": flat(D0, None), "NEGINF": flat(-np.inf, COL_A), "ZERO": flat(0.0, COL_A),
         "E_BELOW": flat(e[-1][0], COL_E), "E_ON": flat(e[0][0], COL_E), "E_ABOVE": flat(e[1][0], COL_E)}
    md = np.float32(p.m_maxIntegrationDistance)
    f["MAXD"] = flat(md, COL_E); f["MAXD_BELOW"] = flat(_step(md, -1), COL_E)
    return f


def alloc_depths(cfg):
    """the depths whose integration at the identity allocates a configuration's blocks: A and B, and, where the edge scripts run, each edge depth and one voxel
    on either side of it (the slice ON the bound ends the range the allocation walks)"""
    f, vs = frames(cfg), np.float32(CONFIGS[cfg][0]["voxel_size"])
    out = [f["A"][0][0, 0], f["B"][0][0, 0]]
    if "edge_on" in scripts_for(cfg):
        for n in ("E_BELOW", "E_ON", "E_ABOVE"):
            out += [f[n][0][0, 0] - vs, f[n][0][0, 0], f[n][0][0, 0] + vs]
    return out


class Volume(Planted):
    """One configuration's volume in the oracle and, with gpu, on the device (exact contract until set_arith says otherwise)"""

    def __init__(self, oracle, cfg, gpu=None, alloc=None):
        self.cfg, self.frames = cfg, frames(cfg)
        if alloc is None:
            alloc = alloc_depths(cfg)
        super().__init__(oracle, params(cfg), [(np.full((H, W), D, np.float32), self.frames["A"][1], IDENT, None) for D in alloc], camera(), gpu=gpu)
        self.dev = {}
        if gpu is not None:
            import torch
            for n, (d, c) in self.frames.items():
                self.dev[n] = (torch.from_numpy(d).cuda(), None if c is None else torch.from_numpy(c).cuda())

    # ---- the three ways to run a script
    def run_oracle(self, ops, st=None, seen=None):
        """the operators on the oracle and, with st (voxel_update_ref.State), in float64 on st - each over the table its update pass sees.
        -> [(kind, frame, T, idx, ok)] per elementary operator; seen: {voxel index: largest weight it was de-integrated at} is updated"""
        log = []
        for kind, f, T0, T1 in ops:
            d, c = self.frames[f]
            for k, T in ((("de", T0), ("in", T1)) if kind == "re" else ((kind, T0),)):
                (self.osc.deintegrate if k == "de" else self.osc.integrate)(T, d, c, self.cam)
                if st is not None:
                    if k == "de" and seen is not None:
                        idx, ok, _, _ = ref.sample(self.osc.hash(), T, d, c is not None, self.cam, self.p)
                        np.maximum.at(seen, idx[ok], st.weight[idx[ok]])
                    idx, ok = ref.run(k, st, self.osc.hash(), T, d, c, self.cam, self.p)
                    log.append((k, f, T, idx, ok))
        return log

    def run_serial(self, ops):
        for kind, f, T0, T1 in ops:
            d, c = self.dev[f]
            if kind == "re":
                self.gs.reintegrate(T0, T1, d, c, self.cam)
            else:
                (self.gs.deintegrate if kind == "de" else self.gs.integrate)(T0, d, c, self.cam)

    def run_batch(self, ops):
        for i in range(0, len(ops), BATCH_MAX):
            self.gs.run_batch([(kind, T0, T1, self.dev[f][0], self.dev[f][1]) for kind, f, T0, T1 in ops[i:i + BATCH_MAX]], self.cam)

    def garbage_collect(self):
        self.osc.garbage_collect()
        if self.gs is not None:
            self.gs.garbage_collect()


# ------------------------------------------------------------------------------------------------ planting
S_RAND, S_PZERO, S_NZERO, S_PDEN, S_NDEN, S_PTINY, S_NTINY, S_CANCEL_DE, S_CANCEL_IN = range(9)
SDF_CLASSES = ["random", "+0.0", "-0.0", "+1e-40", "-1e-40", "+1e-20", "-1e-20", "cancels the de-integration", "cancels the integration"]
_SDF_P = [0.56, 0.04, 0.04, 0.04, 0.04, 0.05, 0.05, 0.09, 0.09]
C_RAND, C_SPECIAL, C_TIE = range(3)
COLOUR_CLASSES = ["random bytes", "bytes 0 / 1 / 127 / 128 / 254", "de-integration tie"]
_COL_P = [0.6, 0.2, 0.2]


def weights_for(p):
    cap = int(p.m_integrationWeightMax)
    return sorted(set([w for w in WEIGHTS if w <= cap] + ([cap - 1, cap] if cap < 70000 else [])))


def tie_bytes(c, w):
    """stored bytes o in 0 .. 254 for which (o w - c) / (w - 1) is an exact half-integer -> (o, quotient)"""
    o = np.arange(255)
    n = o * w - c
    tie = (2 * n) % (2 * (w - 1)) == (w - 1)
    return o[tie], n[tie] / (w - 1)


def _cancelling(target, w):
    """float32 x with float32(x * w) == target, searched around target / w -> (x, found)"""
    w32 = np.float32(w)
    x0 = (target / w32).astype(np.float32)
    best, found = x0.copy(), np.zeros(len(x0), bool)
    for n in (0, 1, -1, 2, -2, 3, -3):
        x = np.where(x0 == 0, x0, (x0.view(np.int32) + np.int32(n)).view(np.float32))
        hit = ~found & ((x * w32).astype(np.float32) == target)
        best[hit] = x[hit]; found |= hit
    return best, found


def plant(vol, seed=1, emptied=False):
    """Overwrites every allocated block (oracle and device).  -> info: arrays over the whole voxel array (-1 where nothing was planted):
    weight, sdf_class, colour_class; `numerator`: the float32 de-integration numerator sdf * w - s under frame A at the identity.
    emptied: every 4th block instead holds weight 1 exactly where ("de", A, identity) updates it and the all-zero voxel elsewhere: that operator empties them."""
    rng = np.random.default_rng(seed)
    p, cam = vol.p, vol.cam
    h = vol.osc.hash()
    idx, coord, key = ref.voxel_index(h)
    m = len(idx)
    dA, cA = vol.frames["A"]
    _, upd, sA, _ = ref.sample(h, IDENT, dA, True, cam, p)
    sA = (np.float32(dA[0, 0]) - slice_z(p, coord[:, 2])).astype(np.float32)          # the sample where the voxel is valid, exact
    allowed = weights_for(p)
    cap = int(p.m_integrationWeightMax)
    weight = np.array(allowed)[rng.integers(len(allowed), size=m)].astype(np.int64)
    scls = rng.choice(9, size=m, p=_SDF_P)
    ccls = rng.choice(3, size=m, p=_COL_P)
    band = float(p.m_truncation)
    sdf = rng.uniform(-band, band, m).astype(np.float32)
    colour = rng.integers(0, 255, (m, 3)).astype(np.int64)
    # ties: the weight follows the colour class
    tie_w = [w for w in (3, 5) if w <= cap]
    ccls[(ccls == C_TIE) & (not tie_w)] = C_RAND
    t = ccls == C_TIE
    if tie_w:
        weight[t] = np.array(tie_w)[rng.integers(len(tie_w), size=int(t.sum()))]
        for w in tie_w:
            for ch in range(3):
                o, q = tie_bytes(cA[0, 0, ch], w)
                near = o[(np.abs(q) < 5) | (np.abs(q - 254.5) < 5)]
                sel = np.nonzero(t & (weight == w))[0]
                pick = np.where(rng.random(len(sel)) < 0.6, near[rng.integers(len(near), size=len(sel))], o[rng.integers(len(o), size=len(sel))])
                colour[sel, ch] = pick
    sp = ccls == C_SPECIAL
    colour[sp] = np.array([0, 1, 127, 128, 254])[rng.integers(5, size=(int(sp.sum()), 3))]
    # cancelling voxels: the weight follows the sdf class (ties keep theirs: their sdf is random)
    can_w = [w for w in [2] + LARGE_CANCEL if w <= cap] or [cap]
    can = ((scls == S_CANCEL_DE) | (scls == S_CANCEL_IN)) & ~t
    scls[((scls == S_CANCEL_DE) | (scls == S_CANCEL_IN)) & t] = S_RAND
    cw = np.array(can_w)[rng.integers(len(can_w), size=m)]
    cw[rng.random(m) < 0.5] = can_w[0]
    weight[can] = cw[can]
    found = np.zeros(m, bool)
    for w in can_w:
        for cls, sign in ((S_CANCEL_DE, 1.0), (S_CANCEL_IN, -1.0)):
            sel = np.nonzero(can & (scls == cls) & (weight == w))[0]
            x, ok = _cancelling((np.float32(sign) * sA[sel]).astype(np.float32), w)
            sdf[sel] = x; found[sel] = ok
    for cls, v in ((S_PZERO, 0.0), (S_NZERO, -0.0), (S_PDEN, 1e-40), (S_NDEN, -1e-40), (S_PTINY, 1e-20), (S_NTINY, -1e-20)):
        sdf[scls == cls] = np.float32(v)
    rec = np.zeros(m, VOXEL_DTYPE)
    rec["sdf"], rec["weight"] = sdf, weight.astype(np.float32)
    rec["color"][:, :3] = colour.astype(np.uint8); rec["color"][:, 3] = 255
    keys_sorted = sorted(hash_map(vol.osc))
    emptied_keys = set(keys_sorted[::4]) if emptied else set()
    if emptied:
        in_emptied = np.array([tuple(k) in emptied_keys for k in key[::VOX_PER_BLOCK]]).repeat(VOX_PER_BLOCK)
        weight[in_emptied] = np.where(upd[in_emptied], 1, 0)
        rec["weight"] = weight.astype(np.float32)
        scls[in_emptied] = S_RAND; ccls[in_emptied] = C_RAND
    zero = weight == 0
    rec[zero] = np.zeros(1, VOXEL_DTYPE)[0]
    vol.write({tuple(int(v) for v in key[b * VOX_PER_BLOCK]): rec[b * VOX_PER_BLOCK:(b + 1) * VOX_PER_BLOCK] for b in range(m // VOX_PER_BLOCK)})
    n = len(vol.osc.voxels())
    info = dict(weight=np.full(n, -1, np.int64), sdf_class=np.full(n, -1, np.int64), colour_class=np.full(n, -1, np.int64), numerator=np.full(n, np.nan, np.float32),
                cancel_found=np.zeros(n, bool), local_z=np.full(n, -1, np.int64), updated_by_A=np.zeros(n, bool), emptied_keys=emptied_keys)
    info["weight"][idx] = weight
    info["sdf_class"][idx] = np.where(zero, -1, scls)
    info["colour_class"][idx] = np.where(zero, -1, ccls)
    info["numerator"][idx] = (rec["sdf"] * rec["weight"]).astype(np.float32) - sA
    info["cancel_found"][idx] = found & ~zero
    info["sample_A"] = np.zeros(n, np.float32); info["sample_A"][idx] = sA
    info["local_z"][idx] = coord[:, 2] & 7
    info["updated_by_A"][idx] = upd
    return info


# ------------------------------------------------------------------------------------------------ the organic script
ORGANIC_INTEGRATIONS = 300


def organic_ops(kind):
    """300 operators cycling the frames A, B, C at the identity"""
    return [(kind, "ABC"[i % 3], IDENT, None) for i in range(ORGANIC_INTEGRATIONS)]


def organic_ref(vol):
    """the 300 integrations on the oracle and in float64.  The table is complete after the first three operators, so the three samples are taken once.
    -> State"""
    st = ref.State(vol.osc.voxels())
    ops = organic_ops("in")
    vol.run_oracle(ops[:3], st)
    h = vol.osc.hash().copy()
    smp = {}
    for f in "ABC":
        d, c = vol.frames[f]
        idx, ok, sdf, (py, px) = ref.sample(h, IDENT, d, True, vol.cam, vol.p)
        smp[f] = (idx, ok, sdf, c[py, px, :3].astype(np.float64))
    for kind, f, T0, _ in ops[3:]:
        vol.osc.integrate(T0, vol.frames[f][0], vol.frames[f][1], vol.cam)
        idx, ok, sdf, col = smp[f]
        ref.apply("in", st, idx, ok, sdf, col, vol.p.m_integrationWeightMax)
    assert np.array_equal(vol.osc.hash().view(np.uint8), h.view(np.uint8)), "the organic script allocated after its third operator"
    return st


def is_empty(hash_np, heap, heap_counter, vox, p):
    """nothing allocated, the heap complete, no voxel byte set"""
    return (bool((hash_np["ptr"] == FREE_ENTRY).all()) and heap_counter == p.m_numSDFBlocks - 1 and
            np.array_equal(np.sort(heap), np.arange(p.m_numSDFBlocks, dtype=heap.dtype)) and not vox.view(np.uint8).any())


# ------------------------------------------------------------------------------------------------ stated facts
# lower bounds that the CPU file asserts on what it measures (the measured figures are printed there)
FACTS = dict(
    per_weight_class={"default": 300, "cap1": 300, "cap2": 300, "cap4": 300, "cap255": 300, "fine": 300, "coarse": 100, "narrow": 300},      # updated voxels per planted weight and operator
    per_sdf_class=100, per_colour_class=1000,
    numerator_zero=50, numerator_tiny=50,                 # de-integration numerators that are 0 / non-zero and below 2^-60, among the voxels ("de", A) updates
    ties_negative=20, ties_low=100, ties_below_254=20, ties_from_254=20,      # colour channels of updated voxels with a half-integer quotient < 0 / in (0, 5) / in (249.5, 254.5) / >= 254.5
    cap_binds=300,                                        # voxels at the cap that ("in", A) changes in sdf and leaves at the cap
    emptied_blocks=15,
    edge_slice=1000,                                      # voxels of the slice the edge depth was found for
    bound_margin_px=1e-3,
)
