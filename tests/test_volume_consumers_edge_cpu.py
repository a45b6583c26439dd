"""CPU tests (-m "not gpu") of the planted volumes of tests/volume_cases.py, the inputs tests/test_volume_consumers_edge_gpu.py gives the HIP marching cubes
and ray cast:

  * the oracle is pinned to the reference's own kernels ON THESE VOLUMES (extractIsoSurface with its Tables.h: the same triangles as a multiset;
    renderKernel from the oracle's interval images: every image bit for bit) - skipped, like tests/test_ref_pin_cpu.py, only where the compiled
    reference is absent;
  * the volumes hold the cases they are named after: counted from the oracle and a float64 numpy recomputation alone, printed, asserted.
"""
import numpy as np
import pytest

from bundlefusion_amd.capi import marching_cubes_tables
from tests import ref_api, volume_cases as vc

needs_reference = pytest.mark.skipif(not ref_api.available(), reason="oracle/_ref/libbfref.so is absent and /root/reference is not here to build it")

HASHES = {"roomy": vc.ROOMY, "tight": vc.TIGHT}
SIZES = [(1, 1), (7, 5), (67, 9), (65, 41), (160, 120)]


def _multiset(a):
    return sorted(map(bytes, np.ascontiguousarray(a).reshape(len(a), -1)))


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ marching cubes
@needs_reference
@pytest.mark.parametrize("name", ["roomy", "chained"])
def test_marching_cubes_oracle_vs_reference_kernels_on_planted_volumes(oracle, name):
    """families (a)-(d), full volume and box, default thresholds and thresh != thresh2; in a roomy hash and in one with overflow chains"""
    vol, _ = vc.build(oracle, {"roomy": vc.ROOMY, "chained": vc.CHAINED}[name], ref_api=ref_api)
    assert set(vc.hash_map(vol.osc)) == set(vc.hash_map(vol.rsc)) and vol.osc.num_dropped() == 0
    assert name == "roomy" or (vol.osc.hash()["offset"] != 0).sum() >= 10
    blocks, _ = vc.plant_mc(vol.osc)
    vol.write(blocks)
    re_, rt = ref_api.mc_tables()
    for th in (vc.DEFAULT_THRESHOLDS, vc.GATE_THRESHOLDS):
        r, rn = ref_api.mc_extract(vol.rsc, th[0], th[1], 400000)
        o, on = oracle.mc_extract(vol.osc, th[0], th[1], re_, rt, 400000)
        assert rn == on > 10000 and _multiset(r) == _multiset(o), (name, th)
        box, _ = vc.box_on_cells(vc.mc_predict(vol.osc.hash(), vol.osc.voxels(), vc.VOXEL, th[0], th[1], re_, rt), vc.VOXEL)
        for bx in (box, vc.shrink_box(box)):
            r, rn = ref_api.mc_extract(vol.rsc, th[0], th[1], 400000, box=bx)
            o, on = oracle.mc_extract(vol.osc, th[0], th[1], re_, rt, 400000, box=bx)
            assert 0 < rn == on and _multiset(r) == _multiset(o), (name, th, bx)


@pytest.mark.parametrize("name", sorted(HASHES))
def test_planted_marching_cubes_volumes_hold_their_cases(oracle, name):
    e, t = marching_cubes_tables()
    th, gt = vc.DEFAULT_THRESHOLDS, vc.GATE_THRESHOLDS
    vol, _ = vc.build(oracle, HASHES[name])
    osc = vol.osc
    extract = lambda th_, box=None: oracle.mc_extract(osc, th_[0], th_[1], e, t, 400000, box=box)
    predict = lambda th_, box=None: vc.mc_predict(osc.hash(), osc.voxels(), vc.VOXEL, th_[0], th_[1], e, t, box=box)
    # the natural volume: the recomputation predicts the oracle's count exactly, and finds a handful of cases
    pr = predict(th)
    natural, n_nat = extract(th)
    assert int(pr["ntri"].sum()) == n_nat > 5000
    print("%s, natural volume: %d blocks (%d dropped, %d chained), %d valid cells, %d triangles, %d emitting cases" % (
        name, osc.num_allocated(), osc.num_dropped(), int((osc.hash()["offset"] != 0).sum()), pr["cells"], n_nat, len(set(pr["ci"][pr["ntri"] > 0].tolist()))))
    if name == "tight":
        assert osc.num_dropped() > 0 and (osc.hash()["offset"] != 0).sum() > 10
    # (a): every case index among the cells that pass the gates
    blocks, info = vc.plant_mc(osc)
    colours = np.concatenate([b["color"] for b in blocks.values()])
    assert len(set(map(bytes, colours))) == len(colours) and (colours[:, :3] == 0).any() and (colours[:, :3] == 255).any() and (colours[:, 3] != 0).all()
    vol.write(blocks)
    planted, n_pl = extract(th)
    pr = predict(th)
    passing = ~pr["gate1"] & ~pr["gate2"]
    print("%s, planted: %d triangles, float64 recomputation %d (difference %+d), %d case indices among the %d cells that pass the gates, %d emitting" % (
        name, n_pl, int(pr["ntri"].sum()), int(pr["ntri"].sum()) - n_pl, len(set(pr["ci"][passing].tolist())), int(passing.sum()), len(set(pr["ci"][pr["ntri"] > 0].tolist()))))
    assert set(pr["ci"][passing].tolist()) == set(range(256))
    assert set(pr["ci"][pr["ntri"] > 0].tolist()) == set(range(1, 255)) - {85, 170}             # (edge masks 0 and 255 emit nothing, as in the reference)
    where = {tuple(int(v) for v in p): i for i, p in enumerate(pr["pos"])}
    cell_of = lambda key, c: where.get((key[0] * 8 + c[0], key[1] * 8 + c[1], key[2] * 8 + c[2]))
    # (b): the planted cells change the mesh; under GATE_THRESHOLDS each gate alone drops some of them and some are kept
    vol_b, _ = vc.build(oracle, HASHES[name])
    vol_b.write(vc.plant_mc(vol_b.osc, families=("cases", "weights", "full"))[0])
    for th_ in (th, gt):
        a = extract(th_)[0]; b = oracle.mc_extract(vol_b.osc, th_[0], th_[1], e, t, 400000)[0]
        assert _multiset(a) != _multiset(b), "family (b) leaves the mesh as it is"
    pg = predict(gt)
    idx = [cell_of(k, c) for k, c, _ in info["interp"]]
    assert None not in idx
    g1 = sum(bool(pg["gate1"][i] and not pg["gate2"][i]) for i in idx); g2 = sum(bool(pg["gate2"][i] and not pg["gate1"][i]) for i in idx)
    kept = sum(bool(pg["ntri"][i] > 0) for i in idx)
    near = sum(bool((np.abs(pr["d"][i]) < 1e-5).any()) for i in idx); beyond = sum(bool(((np.abs(pr["d"][i]) > 1e-5) & (np.abs(pr["d"][i]) < 1e-4)).any()) for i in idx)
    print("%s, (b): of %d cells gate 1 alone drops %d, gate 2 alone %d, %d emit; %d have a corner within 1e-5 of 0, %d one just beyond; whole volume under %s: %d / %d / %d kept" % (
        name, len(idx), g1, g2, kept, near, beyond, gt, int((pg["gate1"] & ~pg["gate2"]).sum()), int((pg["gate2"] & ~pg["gate1"]).sum()), int((~pg["gate1"] & ~pg["gate2"]).sum())))
    assert g1 >= 2 and g2 >= 2 and kept >= 4 and near >= 8 and beyond >= 4
    # (c): a single weight of 0 empties each of the 27 cells; cells that read absent (tight: dropped) blocks
    vol_c, _ = vc.build(oracle, HASHES[name])
    vol_c.write(vc.plant_mc(vol_c.osc, weights_valid=True)[0])
    n_valid = oracle.mc_extract(vol_c.osc, th[0], th[1], e, t, 400000)[1]
    pc = vc.mc_predict(vol_c.osc.hash(), vol_c.osc.voxels(), vc.VOXEL, th[0], th[1], e, t)
    where_c = {tuple(int(v) for v in p): i for i, p in enumerate(pc["pos"])}
    per_cell = [int(pc["ntri"][where_c[(k[0] * 8 + c[0], k[1] * 8 + c[1], k[2] * 8 + c[2])]]) for k, c, _ in info["weights"]]
    assert len(per_cell) == 27 and min(per_cell) > 0 and all(cell_of(k, c) is None for k, c, _ in info["weights"])
    assert n_valid - n_pl >= sum(per_cell)
    absent = vc.absent_neighbour_cells(osc.hash(), osc.voxels())
    print("%s, (c): %d triangles with the 27 weights restored, %d without; cells emptied only by an absent block: %s (face / edge / corner)" % (name, n_valid, n_pl, absent))
    assert min(absent.values()) >= 20
    if name == "tight":
        roomy, _ = vc.build(oracle, vc.ROOMY)
        dropped = set(vc.hash_map(roomy.osc)) - set(vc.hash_map(osc))
        by_drop = vc.absent_neighbour_cells(osc.hash(), osc.voxels(), among=dropped)
        print("tight, (c): %d keys dropped by full buckets; cells emptied only by one of them: %s" % (len(dropped), by_drop))
        assert osc.num_dropped() >= len(dropped) > 0 and min(by_drop.values()) >= 20
    em = pr["pos"][pr["ntri"] > 0]
    zero, neg = (em == 0).any(axis=1), (em < 0).any(axis=1)
    print("%s, (c): emitting cells with a voxel coordinate 0 (they read voxel -1 of block -1): %d; with a negative coordinate: %d" % (name, int(zero.sum()), int(neg.sum())))
    assert zero.sum() >= 20 and neg.sum() >= 1000
    # (d): both bounds of the box lie on emitting cells and are inclusive
    box, (lo, hi) = vc.box_on_cells(pr, vc.VOXEL)
    pb = predict(th, box=box)
    emb = pb["pos"][pb["ntri"] > 0]
    on_bound = [int((emb[:, k] == lo[k]).sum()) for k in range(3)] + [int((emb[:, k] == hi[k]).sum()) for k in range(3)]
    n_box, n_in = extract(th, box)[1], extract(th, vc.shrink_box(box))[1]
    print("%s, (d): box %s: %d triangles, %d with exclusive bounds; emitting cells exactly on the six bounds: %s" % (name, box, n_box, n_in, on_bound))
    assert min(on_bound) > 0 and 0 < n_in < n_box < n_pl


# ------------------------------------------------------------------------------------------------ ray cast
def _render(oracle, osc, cam, rp):
    rmin, rmax = oracle.rc_splat(osc, cam, rp)
    return oracle.rc_render(osc, rp, rmin, rmax), rmin, rmax


def _holes_volume(oracle, ref=None, fraction=0.02):
    vol, frames = vc.build(oracle, vc.ROOMY, ref_api=ref)
    T = frames[1][2].astype(np.float32)
    vol.compactify(T)
    vol.write(vc.plant_holes(vol.osc, fraction=fraction))
    return vol, frames, T


def _near_volume(oracle, ref=None):
    vol, frames = vc.build(oracle, vc.ROOMY, voxel=vc.NEAR_VOXEL, ref_api=ref)
    T = vc.near_camera_pose(frames)
    vol.compactify(T)
    vol.write(vc.plant_holes(vol.osc))
    return vol, frames, T


RAY_VARIANTS = [dict(), vc.TIGHT_GATES, dict(increment=vc.SECOND_INCREMENT)]


@needs_reference
def test_ray_cast_oracle_vs_reference_kernel_on_planted_volumes(oracle):
    """(e) at every image size with and without analytic gradients, under the tightened gates and a second increment; (f) from the near-camera pose"""
    hits = 0
    for make in (_holes_volume, _near_volume):
        vol, frames, T = make(oracle, ref_api)
        K = frames[0][3]
        assert vol.osc.num_occupied() == vol.rsc.num_occupied() > 0
        for (w, h) in SIZES:
            P = vc.pose_for_size(T, (w, h))
            vol.compactify(P)
            for grad in (0, 1):
                for kw in (RAY_VARIANTS if (w, h) == (160, 120) else RAY_VARIANTS[:1]):
                    rp = vc.with_view(oracle, vc.ray_params(K, w, h, use_gradients=grad, **kw), P)
                    o, rmin, rmax = _render(oracle, vol.osc, vol.cam, rp)
                    r = ref_api.rc_render(vol.rsc, rp, rmin, rmax)
                    for k in ("depth", "depth4", "colors") + (("normals",) if grad else ()):
                        assert _bits(o[k], r[k]), (make.__name__, w, h, grad, kw, k)
                    assert (o["depth"] != -np.inf).any(), (make.__name__, w, h)
                    hits += int((o["depth"] != -np.inf).sum())
    assert hits > 50000


def test_planted_ray_cast_volumes_hold_their_cases(oracle):
    natural, frames = vc.build(oracle, vc.ROOMY)
    K = frames[0][3]
    T = frames[1][2].astype(np.float32)
    natural.compactify(T)
    rp = vc.with_view(oracle, vc.ray_params(K, 160, 120), T)
    base = _render(oracle, natural.osc, natural.cam, rp)[0]
    vol, _, _ = _holes_volume(oracle)
    whole, _, _ = _holes_volume(oracle, fraction=0.0)                  # the same sdf and colours with every weight kept
    holes = _render(oracle, vol.osc, vol.cam, rp)[0]
    filled = _render(oracle, whole.osc, whole.cam, rp)[0]
    h0, h1, h2 = (x["depth"] != -np.inf for x in (base, holes, filled))
    lost = h0 & ~h1
    moved = h2 & (filled["depth"].view(np.uint32) != holes["depth"].view(np.uint32))
    same = h1 & (filled["depth"].view(np.uint32) == holes["depth"].view(np.uint32))
    partial = same & (filled["normals"].view(np.uint32) != holes["normals"].view(np.uint32)).any(axis=2)
    m, nv = vc.hash_map(natural.osc), natural.osc.voxels()
    zero_w = sum(int(((b["weight"] == 0) & (nv["weight"][m[k]:m[k] + 512] > 0)).sum()) for k, b in vc.plant_holes(natural.osc).items())
    print("(e): %d hits on the natural volume, %d planted (%d of the natural ones lost); against the same volume with every weight kept (%d hits): %d lose or move "
          "their hit, %d keep their depth bits but get another analytic-gradient normal; %d weights set to 0" % (h0.sum(), h1.sum(), lost.sum(), h2.sum(), moved.sum(), partial.sum(), zero_w))
    assert lost.sum() >= 0.01 * h0.sum() and moved.sum() >= 0.01 * h2.sum() and partial.sum() >= 20
    both = _render(oracle, vol.osc, vol.cam, vc.with_view(oracle, vc.ray_params(K, 160, 120, **vc.TIGHT_GATES), T))[0]
    only_s = _render(oracle, vol.osc, vol.cam, vc.with_view(oracle, vc.ray_params(K, 160, 120, thres_sample=vc.TIGHT_GATES["thres_sample"]), T))[0]
    only_d = _render(oracle, vol.osc, vol.cam, vc.with_view(oracle, vc.ray_params(K, 160, 120, thres_dist=vc.TIGHT_GATES["thres_dist"]), T))[0]
    n, nb, ns, nd = (int((x["depth"] != -np.inf).sum()) for x in (holes, both, only_s, only_d))
    print("(e) gates %s: of %d hits m_thresSampleDist alone keeps %d, m_thresDist alone %d, both %d" % (vc.TIGHT_GATES, n, ns, nd, nb))
    for kept in (ns, nd, nb):
        assert 0.1 * n <= kept <= 0.9 * n
    other = _render(oracle, vol.osc, vol.cam, vc.with_view(oracle, vc.ray_params(K, 160, 120, increment=vc.SECOND_INCREMENT), T))[0]
    assert not _bits(other["depth"], holes["depth"])
    # (f)
    near, frames5, Tn = _near_volume(oracle)
    rpn = vc.with_view(oracle, vc.ray_params(K, 160, 120), Tn)
    facts = vc.near_camera_facts(near.osc, near.cam, rpn, vc.NEAR_VOXEL)
    o, rmin, rmax = _render(oracle, near.osc, near.cam, rpn)
    print("(f): %s; %d pixels covered, %d hit" % ({k: int(v) for k, v in facts.items()}, int((rmin != -np.inf).sum()), int((o["depth"] != -np.inf).sum())))
    assert facts["straddle_z"] >= 1 and min(facts[k] for k in ("left", "right", "top", "bottom")) >= 1
    assert (o["depth"] != -np.inf).sum() > 1000
    # every image size has hits, with a normal from the analytic gradient (the single ray of 1x1 is turned until it hits: vc.pose_for_size)
    for name, (v, fr, Tv) in (("holes", (vol, frames, T)), ("near", (near, frames5, Tn))):
        per_size = []
        for size in SIZES:
            P = vc.pose_for_size(Tv, size)
            v.compactify(P)
            o = _render(oracle, v.osc, v.cam, vc.with_view(oracle, vc.ray_params(K, size[0], size[1], use_gradients=1), P))[0]
            hit = o["depth"] != -np.inf
            per_size.append(int(hit.sum()))
            assert hit.any() and (o["normals"][hit][:, 0] != -np.inf).any(), (name, size)
        print("%s: hits at %s: %s" % (name, SIZES, per_size))
    # the splat's poses: every one sees blocks and covers pixels; several have a block with corners on both sides of camera z = 0
    poses = vc.splat_poses(near.osc, frames5, vc.NEAR_VOXEL)
    blocks, straddling = [], []
    for P in poses:
        near.compactify(P)
        rps = vc.with_view(oracle, vc.ray_params(K, 33, 17), P)
        rmin, _ = oracle.rc_splat(near.osc, near.cam, rps)
        f = vc.near_camera_facts(near.osc, near.cam, rps, vc.NEAR_VOXEL)
        assert f["blocks"] == near.osc.num_occupied() > 0 and (rmin != -np.inf).any()
        blocks.append(f["blocks"]); straddling.append(int(f["straddle_z"]))
    print("splat: 32 poses with %d to %d blocks in view; %d poses have a block across camera z = 0 (%d such blocks)" % (
        min(blocks), max(blocks), sum(s > 0 for s in straddling), sum(straddling)))
    assert len(poses) == 32 and sum(s > 0 for s in straddling) >= 8            # (the near-camera pose and the eight poses placed just in front of a block's centre)
