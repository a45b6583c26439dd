"""GPU parity tests (-m gpu): the HIP marching cubes (csrc/mesh.hip) and ray cast (csrc/raycast.hip) on the planted volumes of tests/volume_cases.py
against the CPU oracle, bit for bit (tol 0).  tests/test_volume_consumers_edge_cpu.py pins the oracle to the reference's own kernels on these very volumes
and shows that they hold the cases they are named after.

Every volume is planted in the oracle and, byte for byte, on the device; assert_same_state runs after planting and before any consumer."""
import ctypes as C

import numpy as np
import pytest

from bundlefusion_amd.capi import default_hash_params, BFError
from tests import volume_cases as vc
from tests.test_tsdf_gpu import assert_same_state

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (67, 9), (65, 41), (160, 120)]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _marching_cubes(gpu, max_triangles, buckets, thresholds):
    """MarchingCubesHashSDF with m_threshMarchingCubes != m_threshMarchingCubes2 (the class derives both from one factor): a subclass that creates
    the handle from its own parameters and inherits everything else"""
    capi = gpu.capi

    class TwoThresholds(capi.MarchingCubesHashSDF):
        def __init__(self):
            self.params = capi.MarchingCubesParams(max_triangles, capi.SDF_BLOCK_SIZE, buckets, capi.HASH_BUCKET_SIZE, thresholds[0], thresholds[1])
            self._h = C.c_void_p()
            capi.check(capi.lib.bf_marching_cubes_create(C.byref(self.params), C.byref(self._h)))
    return TwoThresholds()


class _Volumes:
    """the planted volumes the tests of this module share; built on first use, never written after planting (a test that needs another frustum list
    compactifies for its pose before it renders: every render here does)"""

    def __init__(self, gpu, oracle):
        self.gpu, self.oracle, self.made = gpu, oracle, {}

    def mc(self, name):
        if ("mc", name) not in self.made:
            vol, _ = vc.build(self.oracle, {"roomy": vc.ROOMY, "tight": vc.TIGHT}[name], gpu=self.gpu)
            vol.write(vc.plant_mc(vol.osc)[0])
            assert_same_state(vol.gs, vol.osc, "planted %s volume:" % name)
            self.made[("mc", name)] = vol
        return self.made[("mc", name)]

    def rc(self, name):
        """(e) `holes`: 20 mm, seen from the pose of frame 20; (f) `near`: 50 mm, seen from the near-camera pose - both with the holes planted"""
        if ("rc", name) not in self.made:
            vol, frames = vc.build(self.oracle, vc.ROOMY, voxel=vc.VOXEL if name == "holes" else vc.NEAR_VOXEL, gpu=self.gpu)
            T = frames[1][2].astype(np.float32) if name == "holes" else vc.near_camera_pose(frames)
            vol.compactify(T)
            vol.write(vc.plant_holes(vol.osc))
            assert_same_state(vol.gs, vol.osc, "planted %s volume:" % name)
            self.made[("rc", name)] = (vol, frames, T)
        return self.made[("rc", name)]


@pytest.fixture(scope="module")
def volumes(gpu, oracle):
    v = _Volumes(gpu, oracle)
    yield v
    v.made.clear()


# ------------------------------------------------------------------------------------------------ marching cubes
@pytest.mark.parametrize("thresholds", [vc.DEFAULT_THRESHOLDS, vc.GATE_THRESHOLDS], ids=["default", "gates"])
@pytest.mark.parametrize("name", ["roomy", "tight"])
def test_marching_cubes_on_planted_volumes(gpu, oracle, volumes, name, thresholds):
    """families (a)-(d): the whole volume and the box on cell positions (inclusive bounds, and one float32 step inside them), in the product's order
    (hash slot, voxel index, table order); a second extraction returns the same bytes"""
    vol = volumes.mc(name)
    e, t = gpu.capi.marching_cubes_tables()
    mc = _marching_cubes(gpu, 100000, vol.p.m_hashNumBuckets, thresholds)
    tris, found = mc.extract(vol.gs)
    otris, on = oracle.mc_extract(vol.osc, thresholds[0], thresholds[1], e, t, 100000)
    assert found == on == len(tris) > 10000
    assert _same(tris, otris)
    again, found2 = mc.extract(vol.gs)
    assert found2 == found and _same(again, tris)
    box, _ = vc.box_on_cells(vc.mc_predict(vol.osc.hash(), vol.osc.voxels(), vc.VOXEL, thresholds[0], thresholds[1], e, t), vc.VOXEL)
    counts = []
    for bx in (box, vc.shrink_box(box)):
        tb, fb = mc.extract(vol.gs, box=bx)
        ob, onb = oracle.mc_extract(vol.osc, thresholds[0], thresholds[1], e, t, 100000, box=bx)
        assert 0 < fb == onb < found and _same(tb, ob)
        counts.append(fb)
    assert counts[1] < counts[0]


def test_marching_cubes_capacities_on_a_planted_volume(gpu, oracle, volumes):
    """a buffer of 1 triangle, of exactly the number found and of one fewer: the count found is reported, the buffer holds the first of them"""
    vol = volumes.mc("roomy")
    e, t = gpu.capi.marching_cubes_tables()
    th = vc.DEFAULT_THRESHOLDS
    otris, on = oracle.mc_extract(vol.osc, th[0], th[1], e, t, 100000)
    for cap in (1, on, on - 1):
        mc = _marching_cubes(gpu, cap, vol.p.m_hashNumBuckets, th)
        tris, found = mc.extract(vol.gs)
        assert found == on and len(tris) == cap and _same(tris, otris[:cap]), cap


@pytest.mark.parametrize("blocks", [1, 1024, 1025])
def test_marching_cubes_block_counts_at_the_scan_chunk(gpu, oracle, blocks):
    """exactly 1, 1024 and 1025 occupied blocks (a heap of that many blocks, exhausted): one chunk of k_scan_u32 less one, full, and one more.  Allocated at
    10 mm voxels, not at the 20 mm of the other volumes: at 20 mm the three frames ask for 351 blocks only, too few to exhaust a heap of 1025."""
    frames, cam = vc.room_frames()
    p = default_hash_params(voxel_size=0.01, num_buckets=20011, num_sdf_blocks=blocks)
    vol = vc.Planted(oracle, p, frames, cam, gpu=gpu)
    assert vol.osc.num_allocated() == blocks
    if blocks > 1:
        vol.write(vc.plant_mc(vol.osc, families=("cases",))[0])
    else:
        vol.write({key: vc.full_block(0) for key in vc.hash_map(vol.osc)})          # (alone, the block's natural cells all read absent neighbours)
    assert_same_state(vol.gs, vol.osc, "%d blocks:" % blocks)
    e, t = gpu.capi.marching_cubes_tables()
    mc = gpu.capi.MarchingCubesHashSDF(300000, p.m_hashNumBuckets, 0.01)
    tris, found = mc.extract(vol.gs)
    otris, on = oracle.mc_extract(vol.osc, 0.1, 0.1, e, t, 300000)
    assert found == on == len(tris) and on > (20 if blocks == 1 else 3000)
    assert _same(tris, otris)


def test_marching_cubes_with_more_than_1024_slot_tiles(gpu, oracle):
    """300007 buckets = 1172 tiles of 1024 hash slots: the scan of the tile counts crosses its chunk of 1024, with blocks in tiles on both sides"""
    vol, _ = vc.build(oracle, dict(num_buckets=300007, num_sdf_blocks=4000), gpu=gpu)
    vol.write(vc.plant_mc(vol.osc)[0])
    assert_same_state(vol.gs, vol.osc, "300007 buckets:")
    slots = np.nonzero(vol.osc.hash()["ptr"] != -2)[0]
    assert (slots // 1024 < 1024).sum() >= 100 and (slots // 1024 >= 1024).sum() >= 10
    e, t = gpu.capi.marching_cubes_tables()
    mc = gpu.capi.MarchingCubesHashSDF(100000, vol.p.m_hashNumBuckets, vc.VOXEL)
    tris, found = mc.extract(vol.gs)
    otris, on = oracle.mc_extract(vol.osc, vc.DEFAULT_THRESHOLDS[0], vc.DEFAULT_THRESHOLDS[1], e, t, 100000)
    assert found == on == len(tris) > 10000 and _same(tris, otris)


def test_marching_cubes_of_an_empty_volume(gpu):
    p = default_hash_params(voxel_size=vc.VOXEL, **vc.ROOMY)
    gs = gpu.capi.SceneRepHashSDF(p)
    mc = gpu.capi.MarchingCubesHashSDF(1000, p.m_hashNumBuckets, vc.VOXEL)
    for box in (None, ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])):
        tris, found = mc.extract(gs, box=box)
        assert found == 0 and len(tris) == 0


# ------------------------------------------------------------------------------------------------ ray cast
def _compare(oracle, rc, vol):
    """the existing bar of tests/test_raycast_gpu.py::_check on a ray cast that has rendered: intervals and all four images, tol 0"""
    g = rc.download()
    rp = rc.params()
    omin, omax = oracle.rc_splat(vol.osc, vol.cam, rp)
    assert _same(g["ray_min"], omin) and _same(g["ray_max"], omax)
    o = oracle.rc_render(vol.osc, rp, omin, omax)
    for k in ("depth", "depth4", "colors", "normals"):
        assert _same(g[k], o[k]), k
    return g


def _render(gpu, oracle, vol, rp, T):
    """compactify for T in the oracle and on the device, render from T (the contract of the C ABI), compare"""
    vol.compactify(T)
    rc = gpu.capi.RayCastSDF(rp)
    rc.render(vol.gs, vol.cam, T)
    assert rc.params().m_numOccupiedSDFBlocks == vol.osc.num_occupied() > 0
    return rc, _compare(oracle, rc, vol)


@pytest.mark.parametrize("grad", [0, 1])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["holes", "near"])
def test_ray_cast_on_planted_volumes(gpu, oracle, volumes, name, size, grad):
    """every size has hits (the CPU file counts them): the single ray of the 1x1 image is turned towards the surface (vc.pose_for_size)"""
    vol, frames, T = volumes.rc(name)
    rc, g = _render(gpu, oracle, vol, vc.ray_params(frames[0][3], size[0], size[1], use_gradients=grad), vc.pose_for_size(T, size))
    hits = g["depth"] != -np.inf
    assert hits.sum() > (3000 if size == (160, 120) else 0)
    if grad:
        assert (g["normals"][hits][:, 0] != -np.inf).any()


@pytest.mark.parametrize("grad", [0, 1])
@pytest.mark.parametrize("variant", [vc.TIGHT_GATES, dict(increment=vc.SECOND_INCREMENT)], ids=["gates", "increment"])
def test_ray_cast_gates_and_a_second_increment(gpu, oracle, volumes, variant, grad):
    """m_thresSampleDist / m_thresDist tightened until each removes about half of the hits (counted in the CPU file), and another m_rayIncrement"""
    vol, frames, T = volumes.rc("holes")
    plain = _render(gpu, oracle, vol, vc.ray_params(frames[0][3], 160, 120, use_gradients=grad), T)[1]
    g = _render(gpu, oracle, vol, vc.ray_params(frames[0][3], 160, 120, use_gradients=grad, **variant), T)[1]
    n, m = (plain["depth"] != -np.inf).sum(), (g["depth"] != -np.inf).sum()
    assert not _same(plain["depth"], g["depth"]) and (variant is not vc.TIGHT_GATES or 0.1 * n <= m <= 0.9 * n)


def test_ray_cast_min_max_intrinsics_and_capacity(gpu, oracle, volumes):
    vol, frames, T = volumes.rc("holes")
    K = frames[0][3]
    rc, full = _render(gpu, oracle, vol, vc.ray_params(K, 160, 120), T)
    # update_min_max (the top-down render's path): bounds that cut through the visible surface
    d = full["depth"][full["depth"] != -np.inf]
    lo, hi = float(np.quantile(d, 0.3)), float(np.quantile(d, 0.7))
    rc.update_min_max(lo, hi)
    assert (rc.params().m_minDepth, rc.params().m_maxDepth) == (np.float32(lo), np.float32(hi))
    rc.render(vol.gs, vol.cam, T)
    cut = _compare(oracle, rc, vol)
    assert 0.1 * len(d) < (cut["depth"] != -np.inf).sum() < 0.9 * len(d)
    # set_intrinsics: a smaller image inside the buffers created
    small = vc.ray_params(K, 67, 9)
    Km = np.eye(4, dtype=np.float32)
    Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2] = small.fx, small.fy, small.mx, small.my
    rc.set_intrinsics(67, 9, Km)
    p = rc.params()
    assert (p.m_width, p.m_height, p.fx, p.fy, p.mx, p.my) == (67, 9, small.fx, small.fy, small.mx, small.my)
    rc.render(vol.gs, vol.cam, T)
    g = _compare(oracle, rc, vol)
    assert g["depth"].shape == (9, 67) and (g["depth"] != -np.inf).any()
    with pytest.raises(BFError):
        rc.set_intrinsics(161, 120, Km)
    # m_maxNumVertices <= 6 * numOccupied: BF_ERR_CAPACITY, and the images and the view of the previous render stay
    n = vol.osc.num_occupied()
    closer = T.copy(); closer[:3, 3] += np.float32(0.5) * T[:3, 2]
    rc3, before = _render(gpu, oracle, vol, vc.ray_params(K, 65, 41, max_vertices=6 * n), closer)
    n2 = vol.osc.num_occupied()
    assert 0 < n2 < n
    vol.compactify(T)
    with pytest.raises(BFError):
        rc3.render(vol.gs, vol.cam, T)
    after = rc3.download()
    assert all(_same(before[k], after[k]) for k in before) and rc3.params().m_numOccupiedSDFBlocks == n2
    assert np.array_equal(np.array(list(rc3.params().m_viewMatrixInverse), np.float32).reshape(4, 4), closer)
    _render(gpu, oracle, vol, vc.ray_params(K, 65, 41, max_vertices=6 * n + 1), T)


def test_ray_cast_with_an_empty_frustum_list(gpu, oracle, volumes):
    """a pose that sees no block: nothing is splatted, every image is -inf, and the view of the last render that saw blocks stays in the parameters"""
    vol, frames, T = volumes.rc("holes")
    rc, g = _render(gpu, oracle, vol, vc.ray_params(frames[0][3], 65, 41), T)
    away = T.copy(); away[:3, 3] += np.float32(50.0)
    vol.compactify(away)
    assert vol.osc.num_occupied() == 0 and vol.gs.hash_params().m_numOccupiedBlocks == 0
    rc.render(vol.gs, vol.cam, away)
    e = rc.download()
    assert all((e[k] == -np.inf).all() for k in e)
    assert np.array_equal(np.array(list(rc.params().m_viewMatrixInverse), np.float32).reshape(4, 4), T)


# ------------------------------------------------------------------------------------------------ the splat
def test_interval_splat_from_32_poses(gpu, oracle, volumes):
    """33x17, compactified and rendered from the same pose (the contract of the C ABI), all 32 poses of vc.splat_poses, each with blocks in view: the
    near-camera pose of (f), views from inside the allocated region, views whose nearest block has corners behind the camera (10 of the 32, counted in
    the CPU file), poses along and off the stream"""
    vol, frames, T = volumes.rc("near")
    rc = gpu.capi.RayCastSDF(vc.ray_params(frames[0][3], 33, 17))
    poses = vc.splat_poses(vol.osc, frames, vc.NEAR_VOXEL)
    assert len(poses) == 32
    for i, P in enumerate(poses):
        vol.compactify(P)
        assert vol.gs.hash_params().m_numOccupiedBlocks == vol.osc.num_occupied() > 0, i
        rc.render(vol.gs, vol.cam, P)
        g = rc.download()
        omin, omax = oracle.rc_splat(vol.osc, vol.cam, rc.params())
        assert (omin != -np.inf).any(), i
        assert _same(g["ray_min"], omin) and _same(g["ray_max"], omax), i
