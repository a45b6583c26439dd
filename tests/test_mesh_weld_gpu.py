"""GPU tests (-m gpu) of the device weld (csrc/meshweld.hip) and of the mesh entry points built on it, against the numpy restatement tests/mesh_weld_ref.py and
against the host route (bf_marching_cubes_extract + bf_marching_cubes_save_mesh).  Bar: positions and colours compared as uint32, faces exactly, PLY files byte
for byte - tolerance 0.

Sizes: the kernels work in 256-thread workgroups on 3T corners and on T triangles, count and compact in tiles of 1024 elements, and scan the tile counts 256 at a
time; 86 / 257 are just above a workgroup (258 corners; 257 triangles), 342 / 1025 just above a tile (1026 corners; 1025 triangles), 87382 just above one step of
the tile-count scan (257 tiles of corners).  1365 triangles are 4095 corners in a table of 8192 slots: the densest load allowed."""
import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import camera_params, default_app_state, default_bundling_state, default_hash_params, intrinsics_matrix, sensor_desc
from tests import mesh_weld_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 64, 65, 86, 257, 342, 1025, 1365, 4097]
TRANSFORMS = [None, ref.TRANSFORM]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    return all(g.shape == w.shape and np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def welder(gpu):
    return gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)


def _weld(welder, tris, transform):
    import torch
    return welder.weld(torch.from_numpy(np.ascontiguousarray(tris, np.float32)).cuda(), transform)


@pytest.mark.parametrize("transform", TRANSFORMS, ids=["plain", "transformed"])
@pytest.mark.parametrize("family", ["soup_one_cell", "soup_copies", "soup_pool", "soup_distinct", "soup_range", "soup_boundaries", "soup_mixed"])
def test_weld_planted_soups(welder, family, transform):
    """1. families (a) - (f) and the mixed soup of the CPU test, every size, against the restatement"""
    for T in SIZES:
        tris = getattr(ref, family)(T, seed=T)
        want = ref.weld(tris, transform)
        got = _weld(welder, tris, transform)
        assert _same(got, want), (family, T, [len(x) for x in got], [len(x) for x in want])
        if T and family == "soup_one_cell":
            assert len(got[0]) == 1 and len(got[2]) == 0
        if T and family == "soup_copies":
            assert len(got[0]) == 3 and got[2].tolist() == [[0, 1, 2]]
        if family == "soup_distinct":
            assert len(got[0]) == 3 * T and len(got[2]) == T


def test_weld_contended_merges_keep_the_lowest_corner(welder):
    """(c) 4097 triangles over a pool of 60 cells: every key is wanted by some 200 corners from all over the corner range, each with its own position inside the
    cell and its own colour - "first to arrive" in place of "lowest index" shows in the vertex arrays"""
    tris = ref.soup_pool(4097, seed=11, cells=60)
    want = ref.weld(tris)
    assert len(want[0]) == 60
    corners = tris.reshape(-1, 6)
    assert len(np.unique(corners[:, 3:], axis=0)) == len(corners)
    assert _same(_weld(welder, tris, None), want)
    assert _same(_weld(welder, tris, ref.TRANSFORM), ref.weld(tris, ref.TRANSFORM))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_weld_all_keys_distinct_at_the_densest_load(welder, seed):
    """(d) 1365 triangles, three seeds"""
    tris = ref.soup_distinct(1365, seed=seed)
    got = _weld(welder, tris, None)
    assert len(got[0]) == 4095 and len(got[2]) == 1365 and _same(got, ref.weld(tris))


def test_weld_past_one_step_of_the_tile_scan_and_repeatability(welder):
    """87382 triangles are 257 tiles of corners; 3. a second weld of the same input gives the same arrays; a smaller weld afterwards is not disturbed by the larger
    one's buffers"""
    tris = ref.soup_mixed(87382, seed=7)
    want = ref.weld(tris, ref.TRANSFORM)
    a = _weld(welder, tris, ref.TRANSFORM)
    b = _weld(welder, tris, ref.TRANSFORM)
    assert _same(a, want) and _same(b, a)
    small = ref.soup_mixed(65, seed=8)
    assert _same(_weld(welder, small, None), ref.weld(small))


def test_weld_of_nothing_and_ply_of_nothing(gpu, tmp_path):
    mc = gpu.capi.MarchingCubesHashSDF(10, 1000, 0.02)
    pos, col, faces = mc.weld()                       # no extraction yet: the last extraction has zero triangles
    assert pos.shape == (0, 3) and col.shape == (0, 3) and faces.shape == (0, 3)
    assert mc.save_mesh_gpu(tmp_path / "empty.ply") == (0, 0)
    e3 = np.zeros((0, 3), np.float32)
    assert (tmp_path / "empty.ply").read_bytes() == ref.ply_bytes(e3, e3, np.zeros((0, 3), np.uint32))


# --------------------------------------------------------------------------- behind the extraction
def _volume(gpu):
    import torch
    W, H = 160, 120
    frames = [synth.scene_room(k, W, H) for k in (0, 20, 40)]
    K = frames[0][3]
    cam = camera_params(W, H, K["fx"], K["fy"], K["mx"], K["my"])
    p = default_hash_params(num_buckets=20011, num_sdf_blocks=20000, voxel_size=0.02)
    gs = gpu.capi.SceneRepHashSDF(p)
    for d, c, T, _ in frames:
        gs.integrate(T, torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda(), cam)
    return gs, p


def test_extract_gpu_and_save_mesh_gpu_on_a_volume(gpu, tmp_path):
    """2. the volume of test_marching_cubes_bit_exact_and_ordered (160 x 120, 2 cm, three frames)"""
    gs, p = _volume(gpu)
    mc = gpu.capi.MarchingCubesHashSDF(600000, p.m_hashNumBuckets, 0.02)
    tris, found = mc.extract(gs)
    assert found == len(tris) > 5000
    pts = tris[:, :, :3].reshape(-1, 3)
    box = ([float(v) for v in np.percentile(pts, 30, axis=0)], [float(v) for v in np.percentile(pts, 70, axis=0)])
    for name, transform, bx in (("plain", None, None), ("transformed", ref.TRANSFORM, None), ("box", None, box)):
        host_tris, host_found = mc.extract(gs, box=bx)
        nv, nf = mc.save_mesh(tmp_path / ("host_%s.ply" % name), transform)          # (clears the host mesh buffer)
        cnt = gpu.capi.C.c_uint32()
        gpu.capi.check(gpu.capi.lib.bf_marching_cubes_get_mesh(mc._h, None, 0, gpu.capi.C.byref(cnt)))
        assert cnt.value == 0
        n, f = mc.extract_gpu(gs, box=bx)
        assert (n, f) == (len(host_tris), host_found)
        assert np.array_equal(_bits(mc.download_triangles()), _bits(host_tris))              # the same triangle bytes as extract
        gpu.capi.check(gpu.capi.lib.bf_marching_cubes_get_mesh(mc._h, None, 0, gpu.capi.C.byref(cnt)))
        assert cnt.value == 0                                                                  # the host mesh buffer's count is left alone
        assert mc.save_mesh_gpu(tmp_path / ("gpu_%s.ply" % name), transform) == (nv, nf)
        raw = (tmp_path / ("gpu_%s.ply" % name)).read_bytes()
        assert raw == (tmp_path / ("host_%s.ply" % name)).read_bytes()
        assert raw == ref.ply_bytes(*ref.weld(host_tris, transform))
        if bx is None:
            assert 0.9 * found < nf <= found and 0.3 * nf < nv < nf
        else:
            assert 0 < host_found < found
        # weld() of the last extraction hands out the same arrays
        assert _same(mc.weld(None, transform), ref.weld(host_tris, transform))
    # extract_gpu does not append to a host mesh buffer that holds something
    mc.extract(gs)
    mc.extract_gpu(gs, box=box)
    cnt = gpu.capi.C.c_uint32()
    gpu.capi.check(gpu.capi.lib.bf_marching_cubes_get_mesh(mc._h, None, 0, gpu.capi.C.byref(cnt)))
    assert cnt.value == found
    # a capacity of 1000: the weld covers the clamped 1000 triangles, as the host does
    small = gpu.capi.MarchingCubesHashSDF(1000, p.m_hashNumBuckets, 0.02)
    ts, fs = small.extract(gs)
    assert fs == found and len(ts) == 1000
    small.save_mesh(tmp_path / "host_small.ply")
    assert small.extract_gpu(gs) == (1000, found)
    small.save_mesh_gpu(tmp_path / "gpu_small.ply")
    assert (tmp_path / "gpu_small.ply").read_bytes() == (tmp_path / "host_small.ply").read_bytes() == ref.ply_bytes(*ref.weld(tris[:1000]))
    # no capacity: the buffer is sized to the volume
    grow = gpu.capi.MarchingCubesHashSDF(0, p.m_hashNumBuckets, 0.02)
    assert grow.extract_gpu(gs, box=box)[0] < found
    assert grow.extract_gpu(gs) == (found, found)
    assert np.array_equal(_bits(grow.download_triangles()), _bits(tris))
    grow.save_mesh_gpu(tmp_path / "gpu_grow.ply")
    assert (tmp_path / "gpu_grow.ply").read_bytes() == (tmp_path / "host_plain.ply").read_bytes()


# --------------------------------------------------------------------------- the frame loop
PW, PH = 640, 480
_frames = {}


def _stream(n):
    if n not in _frames:
        _frames[n] = synth.render_frames(range(n))
    return _frames[n]


def _run_pipeline(gpu, n, mesh_dir, gc=True, timings=False):
    """the 25-frame configuration of tests/test_render_gpu.py::_run_pipeline; mesh_dir: save the mesh after frame 12 and after the last frame"""
    import torch
    frames = _stream(n)
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = PW, PH
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.02, 50000, 20000
    gas.s_garbageCollectionEnabled = 1 if gc else 0
    gbs.s_maxNumImages = 8
    gp = gpu.capi.Pipeline(gas, gbs, sensor_desc(PW, PH, K))
    if timings:
        gp.enable_timings(True)
    counts = []
    for k, (d, c, T, _) in enumerate(frames):
        assert gp.process_frame(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda())
        if mesh_dir is not None and k == 12:
            counts.append(gp.save_mesh(mesh_dir / "mid.ply"))
    if mesh_dir is not None:
        counts.append(gp.save_mesh(mesh_dir / "final.ply"))
    gp.synchronize()
    return gp, gas, counts


def _volume_state(gp):
    sc = gp.scene()
    return dict(traj=gp.integrated_trajectory().copy(), opt=gp.optimized_trajectory().copy(), dbg=sc.debug_hash(), heap_free=sc.heap_free_count(),
                blocks=sc.num_allocated_blocks(), counters=gp.counters())


@pytest.mark.parametrize("gc,timings", [(True, False), (False, False), (True, True)], ids=["default", "no_collection", "timings"])
def test_pipeline_save_mesh_leaves_the_reconstruction_alone(gpu, tmp_path, gc, timings):
    """4. one run saves the mesh after frame 12 and after the last frame, the other never: the same trajectories, bf_scene_debug_hash, heap free count, allocated
    blocks and counters; the final file is the one synchronize -> scene() -> stand-alone extract + host save_mesh write"""
    n = 25
    plain, _, _ = _run_pipeline(gpu, n, None, gc=gc, timings=timings)
    a = _volume_state(plain)
    plain.close()
    gp, gas, counts = _run_pipeline(gpu, n, tmp_path, gc=gc, timings=timings)
    b = _volume_state(gp)
    assert np.array_equal(_bits(a["traj"]), _bits(b["traj"])) and np.array_equal(_bits(a["opt"]), _bits(b["opt"]))
    assert a["dbg"] == b["dbg"] and a["heap_free"] == b["heap_free"] and a["blocks"] == b["blocks"] and a["counters"] == b["counters"]
    mc = gpu.capi.MarchingCubesHashSDF.from_global_app_state(gas, max_triangles=3000000)
    tris, found = mc.extract(gp.scene())
    nv, nf = mc.save_mesh(tmp_path / "alone.ply")
    assert found == len(tris) > 5000
    assert counts[1] == (nv, nf, found)
    assert (tmp_path / "final.ply").read_bytes() == (tmp_path / "alone.ply").read_bytes()
    assert counts[0][2] > 0 and (tmp_path / "mid.ply").read_bytes() != (tmp_path / "final.ply").read_bytes()
    # asking again changes nothing, and a transform reaches the vertices
    assert gp.save_mesh(tmp_path / "again.ply") == counts[1] and (tmp_path / "again.ply").read_bytes() == (tmp_path / "final.ply").read_bytes()
    gp.save_mesh(tmp_path / "moved.ply", ref.TRANSFORM)
    assert (tmp_path / "moved.ply").read_bytes() == ref.ply_bytes(*ref.weld(tris, ref.TRANSFORM))
    c = _volume_state(gp)
    assert c["dbg"] == b["dbg"] and c["heap_free"] == b["heap_free"] and c["blocks"] == b["blocks"]


def test_pipeline_save_mesh_refuses_a_sharded_volume(gpu, tmp_path):
    frames = _stream(25)
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = PW, PH
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.02, 50000, 20000
    gbs.s_maxNumImages = 8
    gp = gpu.capi.Pipeline(gas, gbs, sensor_desc(PW, PH, K))
    gp.set_volume_shard(0, 2)
    with pytest.raises(Exception, match="shard"):
        gp.save_mesh(tmp_path / "shard.ply")
    assert not (tmp_path / "shard.ply").exists()
    gp.close()
