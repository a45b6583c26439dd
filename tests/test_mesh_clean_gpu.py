"""GPU tests (-m gpu) of the device mesh cleaning (csrc/meshclean.hip) and of the entry points built on it, against the numpy restatement tests/mesh_clean_ref.py.
Bar: positions, colours and normals compared as uint32; faces, labels and stats exactly; PLY files byte for byte - tolerance 0.

Sizes: the kernels work in 64-lane waves and 256-thread workgroups, count and compact in tiles of 1024 elements and scan the tile counts 256 at a time; a vertex's
normal is summed by one thread up to 64 corners and by one wave beyond.  63 / 64 / 65 are either side of a wave (and of that switch, in the fan), 257 is just above a
workgroup, 1025 just above a tile, 4097 gives several tiles; 87382 islands are 257 tiles of vertices and 262 228 faces 257 tiles of faces: past one step of the
tile-count scan."""
import numpy as np
import pytest

from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix, sensor_desc
from tests import mesh_clean_ref as ref
from tests import mesh_weld_ref
from tests import test_mesh_weld_gpu as weld_gpu
from tests.test_mesh_clean_cpu import same

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 64, 65, 257, 1025, 4097]
PARAMS = [(0, False), (ref.M, False), (0, True), (ref.M, True)]          # (min_faces, largest); normals on


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def cleaner(gpu):
    return gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)


def _upload(mesh):
    import torch
    pos, col, faces = mesh
    return (torch.from_numpy(np.ascontiguousarray(pos, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(col, np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(faces, np.uint32).view(np.int32)).cuda())


def _clean(cleaner, mesh, min_faces=0, largest=False, normals=True):
    """the device's (positions, colours, normals, faces, stats, labels) of a host mesh"""
    dev = _upload(mesh)
    out = cleaner.clean(dev, min_faces, largest, normals)
    return out + (cleaner.clean_labels(len(mesh[0])),)


@pytest.mark.parametrize("order", ref.ORDERS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_clean_planted_families(cleaner, family, order):
    for T in SIZES:
        mesh = ref.build(family, T, seed=T, order=order)
        for min_faces, largest in PARAMS:
            err = same(_clean(cleaner, mesh, min_faces, largest), ref.clean(*mesh, min_faces, largest, True))
            assert err is None, (family, order, T, min_faces, largest, err)


def test_clean_islands_past_one_step_of_the_vertex_tile_scan(cleaner):
    mesh = ref.islands(87382, seed=1, order="shuffled")
    assert len(mesh[0]) == 262146
    got = _clean(cleaner, mesh, 0, False)
    assert same(got, ref.clean(*mesh, 0, False, True)) is None and got[4]["numComponents"] == 87382
    assert _clean(cleaner, mesh, 2, False)[4]["numVerticesOut"] == 0


def test_clean_patches_past_one_step_of_the_face_tile_scan(cleaner):
    mesh = ref.patches(131100, seed=2, order="descending")
    assert len(mesh[2]) > 262144
    got = _clean(cleaner, mesh, ref.M, False)          # everything but the patch of M - 1 faces stays: 257 tiles of kept faces too
    assert same(got, ref.clean(*mesh, ref.M, False, True)) is None and got[4]["numFacesOut"] == len(mesh[2]) - (ref.M - 1)


@pytest.mark.parametrize("family", ["strip", "fan"])
def test_clean_contended_chain_and_hub_twice(cleaner, family):
    """4097 shuffled: every face of the strip hooks into one chain, every face of the fan into one hub; two runs give the same labels and the same arrays"""
    mesh = ref.build(family, 4097, seed=3, order="shuffled")
    want = ref.clean(*mesh, 0, False, True)
    a = _clean(cleaner, mesh); b = _clean(cleaner, mesh)
    assert same(a, want) is None and same(b, a) is None and (a[5] == 0).all()


def test_clean_one_large_component_written_from_everywhere(cleaner):
    """one shuffled patch of 100 000 faces plus a small one that holds vertex 0: the large one is labelled with its lowest id and is the one that stays"""
    rng = np.random.default_rng(4)
    pos, faces = ref._join([ref._grid_patch(100000, rng), ref._grid_patch(ref.M, rng, origin=(0.0, 0.0, 1.0))])
    mesh = ref._finish(pos, faces, "shuffled", rng, first=[len(pos) - 1])
    want = ref.clean(*mesh, 0, True, True)
    got = _clean(cleaner, mesh, 0, True)
    assert same(got, want) is None
    big = np.bincount(got[5]).argmax()
    assert got[4]["numFacesOut"] == 100000 and big == np.nonzero(got[5] == big)[0].min() and big != 0


def test_clean_identity_and_labels_are_a_fixed_point(cleaner):
    mesh = ref.patches(1025, seed=5, order="shuffled")
    got = _clean(cleaner, mesh, 0, False, normals=False)
    assert got[2] is None and all(g.shape == w.shape and np.array_equal(_bits(g), _bits(w)) for g, w in zip((got[0], got[1], got[3]), mesh))
    lab = got[5]
    assert np.array_equal(lab[lab], lab) and (lab <= np.arange(len(lab))).all() and np.array_equal(lab, ref.labels(len(lab), mesh[2]))


def test_clean_small_after_large_and_refusal(gpu, cleaner):
    large = ref.mixed(4097, seed=6, order="shuffled"); small = ref.mixed(65, seed=7, order="descending")
    assert same(_clean(cleaner, large, ref.M, False), ref.clean(*large, ref.M, False, True)) is None
    want = ref.clean(*small, ref.M, False, True)
    assert same(_clean(cleaner, small, ref.M, False), want) is None
    # a face id beyond the vertices: refused, and the last result is still there
    bad = (small[0], small[1], small[2].copy()); bad[2][17, 2] = len(small[0])
    with pytest.raises(Exception, match="numVertices"):
        cleaner.clean(_upload(bad), ref.M, False, True)
    nv, nf = len(want[0]), len(want[3])
    C = gpu.capi.C
    hp = np.zeros((nv, 3), np.float32); hn = np.zeros((nv, 3), np.float32); hf = np.zeros((nf, 3), np.uint32)
    gpu.capi.check(gpu.capi.lib.bf_marching_cubes_download_clean(cleaner._h, hp.ctypes.data_as(C.c_void_p), None, hn.ctypes.data_as(C.c_void_p), hf.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(_bits(hp), _bits(want[0])) and np.array_equal(_bits(hn), _bits(want[2])) and np.array_equal(hf, want[3])
    assert np.array_equal(cleaner.clean_labels(len(small[0])), want[5])


# --------------------------------------------------------------------------- behind the weld
def _floater(k, seed, origin):
    """a planted piece of k faces as a triangle soup [k,3,6]"""
    rng = np.random.default_rng(seed)
    p, f = ref._grid_patch(k, rng, origin=origin)
    tri = np.zeros((k, 3, 6), np.float32)
    tri[:, :, :3] = p.astype(np.float32)[f]
    tri[:, :, 3:] = rng.uniform(0, 1, (k, 1, 3)).astype(np.float32)
    return tri


def test_clean_behind_the_weld_on_a_volume(gpu, tmp_path):
    """the three-frame 160 x 120 volume at 2 cm of tests/test_mesh_weld_gpu.py, with floaters of 1, 5 and 40 faces planted 10 m away: min_faces = 41 drops exactly
    those the restatement drops.  Then the file of save_mesh_clean over the extraction itself."""
    import torch
    gs, p = weld_gpu._volume(gpu)
    mc = gpu.capi.MarchingCubesHashSDF(600000, p.m_hashNumBuckets, 0.02)
    tris, found = mc.extract(gs)
    assert found == len(tris) > 5000
    planted = np.concatenate([tris[:len(tris) // 2], _floater(5, 1, (10.0, 0.0, 0.0)), tris[len(tris) // 2:], _floater(40, 2, (0.0, 10.0, 0.0)), _floater(1, 3, (0.0, 0.0, -10.0))])
    for transform in (None, mesh_weld_ref.TRANSFORM):
        welded = mesh_weld_ref.weld(planted, transform)
        got_weld = mc.weld(torch.from_numpy(planted).cuda(), transform)
        assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got_weld, welded))
        want = ref.clean(*welded, 41, False, True)
        got = mc.clean(None, 41, False, True) + (mc.clean_labels(len(welded[0])),)          # the last weld
        assert same(got, want) is None
        st = got[4]
        assert st["numComponents"] >= 4 and st["numComponents"] - st["numComponentsKept"] >= 3 and st["numFacesIn"] - st["numFacesOut"] >= 46
        gpu.capi.write_ply_indexed_normals(tmp_path / "planted.ply", got[0], got[2], got[1], got[3])
        assert (tmp_path / "planted.ply").read_bytes() == ref.ply_bytes_normals(want[0], want[2], want[1], want[3])
        # the file, from the extraction: weld + clean + PLY in one call
        assert mc.extract_gpu(gs) == (found, found)
        own = ref.clean(*mesh_weld_ref.weld(tris, transform), 41, False, True)
        st = mc.save_mesh_clean(tmp_path / "clean.ply", transform, 41, False, True)
        assert {k: st[k] for k in ref.STAT_KEYS} == own[4]
        assert (tmp_path / "clean.ply").read_bytes() == ref.ply_bytes_normals(own[0], own[2], own[1], own[3])
    # without normals and with nothing to drop: the file of save_mesh_gpu
    mc.save_mesh_clean(tmp_path / "plain.ply", None, 0, False, False)
    full = ref.clean(*mesh_weld_ref.weld(tris), 0, False, False)
    assert (tmp_path / "plain.ply").read_bytes() == mesh_weld_ref.ply_bytes(full[0], full[1], full[3])
    if full[4]["numIsolatedVertices"] == 0:
        mc.save_mesh_gpu(tmp_path / "weld.ply")
        assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "weld.ply").read_bytes()


# --------------------------------------------------------------------------- the frame loop
MIN_FACES = 100


def _run_pipeline(gpu, n, mesh_dir):
    """the 25-frame configuration of tests/test_mesh_weld_gpu.py::_run_pipeline; mesh_dir: save the cleaned mesh after frame 12 and after the last frame"""
    import torch
    frames = weld_gpu._stream(n)
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = weld_gpu.PW, weld_gpu.PH
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.02, 50000, 20000
    gbs.s_maxNumImages = 8
    gp = gpu.capi.Pipeline(gas, gbs, sensor_desc(weld_gpu.PW, weld_gpu.PH, K))
    results = []
    for k, (d, c, T, _) in enumerate(frames):
        assert gp.process_frame(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda())
        if mesh_dir is not None and k == 12:
            results.append(gp.save_mesh_clean(mesh_dir / "mid.ply", None, MIN_FACES, False, True))
    if mesh_dir is not None:
        results.append(gp.save_mesh_clean(mesh_dir / "final.ply", None, MIN_FACES, False, True))
    gp.synchronize()
    return gp, gas, results


def test_pipeline_save_mesh_clean_leaves_the_reconstruction_alone(gpu, tmp_path):
    """one run saves the cleaned mesh after frame 12 and after the last frame, the other never: the same trajectories, bf_scene_debug_hash, heap free count,
    allocated blocks and counters; the final file is stand-alone extract -> the restatement's weld and clean -> bytes"""
    n = 25
    plain, _, _ = _run_pipeline(gpu, n, None)
    a = weld_gpu._volume_state(plain)
    plain.close()
    gp, gas, results = _run_pipeline(gpu, n, tmp_path)
    b = weld_gpu._volume_state(gp)
    assert np.array_equal(_bits(a["traj"]), _bits(b["traj"])) and np.array_equal(_bits(a["opt"]), _bits(b["opt"]))
    assert a["dbg"] == b["dbg"] and a["heap_free"] == b["heap_free"] and a["blocks"] == b["blocks"] and a["counters"] == b["counters"]
    mc = gpu.capi.MarchingCubesHashSDF.from_global_app_state(gas, max_triangles=3000000)
    tris, found = mc.extract(gp.scene())
    assert found == len(tris) > 5000
    welded = mesh_weld_ref.weld(tris)
    want = ref.clean(*welded, MIN_FACES, False, True)
    stats, nt = results[1]
    assert nt == found and {k: stats[k] for k in ref.STAT_KEYS} == want[4]
    assert (tmp_path / "final.ply").read_bytes() == ref.ply_bytes_normals(want[0], want[2], want[1], want[3])
    assert results[0][1] > 0 and (tmp_path / "mid.ply").read_bytes() != (tmp_path / "final.ply").read_bytes()
    nv, nf, nt2 = gp.save_mesh(tmp_path / "uncleaned.ply")
    assert (nv, nf, nt2) == (stats["numVerticesIn"], stats["numFacesIn"], found)
    # only the largest, moved, without normals
    stats, _ = gp.save_mesh_clean(tmp_path / "largest.ply", mesh_weld_ref.TRANSFORM, 0, True, False)
    big = ref.clean(*mesh_weld_ref.weld(tris, mesh_weld_ref.TRANSFORM), 0, True, False)
    assert stats["numComponentsKept"] == 1 and (tmp_path / "largest.ply").read_bytes() == mesh_weld_ref.ply_bytes(big[0], big[1], big[3])
    c = weld_gpu._volume_state(gp)
    assert c["dbg"] == b["dbg"] and c["heap_free"] == b["heap_free"] and c["blocks"] == b["blocks"]
    gp.close()


def test_pipeline_save_mesh_clean_refuses_a_sharded_volume(gpu, tmp_path):
    frames = weld_gpu._stream(25)
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = weld_gpu.PW, weld_gpu.PH
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.02, 50000, 20000
    gbs.s_maxNumImages = 8
    gp = gpu.capi.Pipeline(gas, gbs, sensor_desc(weld_gpu.PW, weld_gpu.PH, K))
    gp.set_volume_shard(0, 2)
    with pytest.raises(Exception, match="shard"):
        gp.save_mesh_clean(tmp_path / "shard.ply", None, MIN_FACES, False, True)
    assert not (tmp_path / "shard.ply").exists()
    gp.close()
