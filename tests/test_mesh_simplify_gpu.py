"""GPU tests (-m gpu) of the device mesh simplification (csrc/meshsimplify.hip) and of the entry points built on it, against the numpy restatement
tests/mesh_simplify_ref.py.  Bar: positions, colours and normals compared as uint32; faces, map and stats exactly; PLY files byte for byte - tolerance 0.

Sizes: the kernels work in 64-lane waves and 256-thread workgroups, count and compact in tiles of 1024 elements and scan the tile counts 256 at a time; the
accumulation combines equal cluster numbers inside a wave.  63 / 64 / 65 are either side of a wave, 257 is just above a workgroup, 1025 just above a tile, 4097
gives several tiles; more than 262 144 leaders, kept faces or clusters are past one step of the tile-count scan (257 tiles); 100 000 members of one cluster is
every wave of the grid adding to the same seven counters; 8 404 097 members near 1024 m is where the int64 sum stops being a binary64 number."""
import gc as _gc

import numpy as np
import pytest

from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix, sensor_desc
from tests import mesh_clean_ref
from tests import mesh_simplify_ref as ref
from tests import mesh_weld_ref
from tests import test_mesh_weld_gpu as weld_gpu
from tests.test_mesh_clean_gpu import _floater
from tests.test_mesh_simplify_cpu import SIZES, big_sum_mesh, refusal_cases, same, want

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def simp(gpu):
    return gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)


def _upload(mesh):
    import torch
    pos, col, faces = mesh[:3]
    return (torch.from_numpy(np.ascontiguousarray(pos, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(col, np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(faces, np.uint32).view(np.int32)).cuda())


def _simplify(simp, mesh, normals=True, dev=None):
    """the device's (positions, colours, normals, faces, stats, map) of a host mesh (positions, colours, faces, cell size, ...)"""
    out = simp.simplify(dev if dev is not None else _upload(mesh), mesh[3], normals)
    return out + (simp.simplify_map(len(mesh[0])),)


@pytest.mark.parametrize("order", ref.ORDERS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_simplify_planted_families(simp, family, order):
    """every size either side of a wave, a workgroup and a tile, with and without normals: `in` given explicitly; and as NULL behind a clean that drops nothing
    but the vertices no face uses, against the restatement of both"""
    for T in SIZES:
        mesh, _ = want(family, T, order, True)
        dev = _upload(mesh)
        for normals in (False, True):
            err = same(_simplify(simp, mesh, normals, dev), want(family, T, order, normals)[1])
            assert err is None, (family, order, T, normals, err)
        cleaned = mesh_clean_ref.clean(*mesh[:3], 0, False, False)
        simp.clean(dev, 0, False, False)
        got = simp.simplify(None, mesh[3], True) + (simp.simplify_map(len(cleaned[0])),)
        err = same(got, ref.simplify(cleaned[0], cleaned[1], cleaned[3], mesh[3], True))
        assert err is None, (family, order, T, "behind a clean", err)


def test_simplify_without_a_clean_refuses_a_null_input(gpu):
    mc = gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)
    with pytest.raises(Exception, match="clean"):
        mc.simplify(None, 0.05, True)
    mc.close()


def test_simplify_leaders_past_one_step_of_the_tile_scan(simp):
    """more than 262 144 vertices that are all leaders, and as many kept faces: the output is the input"""
    mesh = ref.singles(523000, seed=1, order="shuffled")
    assert len(mesh[0]) > 262144 and len(mesh[2]) > 262144
    got = _simplify(simp, mesh)
    assert same(got, ref.simplify(*mesh[:4], True)) is None
    assert np.array_equal(_bits(got[0]), _bits(mesh[0])) and np.array_equal(got[3], mesh[2]) and got[4]["numClusters"] == len(mesh[0])


def test_simplify_kept_faces_past_one_step_of_the_tile_scan(simp):
    """`grid` with a cell below its spacing: every face but the planted duplicates stays"""
    pos, col, faces, _, _ = ref.grid(270000, seed=2, order="descending")
    mesh = (pos, col, faces, 0.004)
    got = _simplify(simp, mesh)
    assert same(got, ref.simplify(*mesh, True)) is None
    assert got[4]["numFacesOut"] == 270000 and got[4]["numFacesDuplicate"] == 54000 and got[4]["largestCluster"] == 1


def test_simplify_clusters_past_one_step_of_the_tile_scan(simp):
    """`grid` with a cell of one and a half spacings: more than 262 144 clusters of several members each"""
    pos, col, faces, _, _ = ref.grid(1200000, seed=3, order="shuffled")
    mesh = (pos, col, faces, 0.015)
    want_ = ref.simplify(*mesh, True)
    assert want_[4]["numClusters"] > 262144 and want_[4]["largestCluster"] >= 4 and want_[4]["numFacesCollapsed"] > 0
    assert same(_simplify(simp, mesh), want_) is None


def _two_cells(n, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.uniform(0.05, 0.95, (n, 3)) + np.stack([rng.integers(0, 2, n), np.zeros(n), np.zeros(n)], 1)).astype(np.float32)
    return pos, rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.integers(0, n, (n, 3)).astype(np.uint32), 1.0


@pytest.mark.parametrize("case", ["hub_4097_shuffled", "hub_100000", "two_cells"])
def test_simplify_contended_clusters_twice(simp, case):
    """every vertex of the hub adds to one cluster's counters, every vertex of `two_cells` to one of two; two runs give the same bits, those of the restatement"""
    mesh = {"hub_4097_shuffled": lambda: ref.hub(4097, 4, "shuffled")[:4], "hub_100000": lambda: ref.hub(100000, 5, "shuffled")[:4], "two_cells": lambda: _two_cells(100000, 6)}[case]()
    want_ = ref.simplify(*mesh, True)
    dev = _upload(mesh)
    a = _simplify(simp, mesh, True, dev); b = _simplify(simp, mesh, True, dev)
    assert same(a, want_) is None and same(b, a) is None
    if case == "two_cells":
        assert a[4]["numClusters"] == 2 and a[4]["numFacesOut"] == 0 and a[4]["largestCluster"] > 49000 and (a[5] == ref.NONE).all()
    else:
        assert a[4]["largestCluster"] == len(mesh[0]) - 8 and a[4]["numFacesOut"] == 8


def test_simplify_sum_beyond_2_53_device_vs_host(gpu, simp):
    pos, col, faces, cell, S = big_sum_mesh()
    assert S > 2 ** 53 and int(np.float64(S)) != S
    host = gpu.capi.mesh_simplify_host(pos, col, faces, cell, True)
    got = _simplify(simp, (pos, col, faces, cell))
    assert same(got, host) is None and got[4]["largestCluster"] == 8404097 and got[4]["numVerticesOut"] == 6


def test_simplify_small_after_large_and_refusals(gpu, simp):
    large = ref.build("mixed@coarse", 4097, 6, "shuffled"); small = ref.grid(257, 7, "descending")
    assert same(_simplify(simp, large), ref.simplify(*large[:4], True)) is None
    live = gpu.capi.debug_live_resources()
    w = ref.simplify(*small[:4], True)
    assert same(_simplify(simp, small), w) is None
    assert gpu.capi.debug_live_resources()[:4] == live[:4]          # the larger buffers serve the smaller mesh
    nv, nf = len(w[0]), len(w[3])
    for name, pos, col, faces, cell in refusal_cases():
        with pytest.raises(Exception):
            simp.simplify(_upload((pos, col, faces)), cell, True)
        # the last result is still there, unchanged
        got = simp.download_simplified(nv, nf, True) + (w[4], simp.simplify_map(len(small[0])))
        assert same(got, w) is None, name


def test_simplify_gives_everything_back(gpu):
    _gc.collect()
    live = gpu.capi.debug_live_resources()
    mc = gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)
    mesh = ref.grid(1025, 8, "shuffled")
    assert same(_simplify(mc, mesh), ref.simplify(*mesh[:4], True)) is None
    assert gpu.capi.debug_live_resources()[1] > live[1]
    mc.close()
    _gc.collect()
    assert gpu.capi.debug_live_resources()[:4] == live[:4] and gpu.capi.debug_live_resources()[5] == 0


# --------------------------------------------------------------------------- behind the weld and the clean
CELL = 0.05


def test_simplify_behind_the_weld_and_the_clean_on_a_volume(gpu, tmp_path):
    """the three-frame 160 x 120 volume at 2 cm of tests/test_mesh_weld_gpu.py with the clean's planted floaters: clean(41) then simplify(5 cm), moved and not"""
    import torch
    gs, p = weld_gpu._volume(gpu)
    mc = gpu.capi.MarchingCubesHashSDF(600000, p.m_hashNumBuckets, 0.02)
    tris, found = mc.extract(gs)
    assert found == len(tris) > 5000
    planted = np.concatenate([tris[:len(tris) // 2], _floater(5, 1, (10.0, 0.0, 0.0)), tris[len(tris) // 2:], _floater(40, 2, (0.0, 10.0, 0.0)), _floater(1, 3, (0.0, 0.0, -10.0))])
    for transform in (None, mesh_weld_ref.TRANSFORM):
        cleaned = mesh_clean_ref.clean(*mesh_weld_ref.weld(planted, transform), 41, False, False)
        w = ref.simplify(cleaned[0], cleaned[1], cleaned[3], CELL, True)
        mc.weld(torch.from_numpy(planted).cuda(), transform)
        mc.clean(None, 41, False, False)
        got = mc.simplify(None, CELL, True) + (mc.simplify_map(len(cleaned[0])),)
        assert same(got, w) is None
        st = got[4]
        assert 0 < st["numFacesOut"] < st["numFacesIn"] and st["numFacesIn"] == st["numFacesOut"] + st["numFacesCollapsed"] + st["numFacesDuplicate"]
        assert st["numVerticesOut"] <= st["numClusters"] <= st["numVerticesIn"] == len(cleaned[0])
        # through the map: a vertex lies within the diagonal of its cell (widened by the quantisation and the binary32 rounding below 8 m) of its output vertex
        there = got[5] != ref.NONE
        d = np.linalg.norm(cleaned[0][there].astype(np.float64) - got[0][got[5][there]].astype(np.float64), axis=1)
        assert there.any() and d.max() <= np.sqrt(3.0) * (CELL + 2e-6)
        # the file, from the extraction: weld + clean + simplify + PLY in one call; the normals are the simplified mesh's, asked for by the clean's params alone
        assert mc.extract_gpu(gs) == (found, found)
        own_clean = mesh_clean_ref.clean(*mesh_weld_ref.weld(tris, transform), 41, False, False)
        own = ref.simplify(own_clean[0], own_clean[1], own_clean[3], CELL, True)
        cst, sst = mc.save_mesh_simplified(tmp_path / "simple.ply", CELL, transform, 41, False, True)
        assert {k: cst[k] for k in mesh_clean_ref.STAT_KEYS} == own_clean[4] and sst == own[4]
        assert (tmp_path / "simple.ply").read_bytes() == ref.ply_bytes(own[0], own[2], own[1], own[3])
    cst, sst = mc.save_mesh_simplified(tmp_path / "plain.ply", CELL, None, 41, False, False)
    own_clean = mesh_clean_ref.clean(*mesh_weld_ref.weld(tris), 41, False, False)
    own = ref.simplify(own_clean[0], own_clean[1], own_clean[3], CELL, False)
    assert (tmp_path / "plain.ply").read_bytes() == ref.ply_bytes(own[0], None, own[1], own[3])
    mc.close()


# --------------------------------------------------------------------------- the frame loop
MIN_FACES = 100


def _pipeline(gpu):
    frames = weld_gpu._stream(25)
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = weld_gpu.PW, weld_gpu.PH
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.02, 50000, 20000
    gbs.s_maxNumImages = 8
    return gpu.capi.Pipeline(gas, gbs, sensor_desc(weld_gpu.PW, weld_gpu.PH, K)), gas, frames


def _run_pipeline(gpu, mesh_dir):
    """the 25-frame configuration of tests/test_mesh_clean_gpu.py::_run_pipeline; mesh_dir: save the simplified mesh after frame 12 and after the last frame"""
    import torch
    gp, gas, frames = _pipeline(gpu)
    results = []
    for k, (d, c, T, _) in enumerate(frames):
        assert gp.process_frame(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda())
        if mesh_dir is not None and k == 12:
            results.append(gp.save_mesh_simplified(mesh_dir / "mid.ply", CELL, None, MIN_FACES, False, True))
    if mesh_dir is not None:
        results.append(gp.save_mesh_simplified(mesh_dir / "final.ply", CELL, None, MIN_FACES, False, True))
    gp.synchronize()
    return gp, gas, results


def test_pipeline_save_mesh_simplified_leaves_the_reconstruction_alone(gpu, tmp_path):
    """one run saves the simplified mesh after frame 12 and after the last frame, the other never: the same trajectories, bf_scene_debug_hash, heap free count,
    allocated blocks and counters; the final file is stand-alone extract -> the restatements' weld, clean and simplify -> bytes"""
    plain, _, _ = _run_pipeline(gpu, None)
    a = weld_gpu._volume_state(plain)
    plain.close()
    gp, gas, results = _run_pipeline(gpu, tmp_path)
    b = weld_gpu._volume_state(gp)
    assert np.array_equal(_bits(a["traj"]), _bits(b["traj"])) and np.array_equal(_bits(a["opt"]), _bits(b["opt"]))
    assert a["dbg"] == b["dbg"] and a["heap_free"] == b["heap_free"] and a["blocks"] == b["blocks"] and a["counters"] == b["counters"]
    mc = gpu.capi.MarchingCubesHashSDF.from_global_app_state(gas, max_triangles=3000000)
    tris, found = mc.extract(gp.scene())
    assert found == len(tris) > 5000
    cleaned = mesh_clean_ref.clean(*mesh_weld_ref.weld(tris), MIN_FACES, False, False)
    w = ref.simplify(cleaned[0], cleaned[1], cleaned[3], CELL, True)
    cst, sst, nt = results[1]
    assert nt == found and {k: cst[k] for k in mesh_clean_ref.STAT_KEYS} == cleaned[4] and sst == w[4] and 0 < sst["numFacesOut"] < sst["numFacesIn"]
    assert (tmp_path / "final.ply").read_bytes() == ref.ply_bytes(w[0], w[2], w[1], w[3])
    assert results[0][2] > 0 and (tmp_path / "mid.ply").read_bytes() != (tmp_path / "final.ply").read_bytes()
    c = weld_gpu._volume_state(gp)
    assert c["dbg"] == b["dbg"] and c["heap_free"] == b["heap_free"] and c["blocks"] == b["blocks"]
    mc.close()
    gp.close()


def test_pipeline_save_mesh_simplified_refuses_a_sharded_volume(gpu, tmp_path):
    gp, _, _ = _pipeline(gpu)
    gp.set_volume_shard(0, 2)
    with pytest.raises(Exception, match="shard"):
        gp.save_mesh_simplified(tmp_path / "shard.ply", CELL, None, MIN_FACES, False, True)
    assert not (tmp_path / "shard.ply").exists()
    gp.close()
