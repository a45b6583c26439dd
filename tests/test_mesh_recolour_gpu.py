"""GPU tests (-m gpu) of the device mesh recolouring (csrc/meshrecolour.hip) and of the entry points built on it, against the numpy restatement
tests/mesh_recolour_ref.py.  Bar: colours compared as uint32, view counts and stats exactly, PLY files byte for byte - tolerance 0.

Sizes: the kernel works in 64-lane waves and 256-thread workgroups, one thread per vertex, and past 8192 workgroups a thread takes a second vertex: 63 / 64 / 65 are
either side of a wave, 255 / 256 / 257 either side of a workgroup, 8192 * 256 + 1 is one vertex past a step of the vertex loop.  All frames go in one launch, so
there is no batch size to cross."""
import gc as _gc

import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix, sensor_desc
from tests import mesh_clean_ref
from tests import mesh_recolour_cases as cases
from tests import mesh_recolour_ref as R
from tests import mesh_simplify_ref
from tests import mesh_weld_ref
from tests import test_mesh_weld_gpu as weld_gpu
from tests.test_mesh_recolour_cpu import MODES, all_cases, random_want, refusals, rparams, want, with_mode

pytestmark = pytest.mark.gpu

GRID_STEP = 8192 * 256


@pytest.fixture(scope="module")
def mc(gpu):
    return gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)


class Dev:
    """a case's mesh and frames in device memory (kept alive by this object)"""

    def __init__(self, capi, case):
        import torch
        self.mesh = tuple(torch.from_numpy(np.ascontiguousarray(case[k], np.float32)).cuda() if case[k] is not None else None for k in ("pos", "col", "nrm")) + (None,)
        self.images = [(torch.from_numpy(f[0]).cuda(), torch.from_numpy(f[1]).cuda()) for f in case["frames"]]
        self.frames = capi.recolour_frames([(d.data_ptr(), c.data_ptr(), f[2], f[3], f[4]) for (d, c), f in zip(self.images, case["frames"])])


def device(capi, mc, case, dev=None):
    dev = dev or Dev(capi, case)
    return mc.recolour(dev.mesh, dev.frames, case["w"], case["h"], case["K"], rparams(case["params"]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_recolour_planted_families(gpu, mc, family, mode):
    for case in all_cases():
        if case["family"] != family:
            continue
        case = with_mode(case, mode)
        err = R.same(device(gpu.capi, mc, case), want(case)[:3])
        assert err is None, (case["name"], err)


@pytest.mark.parametrize("mode", MODES)
def test_recolour_random_sphere(gpu, mc, mode):
    case, w = random_want(mode)
    err = R.same(device(gpu.capi, mc, case), w[:3])
    assert err is None, err


def _resized(case, n, frames=None):
    idx = np.arange(n) % len(case["pos"])
    return dict(case, pos=case["pos"][idx], nrm=case["nrm"][idx], col=case["col"][idx], frames=case["frames"] if frames is None else case["frames"][:frames])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_recolour_vertex_counts_around_a_wave_and_a_workgroup(gpu, mc, n):
    case = _resized(random_want(0)[0], n)
    assert R.same(device(gpu.capi, mc, case), want(case)[:3]) is None


def test_recolour_one_vertex_past_a_step_of_the_vertex_loop_then_a_small_mesh(gpu, mc):
    """8192 * 256 + 1 vertices (the sphere's, repeated: vertex i and vertex i - 8192 * 256 differ) against two frames; then a small mesh, which the buffers of
    the large one serve"""
    large = _resized(random_want(0)[0], GRID_STEP + 1, frames=2)
    got = device(gpu.capi, mc, large)
    w = want(large)
    assert GRID_STEP % len(random_want(0)[0]["pos"]) != 0
    assert R.same(got, w[:3]) is None
    live = gpu.capi.debug_live_resources()
    small = _resized(random_want(1)[0], 257)
    assert R.same(device(gpu.capi, mc, small), want(small)[:3]) is None
    assert gpu.capi.debug_live_resources()[:4] == live[:4]          # the larger buffers serve the smaller mesh (the test's own tensors are torch's)


def test_recolour_refusals_leave_the_last_result(gpu, mc):
    capi = gpu.capi
    good = with_mode(cases.random_case(n=300), 0)
    dev = Dev(capi, good)
    w = want(good)
    assert R.same(device(capi, mc, good, dev), w[:3]) is None
    for name, change in refusals():
        bad = dict(good, **change)
        bdev = Dev(capi, bad) if "nrm" in change else dev
        with pytest.raises(capi.BFError):
            mc.recolour(bdev.mesh, bdev.frames, bad["w"], bad["h"], bad["K"], rparams(bad["params"]))
        got = (mc.download_recoloured(len(good["pos"]), 0)[1], mc.recolour_views(len(good["pos"])), w[2])
        assert R.same(got, w[:3]) is None, name


def test_recolour_without_a_mesh_refuses_a_null_input(gpu):
    m = gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)
    case = cases.meaning_case()
    dev = Dev(gpu.capi, case)
    with pytest.raises(gpu.capi.BFError, match="clean"):
        m.recolour(None, dev.frames, case["w"], case["h"], case["K"], rparams(case["params"]))
    m.close()


def test_recolour_gives_everything_back(gpu):
    _gc.collect()
    live = gpu.capi.debug_live_resources()
    m = gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)
    case = with_mode(cases.random_case(n=1025), 0)
    dev = Dev(gpu.capi, case)
    assert R.same(device(gpu.capi, m, case, dev), want(case)[:3]) is None
    assert gpu.capi.debug_live_resources()[1] > live[1]
    m.close()
    del dev
    _gc.collect()
    assert gpu.capi.debug_live_resources()[:4] == live[:4] and gpu.capi.debug_live_resources()[5] == 0


# --------------------------------------------------------------------------- behind the weld and the clean
CELL = 0.05


def _default_params(mode=0):
    gas = default_app_state()
    return R.params(depthMin=gas.s_sensorDepthMin, depthMax=gas.s_SDFMaxIntegrationDistance, depthTolerance=0.01, depthToleranceLin=0.01, minCos=0.3, mode=mode)


def test_recolour_behind_the_weld_and_the_clean_on_a_volume(gpu, tmp_path):
    """the three-frame 160 x 120 volume at 2 cm of tests/test_mesh_weld_gpu.py, recoloured from those three frames with the pipeline's default parameters, moved
    and not: the device against the restatement as bits; more than half of the vertices are recoloured, which the wrong sign of the normals (every pair FACING)
    or a tolerance below the mesh's distance from the depth images would not give; then the simplification of the recoloured mesh"""
    import torch
    capi = gpu.capi
    gs, p = weld_gpu._volume(gpu)
    W, H = 160, 120
    shots = [synth.scene_room(k, W, H) for k in (0, 20, 40)]
    Kd = shots[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    images = [(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()) for d, c, _, _ in shots]
    m = capi.MarchingCubesHashSDF(600000, p.m_hashNumBuckets, 0.02)
    tris, found = m.extract(gs)
    assert found == len(tris) > 5000
    for transform in (None, mesh_weld_ref.TRANSFORM):
        for mode in MODES:
            rp = _default_params(mode)
            poses = [T if transform is None else R.mul44(transform, T) for _, _, T, _ in shots]
            frames = [(d, c) + capi.mesh_recolour_frame_from_pose(M) for (d, c, _, _), M in zip(shots, poses)]
            assert not any(f[4] for f in frames)
            cleaned = mesh_clean_ref.clean(*mesh_weld_ref.weld(tris, transform), 41, False, True)
            w = R.recolour(cleaned[0], cleaned[2], cleaned[1], frames, W, H, K, rp)
            m.weld(None, transform)
            m.clean(None, 41, False, True)
            dframes = capi.recolour_frames([(d.data_ptr(), c.data_ptr(), f[2], f[3], f[4]) for (d, c), f in zip(images, frames)])
            got = m.recolour(None, dframes, W, H, K, rparams(rp))
            st = got[2]
            print("recoloured %d of %d vertices (mode %d, %s), most views %d" % (st["numRecoloured"], st["numVertices"], mode, "moved" if transform is not None else "in place", st["maxViews"]))
            err = R.same(got, w[:3])
            assert err is None, err
            assert st["numVertices"] == len(cleaned[0]) and 2 * st["numRecoloured"] > st["numVertices"]
            down = m.download_recoloured(len(cleaned[0]), len(cleaned[3]), True)
            assert all(np.array_equal(R.bits(x), R.bits(y)) for x, y in zip(down[:3], (cleaned[0], w[0], cleaned[2]))) and np.array_equal(down[3], cleaned[3])
            # a recoloured mesh is a legal input of the simplification, and its colour array is not the simplification's scratch
            simple = m.simplify_recoloured(CELL, True) + (m.simplify_map(len(cleaned[0])),)
            sref = mesh_simplify_ref.simplify(cleaned[0], w[0], cleaned[3], CELL, True)
            assert mesh_simplify_ref_same(simple, sref)
            assert np.array_equal(R.bits(m.download_recoloured(len(cleaned[0]), 0)[1]), R.bits(w[0]))
            # the simplify ran later than the clean: a NULL input is now the simplified mesh, with its own normals
            again = m.recolour(None, dframes, W, H, K, rparams(rp))
            err = R.same(again, R.recolour(sref[0], sref[2], sref[1], frames, W, H, K, rp)[:3])
            assert err is None and again[2]["numVertices"] == len(sref[0]) < len(cleaned[0]), err
        # the file, from the extraction: weld + clean + recolour (+ simplify) + PLY in one call; the clean's params ask for no normals, the file has none
        rp = _default_params(0)
        assert m.extract_gpu(gs) == (found, found)
        cst, rst, sst = m.save_mesh_recoloured(tmp_path / "re.ply", dframes, W, H, K, rparams(rp), transform, 41, False, False)
        w = R.recolour(cleaned[0], cleaned[2], cleaned[1], frames, W, H, K, rp)
        assert {k: cst[k] for k in mesh_clean_ref.STAT_KEYS} == cleaned[4] and rst == w[2] and sst is None
        assert (tmp_path / "re.ply").read_bytes() == R.ply_bytes(cleaned[0], None, w[0], cleaned[3])
        cst, rst, sst = m.save_mesh_recoloured(tmp_path / "re_simple.ply", dframes, W, H, K, rparams(rp), transform, 41, False, True, CELL)
        own = mesh_simplify_ref.simplify(cleaned[0], w[0], cleaned[3], CELL, True)
        assert rst == w[2] and sst == own[4]
        assert (tmp_path / "re_simple.ply").read_bytes() == R.ply_bytes(own[0], own[2], own[1], own[3])
    m.close()


def mesh_simplify_ref_same(got, w):
    from tests.test_mesh_simplify_cpu import same
    return same(got, w) is None


# --------------------------------------------------------------------------- the frame loop
MIN_FACES = 100
STRIDE = 10


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
    """the 25-frame configuration of tests/test_mesh_simplify_gpu.py::_run_pipeline; mesh_dir: save the recoloured mesh after frame 12 and after the last frame"""
    import torch
    gp, gas, frames = _pipeline(gpu)
    results = []
    for k, (d, c, T, _) in enumerate(frames):
        assert gp.process_frame(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda())
        if mesh_dir is not None and k == 12:
            results.append(gp.save_mesh_recoloured(mesh_dir / "mid.ply", None, MIN_FACES, False, True, None, STRIDE))
    if mesh_dir is not None:
        results.append(gp.save_mesh_recoloured(mesh_dir / "final.ply", None, MIN_FACES, False, True, None, STRIDE))
    gp.synchronize()
    return gp, gas, results


def test_pipeline_save_mesh_recoloured_leaves_the_reconstruction_alone(gpu, tmp_path):
    """one run saves the recoloured mesh after frame 12 and after the last frame, the other never: the same trajectories, bf_scene_debug_hash, heap free count,
    allocated blocks and counters; the final file is stand-alone extract -> the restatements' weld, clean and recolour (frames and poses: the stored frames on the
    stride under the optimised trajectory, through bf_mesh_recolour_frame_from_pose) -> bytes; the same with the simplification behind it"""
    plain, _, _ = _run_pipeline(gpu, None)
    a = weld_gpu._volume_state(plain)
    plain.close()
    gp, gas, results = _run_pipeline(gpu, tmp_path)
    b = weld_gpu._volume_state(gp)
    assert np.array_equal(R.bits(a["traj"]), R.bits(b["traj"])) and np.array_equal(R.bits(a["opt"]), R.bits(b["opt"]))
    assert a["dbg"] == b["dbg"] and a["heap_free"] == b["heap_free"] and a["blocks"] == b["blocks"] and a["counters"] == b["counters"]
    m = gpu.capi.MarchingCubesHashSDF.from_global_app_state(gas, max_triangles=3000000)
    tris, found = m.extract(gp.scene())
    assert found == len(tris) > 5000
    cleaned = mesh_clean_ref.clean(*mesh_weld_ref.weld(tris), MIN_FACES, False, True)
    frames, K, W, H = gp.mesh_recolour_frames_host(STRIDE)
    assert len(frames) >= 2 and (W, H) == (weld_gpu.PW, weld_gpu.PH)          # (the frames of the last, unfinished chunk have no optimised pose yet)
    d = gp.mesh_recolour_defaults()
    rp = R.params(d.depthMin, d.depthMax, d.depthTolerance, d.depthToleranceLin, d.minCos, d.mode)
    assert all(np.float32(rp[k]) == np.float32(v) for k, v in _default_params(0).items())
    w = R.recolour(cleaned[0], cleaned[2], cleaned[1], frames, W, H, K, rp)
    cst, rst, sst, nt = results[1]
    print("frame loop: recoloured %d of %d vertices from %d frames" % (rst["numRecoloured"], rst["numVertices"], rst["numFramesUsed"]))
    assert nt == found and {k: cst[k] for k in mesh_clean_ref.STAT_KEYS} == cleaned[4] and rst == w[2] and sst is None and rst["numRecoloured"] > 0
    assert (tmp_path / "final.ply").read_bytes() == R.ply_bytes(cleaned[0], cleaned[2], w[0], cleaned[3])
    assert results[0][3] > 0 and (tmp_path / "mid.ply").read_bytes() != (tmp_path / "final.ply").read_bytes()
    # with simplifyParams: the recoloured mesh's clusters; the normals are the simplified mesh's
    cst, rst, sst, nt = gp.save_mesh_recoloured(tmp_path / "simple.ply", None, MIN_FACES, False, True, None, STRIDE, CELL)
    own = mesh_simplify_ref.simplify(cleaned[0], w[0], cleaned[3], CELL, True)
    assert nt == found and rst == w[2] and sst == own[4] and 0 < sst["numFacesOut"] < sst["numFacesIn"]
    assert (tmp_path / "simple.ply").read_bytes() == R.ply_bytes(own[0], own[2], own[1], own[3])
    # best view, moved: the transform reaches the vertices and the poses alike
    best = gpu.capi.MeshRecolourParams(d.depthMin, d.depthMax, d.depthTolerance, d.depthToleranceLin, d.minCos, 1)
    gp.save_mesh_recoloured(tmp_path / "moved.ply", mesh_weld_ref.TRANSFORM, MIN_FACES, False, False, best, STRIDE)
    moved = mesh_clean_ref.clean(*mesh_weld_ref.weld(tris, mesh_weld_ref.TRANSFORM), MIN_FACES, False, True)
    mframes = gp.mesh_recolour_frames_host(STRIDE, mesh_weld_ref.TRANSFORM)[0]
    wm = R.recolour(moved[0], moved[2], moved[1], mframes, W, H, K, dict(rp, mode=1))
    assert (tmp_path / "moved.ply").read_bytes() == R.ply_bytes(moved[0], None, wm[0], moved[3])
    c = weld_gpu._volume_state(gp)
    assert c["dbg"] == b["dbg"] and c["heap_free"] == b["heap_free"] and c["blocks"] == b["blocks"]
    m.close()
    gp.close()


def test_pipeline_save_mesh_recoloured_refuses_a_sharded_volume(gpu, tmp_path):
    gp, _, _ = _pipeline(gpu)
    gp.set_volume_shard(0, 2)
    with pytest.raises(Exception, match="shard"):
        gp.save_mesh_recoloured(tmp_path / "shard.ply", None, MIN_FACES, False, True, None, STRIDE)
    assert not (tmp_path / "shard.ply").exists()
    gp.close()
