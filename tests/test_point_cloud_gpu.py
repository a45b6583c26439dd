"""GPU tests (-m gpu) of the point-cloud accumulator (include/bf_pointcloud.h, csrc/pointcloud.hip): the object through the C ABI against the numpy restatement
of tests/point_cloud_ref.py at tolerance 0 - positions and normals as bits, colours and counts exactly - over the image sizes at which the kernels take another
path, frame by frame over the planted families of tests/point_cloud_cases.py, at the densest load the parameters allow, through overflow and reset, with every
acquisition of the create failing in turn, and from inside the frame loop, where the saved file equals the host route's byte for byte and the reconstruction
does not notice."""
import ctypes as C
import gc as _gc
import os
import re

import numpy as np
import pytest

from tests import point_cloud_cases as cases
from tests import point_cloud_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases.all_cases()
_expected = {}


def expected(key, frames, K, cell, max_depth):
    """the restatement of one frame sequence, computed once and shared"""
    if key not in _expected:
        out = R.build(frames, K, cell, max_depth)
        for a in out[:3]:
            a.setflags(write=False)
        _expected[key] = out
    return _expected[key]


def same_cloud(got, want):
    return (got[0].shape == want[0].shape and np.array_equal(R.bits(got[0]), R.bits(want[0])) and np.array_equal(R.bits(got[1]), R.bits(want[1]))
            and np.array_equal(got[2], want[2]))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _add_all(pc, frames, K):
    return [pc.add_frame(_dev(D), _dev(Cc), K, T) for D, Cc, T in frames]


def _live(capi):
    _gc.collect()
    return capi.debug_live_resources()


def test_header_declares_what_the_library_exports(gpu):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bf_pointcloud.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"BF_API\s+[\w\s\*]+?\b(bf_\w+)\s*\(", txt)))
    assert len(names) == 11, names
    missing = [n for n in names if not hasattr(gpu.capi.lib, n)]
    assert not missing, missing


# 1x1 and 3x3: only the centre of the 3x3 can have a normal; 64x4: exactly one tile of the candidates kernel; 65x5, 67x9, 130x7: partial tiles on both axes, the halo
# across tile seams; 640x480: 300 scan tiles of 1024 pixels, past one 256-wide step of the tile-count scan
@pytest.mark.parametrize("w,h", [(1, 1), (3, 3), (64, 4), (65, 5), (67, 9), (130, 7), (640, 480)])
def test_image_sizes(gpu, w, h):
    K = cases.kinv(2.0 ** -9)                         # a pixel step is a third of a cell: cells are contended inside a frame and between the frames
    frames = []
    for f in range(2):
        D, Cc = cases.random_frame(w, h, seed=100 * w + f, spread=0.05)
        if (w, h) == (3, 3):
            D[:] = 1.0 + 0.01 * f; Cc[1, 1] = [9, 8, 7, 6]
        frames.append((D, Cc, cases.pose(tx=f * 2.0 ** -8, ty=-f * 2.0 ** -9)))
    want = expected(("size", w, h), frames, K, cases.CELL, cases.MAX_DEPTH)
    assert (len(want[0]) > 0) == (w >= 3 and h >= 3)
    if w * h > 9:
        assert len(want[0]) < want[3]                  # cells were contended
    pc = gpu.capi.PointCloud(max(want[3], 1), w * h, cases.CELL, cases.MAX_DEPTH)
    added = _add_all(pc, frames, K)
    assert sum(added) == len(want[0]) == pc.num_points()
    assert same_cloud(pc.download(), want)
    # the same frames without thinning: every candidate, in raster order
    flat = expected(("size flat", w, h), frames, K, 0.0, cases.MAX_DEPTH)
    assert len(flat[0]) == want[3]
    pc2 = gpu.capi.PointCloud(max(want[3], 1), w * h, 0.0, cases.MAX_DEPTH)
    assert sum(_add_all(pc2, frames, K)) == want[3]
    assert same_cloud(pc2.download(), flat)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_families_frame_by_frame(gpu, case):
    frames, K = case["frames"], case["Kinv"]
    want = expected(("case", case["name"]), frames, K, case["cell"], case["max_depth"])
    h, w = frames[0][0].shape
    pc = gpu.capi.PointCloud(max(len(want[0]), 1), w * h, case["cell"], case["max_depth"])
    added = _add_all(pc, frames, K)
    assert sum(added) == len(want[0])
    first = pc.download()
    assert same_cloud(first, want)
    # per frame: what the restatement gives for the sequence up to that frame
    for k in range(1, len(frames)):
        assert sum(added[:k]) == len(R.build(frames[:k], K, case["cell"], case["max_depth"])[0])
    # the same sequence after a reset: the same arrays
    pc.reset()
    assert pc.num_points() == 0
    assert _add_all(pc, frames, K) == added
    assert same_cloud(pc.download(), first)
    if case["cell"] > 0:
        # a frame whose cells the cloud already owns adds nothing and changes nothing
        for D, Cc, T in frames:
            assert pc.add_frame(_dev(D), _dev(Cc), K, T) == 0
        assert same_cloud(pc.download(), first)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_densest_load(gpu, seed):
    """maxPoints = the number of distinct cells, maxFramePixels = the frame: the table as full as the parameters let it get, every key different"""
    w, h = 66, 34
    K = cases.kinv(2.0 ** -6)
    frames = []
    for f in range(3):
        D, Cc = cases.distinct_frame(w, h, 10 * seed + f)
        frames.append((D, Cc, cases.pose(tx=4.0 * f)))
    want = expected(("dense", seed), frames, K, cases.CELL, cases.MAX_DEPTH)
    assert len(want[0]) == want[3] == 3 * (w - 2) * (h - 2)
    pc = gpu.capi.PointCloud(len(want[0]), w * h, cases.CELL, cases.MAX_DEPTH)
    assert _add_all(pc, frames, K) == [(w - 2) * (h - 2)] * 3
    assert same_cloud(pc.download(), want)


def test_overflow_is_sticky_until_reset(gpu, tmp_path):
    capi = gpu.capi
    case = {c["name"]: c for c in CASES}["distinct"]
    frames, K = case["frames"], case["Kinv"]
    want = expected(("case", "distinct"), frames, K, case["cell"], case["max_depth"])
    n = len(want[0])
    h, w = frames[0][0].shape
    pc = capi.PointCloud(n - 1, w * h, case["cell"], case["max_depth"])
    live = _live(capi)
    assert pc.add_frame(_dev(frames[0][0]), _dev(frames[0][1]), K, frames[0][2]) == n // 2
    with pytest.raises(capi.BFError, match="overflowed.*%d points" % (n - 1)):
        pc.add_frame(_dev(frames[1][0]), _dev(frames[1][1]), K, frames[1][2])
    for call in (pc.view, pc.download, lambda: pc.save(tmp_path / "no.ply"), lambda: pc.add_frame(_dev(frames[0][0]), _dev(frames[0][1]), K, frames[0][2])):
        with pytest.raises(capi.BFError, match="overflowed"):
            call()
        assert _live(capi)[:4] == live[:4]
    assert not (tmp_path / "no.ply").exists()
    pc.reset()
    assert pc.num_points() == 0
    assert pc.add_frame(_dev(frames[1][0]), _dev(frames[1][1]), K, frames[1][2]) == n // 2
    assert same_cloud(pc.download(), R.build(frames[1:], K, case["cell"], case["max_depth"]))
    assert pc.save(tmp_path / "yes.ply") == n // 2
    assert (tmp_path / "yes.ply").read_bytes() == R.ply_bytes(*pc.download())
    assert _live(capi)[:4] == live[:4] and _live(capi)[5] == 0
    # a frame larger than maxFramePixels is refused, and that is not an overflow
    big = np.ones((h + 1, w), np.float32)
    with pytest.raises(capi.BFError, match="maxFramePixels"):
        pc.add_frame(_dev(big), _dev(np.ones((h + 1, w, 4), np.uint8)), K, frames[0][2])
    assert pc.num_points() == n // 2


@pytest.mark.parametrize("cell", [cases.CELL, 0.0])
def test_every_acquisition_of_create_fails_in_turn(gpu, cell):
    capi = gpu.capi
    params = capi.PointCloudParams(1000, 640 * 480, cell, 3.5)

    def create():
        h = C.c_void_p()
        return capi.lib.bf_point_cloud_create(C.byref(params), C.byref(h)), h

    before = _live(capi)
    status, h = create()
    assert status == 0 and h.value
    N = _live(capi)[4] - before[4]
    assert N == (8 if cell > 0 else 7)
    assert capi.lib.bf_point_cloud_destroy(h) == 0
    assert _live(capi)[:4] == before[:4]
    for n in range(1, N + 1):
        capi.debug_fail_acquire(n)
        status, h = create()
        message = capi.lib.bf_last_error()
        capi.debug_fail_acquire(0)
        assert status != 0 and not h.value, n
        assert b"injected" in message, (n, message)
        assert _live(capi)[:4] == before[:4], n
    status, h = create()
    assert status == 0 and h.value
    assert capi.lib.bf_point_cloud_destroy(h) == 0
    assert _live(capi)[:4] == before[:4] and _live(capi)[5] == 0


# --------------------------------------------------------------------------- the frame loop
_plain = {}


def _loop(gpu, n, gc, timings, tmp_path=None):
    """the 25-frame configuration of tests/test_render_gpu.py::_run_pipeline; with tmp_path the run saves the point cloud after frame 12 and after the last frame"""
    import torch
    from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix, sensor_desc
    from tests.test_render_gpu import PH, PW, _stream
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
    saved = {}
    for k, (d, c, T, _) in enumerate(frames):
        assert gp.process_frame(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda())
        if tmp_path is not None and k == 12:
            saved["mid"] = (gp.save_point_cloud(tmp_path / "mid.ply", 1), gp.optimized_trajectory().copy())
    if tmp_path is not None:
        saved["one"] = (gp.save_point_cloud(tmp_path / "one.ply", 1), gp.optimized_trajectory().copy())
        saved["key"] = (gp.save_point_cloud(tmp_path / "key.ply"), gp.optimized_trajectory().copy())
    gp.synchronize()
    return gp, gbs, saved


def _host_file(gpu, gp, T, stride, path):
    capi = gpu.capi
    im = C.c_void_p(); Kinv = (C.c_float * 16)()
    capi.check(capi.lib.bf_pipeline_get_image_manager(gp._h, C.byref(im)))
    capi.check(capi.lib.bf_image_manager_get_depth_intrinsics(im, None, Kinv))
    idx = [f for f in range(0, len(T), stride) if not R.pose_invalid(T[f])]
    ds, cs = zip(*[gp.integrate_frame_cpu(f) for f in idx]) if idx else ((), ())          # (no optimised pose yet: the empty cloud, a header and nothing else)
    pos, nrm, col, n = capi.point_cloud_build_host(ds, cs, T[idx].reshape(-1, 4, 4), np.array(list(Kinv), np.float32).reshape(4, 4), 0.005, 3.5)
    capi.write_ply_points(path, pos, nrm, col)
    return n, len(idx)


@pytest.mark.parametrize("gc,timings", [(True, False), (False, False), (True, True)])
def test_saving_from_the_frame_loop_leaves_the_reconstruction_alone(gpu, tmp_path, gc, timings):
    from tests.test_render_gpu import _volume_state
    n = 25
    plain, _, _ = _loop(gpu, n, gc, timings)
    a = _volume_state(plain)
    plain.close()
    gp, gbs, saved = _loop(gpu, n, gc, timings, tmp_path)
    b = _volume_state(gp)
    assert np.array_equal(a["traj"].view(np.uint32), b["traj"].view(np.uint32)) and np.array_equal(a["opt"].view(np.uint32), b["opt"].view(np.uint32))
    assert a["dbg"] == b["dbg"] and a["heap_free"] == b["heap_free"] and a["blocks"] == b["blocks"] and a["counters"] == b["counters"]
    assert np.array_equal(saved["one"][1].view(np.uint32), b["opt"].view(np.uint32))
    for name, stride in (("mid", 1), ("one", 1), ("key", int(gbs.s_submapSize))):
        (points, used), T = saved[name]
        want_points, want_used = _host_file(gpu, gp, T, stride, tmp_path / ("host_" + name + ".ply"))
        assert (points, used) == (want_points, want_used), name
        if name != "mid":          # (after frame 12 the first chunk may not have an optimised pose yet)
            assert used >= 1 and points > 1000, name
        assert (tmp_path / (name + ".ply")).read_bytes() == (tmp_path / ("host_" + name + ".ply")).read_bytes(), name
    assert saved["mid"][0][1] <= 13 and saved["one"][0][1] > saved["key"][0][1]
