"""GPU tests (-m gpu) of the ownership of device resources (csrc/bf_resources.h) through bf_debug_live_resources and bf_debug_fail_acquire: every handle type is
used once so that its grow paths run and leaves nothing behind; every acquisition of every create, failed in turn, unwinds the create completely; a failed
re-allocation in a grow path leaves an object that the next call repairs.  The counters are this process's own (other processes share the card)."""
import ctypes as C
import gc

import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import BFError, camera_params, default_app_state, default_bundling_state, default_hash_params, intrinsics_matrix, sensor_desc
from tests import resource_cases as rc

pytestmark = pytest.mark.gpu

VW, VH, VOXEL, VBUCKETS, VBLOCKS = 160, 120, 0.02, 1009, 4000      # the planted volumes' frame size (tests/volume_cases.py); one frame of the room takes < 300 blocks


class _Baseline:
    """fields 1-4 of bf_debug_live_resources are back where they were at the end of the block, and no release has failed"""

    def __init__(self, capi):
        self.capi = capi

    def __enter__(self):
        gc.collect()                                    # handles an earlier test left to the collector go now, not inside the block
        self.before = self.capi.debug_live_resources()
        return self

    def check(self, what=""):
        now = self.capi.debug_live_resources()
        assert now[:4] == self.before[:4], (what, self.before, now)
        assert now[5] == 0, what

    def __exit__(self, et, ev, tb):
        if et is None:
            self.check("at the end")
        return False


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def room():
    """one frame of the synthetic room at the planted volumes' size, and its camera"""
    d, c, T, K = synth.scene_room(0, VW, VH)
    return d, c, T, camera_params(VW, VH, K["fx"], K["fy"], K["mx"], K["my"])


def _scene_with_room(gpu, room):
    import torch
    d, c, T, cam = room
    sc = gpu.capi.SceneRepHashSDF(default_hash_params(num_buckets=VBUCKETS, num_sdf_blocks=VBLOCKS, voxel_size=VOXEL))
    sc.set_arith("fast")
    sc.integrate(T, _dev(d), _dev(c), cam)              # fast contract, no caller texels: the scene grows its own texel buffers
    torch.cuda.synchronize()
    return sc


def _raw_frames():
    """two frames in sensor format: raw RGB8, then a JPEG (the device takes its coefficients: larger upload and sample planes than any frame before)"""
    from bundlefusion_amd import sensordata as sdm
    rng = np.random.default_rng(5)
    out = []
    for k in range(2):
        d = np.full((rc.H, rc.W), 1000 + 50 * k, np.uint16); d[::7, ::5] = 0
        rgb = rng.integers(0, 256, (rc.H // 8, rc.W // 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)
        out.append((d, rgb.tobytes(), sdm.COLOR_RAW) if k == 0 else (d, sdm.encode_jpeg_rgb(rgb, 92), sdm.COLOR_JPEG))
    return out


def _image_manager(gpu):
    gas, gbs = rc.params()
    return gpu.capi.ImageManager(gas, gbs, rc.sensor(), 1)


# ------------------------------------------------------------------------------------------------ 1: round trips
def test_round_trip_image_manager(gpu):
    with _Baseline(gpu.capi):
        im = _image_manager(gpu)
        for d, blob, comp in _raw_frames():
            assert im.process_raw(d, 1000.0, blob, comp)
        assert im.num_frames() == 2
        im.close()


def test_round_trip_scene_marching_cubes_and_weld(gpu, room):
    with _Baseline(gpu.capi):
        sc = _scene_with_room(gpu, room)
        mc = gpu.capi.MarchingCubesHashSDF(0, VBUCKETS, VOXEL)          # m_maxNumTriangles = 0: the triangle buffer is sized by the extraction
        n, found = mc.extract_gpu(sc)
        assert n == found > 0
        pos, col, faces = mc.weld()
        assert len(faces) > 0 and len(pos) > 0
        mc.close(); sc.close()


def test_round_trip_evaluator(gpu):
    from bundlefusion_amd.capi import CorrespondenceEvaluator
    from tests.test_match_gpu import _chunk
    import torch
    with _Baseline(gpu.capi):
        n = 3
        frames, K, sift, mgr, cache = _chunk(gpu, n, 12, first=20)
        T0inv = np.linalg.inv(frames[0][2].astype(np.float64))
        ev = CorrespondenceEvaluator(np.stack([(T0inv @ f[2].astype(np.float64)).astype(np.float32) for f in frames]), None)
        for k in range(n - 1):
            mgr.set_valid_image(k, 1)
        mgr.update_gpu_valid_images()
        mgr.set_current_frame(n - 1)
        mgr.match(n - 1, 0, n)
        a0 = gpu.capi.debug_live_resources()[4]
        ev.evaluate(mgr, cache, np.linalg.inv(np.asarray(K, np.float64).reshape(4, 4)).astype(np.float32), False, True, False, "raw")
        assert gpu.capi.debug_live_resources()[4] - a0 == 2             # the evaluator's two scratch buffers grew from nothing
        torch.cuda.synchronize()
        ev.close(); sift.close(); mgr.close(); cache.close()


def test_round_trip_pipeline_frame_render_and_mesh(gpu, tmp_path):
    W, H = 640, 480
    frames = synth.render_frames(range(2))
    Kd = frames[0][3]
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = W, H
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.02, 50000, 20000
    gbs.s_maxNumImages, gbs.s_submapSize = 3, 2          # (the key-point cap stays: a real frame has more than 16, which the frame loop reports as an error)
    with _Baseline(gpu.capi):
        gp = gpu.capi.Pipeline(gas, gbs, sensor_desc(W, H, intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])))
        for d, c, _, _ in frames:
            assert gp.process_frame(d, c)
        gp.synchronize()
        pic = gp.render(1)
        assert pic.shape == (gas.s_rayCastHeight, gas.s_rayCastWidth, 4) and pic.any()
        nv, nf, nt = gp.save_mesh(tmp_path / "scan.ply")
        assert nv > 0 and nf > 0 and nt >= nf
        gp.close()


@pytest.mark.parametrize("case", rc.HOST_CASES + [c for c in rc.DEVICE_CASES if not c[1]], ids=lambda c: c[0])
def test_round_trip_create_destroy(gpu, tmp_path, case):
    """every other type (and the ones above once more, at the small configuration): create, destroy, nothing left"""
    name, _, create = case
    ctx = {"tmp": tmp_path, "sens": rc.write_sens(tmp_path / "small.sens")}
    with _Baseline(gpu.capi):
        status, h, destroy = create(ctx)
        assert status == 0 and h.value, (name, gpu.capi.lib.bf_last_error())
        assert destroy() == 0


# ------------------------------------------------------------------------------------------------ 2: every acquisition of every create fails in turn
def _which(N):
    """1..N, or - a composite handle - 1..32 and 32 values evenly spaced up to and including N"""
    if N <= 64:
        return list(range(1, N + 1))
    return sorted(set(range(1, 33)) | {32 + ((N - 32) * k + 31) // 32 for k in range(1, 33)})


@pytest.fixture()
def ctx(gpu, tmp_path):
    """what some creates build on: an image manager, a pipeline, an open .sens file"""
    lib = gpu.capi.lib
    c = {"tmp": tmp_path, "sens": rc.write_sens(tmp_path / "small.sens")}
    made = []
    for key, create in (("im", rc._image_manager), ("pipeline", rc._pipeline), ("sd", rc._sensor_data)):
        status, h, destroy = create(c)
        assert status == 0, (key, lib.bf_last_error())
        c[key] = h
        made.append(destroy)
    yield c
    for destroy in reversed(made):
        destroy()


@pytest.mark.parametrize("case", rc.DEVICE_CASES, ids=[c[0] for c in rc.DEVICE_CASES])
def test_injected_failure_in_create_unwinds_completely(gpu, ctx, case):
    capi = gpu.capi
    name, _, create = case
    with _Baseline(capi) as base:
        a0 = capi.debug_live_resources()[4]
        status, h, destroy = create(ctx)
        assert status == 0, (name, capi.lib.bf_last_error())
        N = capi.debug_live_resources()[4] - a0
        assert destroy() == 0
        base.check("after the counting create")
        assert N >= 1, name
        tried = _which(N)
        assert tried[0] == 1 and tried[-1] == N and len(tried) <= 64
        for n in tried:
            capi.debug_fail_acquire(n)
            status, h, _ = create(ctx)
            message = capi.lib.bf_last_error()
            capi.debug_fail_acquire(0)
            assert status != 0 and not h.value, (name, n, N)
            assert b"injected" in message, (name, n, message)
            base.check("%s, acquisition %d of %d failed" % (name, n, N))
        status, h, destroy = create(ctx)
        assert status == 0 and h.value, (name, capi.lib.bf_last_error())
        assert destroy() == 0


# ------------------------------------------------------------------------------------------------ 3: a failure in a grow path
def test_injected_failure_in_marching_cubes_grow_paths(gpu, room):
    """the three re-allocations of the slot buffers and the regrow of the triangle buffer (acquisitions 1-4 of the first extraction): the call fails, the next
    one succeeds with the untouched object's triangle count"""
    capi = gpu.capi
    with _Baseline(capi):
        sc = _scene_with_room(gpu, room)
        ref = capi.MarchingCubesHashSDF(0, VBUCKETS, VOXEL)
        a0 = capi.debug_live_resources()[4]
        want = ref.extract_gpu(sc)
        assert capi.debug_live_resources()[4] - a0 == 4 and want[0] == want[1] > 0
        ref.close()
        for n in (1, 2, 3, 4):
            mc = capi.MarchingCubesHashSDF(0, VBUCKETS, VOXEL)
            capi.debug_fail_acquire(n)
            with pytest.raises(BFError, match="injected"):
                mc.extract_gpu(sc)
            capi.debug_fail_acquire(0)
            assert mc.extract_gpu(sc) == want, n
            assert len(mc.weld()[2]) > 0
            mc.close()
        sc.close()


def test_injected_failure_in_image_manager_raw_grow_paths(gpu):
    """the second, larger frame grows the sensor-format ingest's buffers (rawEnsure, rawSlot): each of its acquisitions failed in turn, then the frame goes in and
    is stored as in an untouched manager"""
    capi = gpu.capi
    first, second = _raw_frames()
    with _Baseline(capi):
        ref = _image_manager(gpu)
        assert ref.process_raw(first[0], 1000.0, first[1], first[2])
        a0 = capi.debug_live_resources()[4]
        assert ref.process_raw(second[0], 1000.0, second[1], second[2])
        N = capi.debug_live_resources()[4] - a0
        assert N >= 2                                                    # the sample planes and the slot's pinned colour buffer at least
        want = ref.get_integrate_frame_cpu(1)
        ref.close()
        for n in range(1, N + 1):
            im = _image_manager(gpu)
            assert im.process_raw(first[0], 1000.0, first[1], first[2])
            capi.debug_fail_acquire(n)
            with pytest.raises(BFError, match="injected"):
                im.process_raw(second[0], 1000.0, second[1], second[2])
            capi.debug_fail_acquire(0)
            assert im.num_frames() == 1
            assert im.process_raw(second[0], 1000.0, second[1], second[2]) and im.num_frames() == 2
            got = im.get_integrate_frame_cpu(1)
            assert np.array_equal(got[0].view(np.uint8), want[0].view(np.uint8)) and np.array_equal(got[1], want[1]), n
            im.close()
