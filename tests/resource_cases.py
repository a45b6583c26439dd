"""Every create / open entry of the C ABI at the smallest configuration it accepts, for tests/test_resources_cpu.py and tests/test_resources_gpu.py: a case is
(name, needs, create) where create(ctx) -> (status, handle, destroy) calls the entry through ctypes and ctx holds the handles some creates build on (an image
manager for the bundlers, a pipeline for a pinned player / recorder)."""
import ctypes as C

import numpy as np

from bundlefusion_amd import sensordata as sdm
from bundlefusion_amd import synth
from bundlefusion_amd.capi import (lib, MarchingCubesParams, RayCastParams, default_app_state, default_bundling_state, default_hash_params,
                                   default_solver_config, intrinsics_matrix, sensor_desc, SDF_BLOCK_SIZE, HASH_BUCKET_SIZE, _ALL_GATHER_FN)

W, H = 128, 96                      # the detector takes no image below 64 x 64 or off a multiple of 8
MAX_IMAGES, SUBMAP, MAX_KEYS = 3, 2, 16
BUCKETS, BLOCKS, VOXEL = 1009, 64, 0.02


def params():
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = W, H
    gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks, gas.s_SDFVoxelSize = BUCKETS, BLOCKS, VOXEL
    gas.s_rayCastWidth, gas.s_rayCastHeight = W, H
    gbs.s_widthSIFT, gbs.s_heightSIFT = W, H
    gbs.s_maxNumImages, gbs.s_submapSize, gbs.s_maxNumKeysPerImage = MAX_IMAGES, SUBMAP, MAX_KEYS
    return gas, gbs


def sensor():
    k = synth.intrinsics(W, H)
    return sensor_desc(W, H, intrinsics_matrix(k["fx"], k["fy"], k["mx"], k["my"]))


def sens_info():
    """the header of a recording of W x H frames (JPEG colour)"""
    info = sdm.SensorDataInfo()
    info.versionNumber = 4
    info.sensorName = b"synthetic"
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
    info.depthIntrinsic = info.colorIntrinsic = info.depthExtrinsic = info.colorExtrinsic = eye
    info.depthWidth, info.depthHeight, info.colorWidth, info.colorHeight = W, H, W, H
    info.depthShift = 1000.0
    info.depthCompressionType, info.colorCompressionType = sdm.DEPTH_ZLIB_USHORT, sdm.COLOR_JPEG
    return info


def write_sens(path, frames=2):
    """a small .sens file, by the writer tools/make_sens.py uses"""
    k = synth.intrinsics(W, H)
    K4 = np.eye(4, dtype=np.float32); K4[0, 0], K4[1, 1], K4[0, 2], K4[1, 2] = k["fx"], k["fy"], k["mx"], k["my"]
    rgb = np.zeros((H, W, 3), np.uint8); rgb[::2] = 200
    with sdm.SensorDataWriter(path, (W, H), (W, H), K4, depth_shift=1000.0, color_compression=sdm.COLOR_JPEG) as wr:
        for i in range(frames):
            wr.add_frame(np.eye(4, dtype=np.float32), np.full((H, W), 1000 + i, np.uint16), sdm.encode_jpeg_rgb(rgb, 90))
    return path


def _made(rc, h, destroy):
    return rc, h, (lambda: destroy(h))


def _image_manager(ctx, store=1):
    gas, gbs = params(); s = sensor(); h = C.c_void_p()
    return _made(lib.bf_image_manager_create(W, H, W, H, C.byref(s), C.byref(gbs), store, C.byref(h)), h, lib.bf_image_manager_destroy)


def _scene(ctx):
    p = default_hash_params(num_buckets=BUCKETS, num_sdf_blocks=BLOCKS, voxel_size=VOXEL); h = C.c_void_p()
    return _made(lib.bf_scene_create(C.byref(p), C.byref(h)), h, lib.bf_scene_destroy)


def _solver(ctx):
    cfg = default_solver_config(); h = C.c_void_p()
    return _made(lib.bf_solver_create(2, 25, C.byref(cfg), C.byref(h)), h, lib.bf_solver_destroy)


def _sift(ctx):
    h = C.c_void_p()
    return _made(lib.bf_sift_create(W, H, W, H, 150, C.c_float(0.1), C.c_float(4.0), C.c_float(3.0), MAX_KEYS, C.byref(h)), h, lib.bf_sift_destroy)


def _siftmgr(ctx):
    h = C.c_void_p()
    return _made(lib.bf_siftmgr_create(MAX_IMAGES, MAX_KEYS, C.byref(h)), h, lib.bf_siftmgr_destroy)


def _cache(ctx):
    k = synth.intrinsics(W, H); K = (C.c_float * 16)(*np.asarray(intrinsics_matrix(k["fx"], k["fy"], k["mx"], k["my"]), np.float32).reshape(16)); h = C.c_void_p()
    return _made(lib.bf_cache_create(W, H, 32, 24, MAX_IMAGES, K, C.c_float(2.5), C.c_float(1.0), C.c_float(0.05), C.byref(h)), h, lib.bf_cache_destroy)


def _calibrator(ctx):
    h = C.c_void_p()
    return _made(lib.bf_image_calibrator_create(W, H, C.byref(h)), h, lib.bf_image_calibrator_destroy)


def _marching_cubes(ctx, max_triangles=1000):
    p = MarchingCubesParams(max_triangles, SDF_BLOCK_SIZE, BUCKETS, HASH_BUCKET_SIZE, 10 * VOXEL, 10 * VOXEL); h = C.c_void_p()
    return _made(lib.bf_marching_cubes_create(C.byref(p), C.byref(h)), h, lib.bf_marching_cubes_destroy)


def _ray_cast(ctx):
    p = RayCastParams(); p.m_width, p.m_height = W, H; h = C.c_void_p()
    return _made(lib.bf_ray_cast_create(C.byref(p), C.byref(h)), h, lib.bf_ray_cast_destroy)


def _frame_renderer(ctx):
    h = C.c_void_p()
    return _made(lib.bf_frame_renderer_create(W, H, C.byref(h)), h, lib.bf_frame_renderer_destroy)


def _bundler(ctx):
    gas, gbs = params(); eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16)); h = C.c_void_p()
    return _made(lib.bf_bundler_create(SUBMAP + 1, MAX_KEYS, eye, ctx["im"], 1, C.byref(gas), C.byref(gbs), C.byref(h)), h, lib.bf_bundler_destroy)


def _online_bundler(ctx):
    gas, gbs = params(); s = sensor(); h = C.c_void_p()
    return _made(lib.bf_online_bundler_create(C.byref(s), ctx["im"], C.byref(gas), C.byref(gbs), C.byref(h)), h, lib.bf_online_bundler_destroy)


def _pipeline(ctx):
    gas, gbs = params(); s = sensor(); h = C.c_void_p()
    return _made(lib.bf_pipeline_create(C.byref(gas), C.byref(gbs), C.byref(s), C.byref(h)), h, lib.bf_pipeline_destroy)


def _chunk_worker(ctx):
    gas, gbs = params(); s = sensor(); h = C.c_void_p()
    return _made(lib.bf_chunk_worker_create(C.byref(gas), C.byref(gbs), C.byref(s), C.byref(h)), h, lib.bf_chunk_worker_destroy)


def _sens_player(ctx):
    h = C.c_void_p()
    return _made(lib.bf_sens_player_create(ctx["pipeline"], ctx["sd"], 1, C.byref(h)), h, lib.bf_sens_player_destroy)


def _sens_recorder(ctx):
    info = sens_info(); h = C.c_void_p()
    return _made(lib.bf_sens_recorder_create(ctx["pipeline"], C.byref(info), str(ctx["tmp"] / "rec.tmp.sens").encode(), 1, 2, C.byref(h)), h, lib.bf_sens_recorder_destroy)


def _evaluator(ctx):
    t = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (4, 1)); h = C.c_void_p()
    return _made(lib.bf_correspondence_evaluator_create(t.ctypes.data_as(C.POINTER(C.c_float)), 4, b"", C.byref(h)), h, lib.bf_correspondence_evaluator_destroy)


def _trajectory_manager(ctx):
    h = C.c_void_p()
    return _made(lib.bf_trajectory_manager_create(MAX_IMAGES * SUBMAP, 30, C.c_float(0.0), C.byref(h)), h, lib.bf_trajectory_manager_destroy)


def _sensor_data(ctx):
    h = C.c_void_p()
    return _made(lib.bf_sensor_data_open(str(ctx["sens"]).encode(), C.byref(h)), h, lib.bf_sensor_data_close)


def _sensor_data_writer(ctx):
    info = sens_info(); h = C.c_void_p()
    return _made(lib.bf_sensor_data_writer_create(str(ctx["tmp"] / "w.sens").encode(), C.byref(info), C.byref(h)), h, lib.bf_sensor_data_writer_close)


_CB = _ALL_GATHER_FN(lambda user, send, recv, nbytes, stream: 0)


def _comm_callback(ctx):
    h = C.c_void_p()
    return _made(lib.bf_comm_create_callback(_CB, None, 2, 0, C.byref(h)), h, lib.bf_comm_destroy)


# the creates that take something from the device; needs: what of ctx they build on
DEVICE_CASES = [
    ("image_manager", (), _image_manager), ("image_manager_host_frames", (), lambda ctx: _image_manager(ctx, 0)), ("scene", (), _scene), ("solver", (), _solver),
    ("sift", (), _sift), ("siftmgr", (), _siftmgr), ("cache", (), _cache), ("image_calibrator", (), _calibrator), ("marching_cubes", (), _marching_cubes),
    ("ray_cast", (), _ray_cast), ("frame_renderer", (), _frame_renderer), ("bundler", ("im",), _bundler), ("online_bundler", ("im",), _online_bundler),
    ("pipeline", (), _pipeline), ("chunk_worker", (), _chunk_worker), ("sens_player", ("pipeline", "sd"), _sens_player), ("sens_recorder", ("pipeline",), _sens_recorder),
]
# ... and those that need no device
HOST_CASES = [("trajectory_manager", (), _trajectory_manager), ("sensor_data", (), _sensor_data), ("sensor_data_writer", (), _sensor_data_writer),
              ("comm_callback", (), _comm_callback), ("correspondence_evaluator", (), _evaluator)]
