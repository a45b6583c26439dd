"""ctypes bindings of include/bf_hip.h (the C ABI of libbf_hip.so)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BF_LIB_PATH") or os.path.join(_HERE, "lib", "libbf_hip.so")      # BF_LIB_PATH: a variant build of the same library (tools/build_variant.py; diagnostics)


class BFError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(
        "bundlefusion_amd: %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(there is no CPU fallback)" % LIB_PATH)

try:
    # PyTorch ships its own libamdhip64/libhsa-runtime64.  Load it FIRST so that libbf_hip.so binds to the same HIP
    # runtime (same soname): two runtimes in one process have independent null streams and no mutual ordering.
    import torch  # noqa: F401
except ImportError:      # pure C-ABI use without torch is fine: the library then brings /opt/rocm's runtime
    pass
lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)

SDF_BLOCK_SIZE = 8
HASH_BUCKET_SIZE = 4
FREE_ENTRY = -2
VOX_PER_BLOCK = 512


class HashParams(C.Structure):
    _fields_ = [
        ("m_rigidTransform", C.c_float * 16),
        ("m_rigidTransformInverse", C.c_float * 16),
        ("m_hashNumBuckets", C.c_uint32),
        ("m_hashBucketSize", C.c_uint32),
        ("m_hashMaxCollisionLinkedListSize", C.c_uint32),
        ("m_numSDFBlocks", C.c_uint32),
        ("m_SDFBlockSize", C.c_int32),
        ("m_virtualVoxelSize", C.c_float),
        ("m_numOccupiedBlocks", C.c_uint32),
        ("m_maxIntegrationDistance", C.c_float),
        ("m_truncScale", C.c_float),
        ("m_truncation", C.c_float),
        ("m_integrationWeightSample", C.c_uint32),
        ("m_integrationWeightMax", C.c_uint32),
        ("m_streamingVoxelExtents", C.c_float * 3),
        ("m_streamingGridDimensions", C.c_int32 * 3),
        ("m_streamingMinGridPos", C.c_int32 * 3),
        ("m_streamingInitialChunkListSize", C.c_uint32),
        ("m_dummy", C.c_uint32 * 2),
    ]


class DepthCameraParams(C.Structure):
    _fields_ = [
        ("fx", C.c_float), ("fy", C.c_float), ("mx", C.c_float), ("my", C.c_float),
        ("m_imageWidth", C.c_uint32), ("m_imageHeight", C.c_uint32),
        ("m_sensorDepthWorldMin", C.c_float), ("m_sensorDepthWorldMax", C.c_float),
    ]


class DepthCameraData(C.Structure):
    _fields_ = [("d_depthData", C.c_void_p), ("d_colorData", C.c_void_p)]


SCENE_BATCH_MAX = 12
SCENE_OP_INTEGRATE, SCENE_OP_DEINTEGRATE, SCENE_OP_REINTEGRATE = 0, 1, 2      # BF_SCENE_OP_* (bf_hip.h)


class SceneBatchOp(C.Structure):
    """bf_scene_batch_op: kind 0 integrate(T0), 1 deIntegrate(T0), 2 deIntegrate(T0) + integrate(T1) of the same frame"""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("T0", C.c_float * 16), ("T1", C.c_float * 16), ("data", DepthCameraData),
                ("d_texels", C.c_void_p), ("wait_event", C.c_void_p)]


class HashData(C.Structure):
    _fields_ = [
        ("d_heap", C.c_void_p), ("d_heapCounter", C.c_void_p), ("d_hashDecision", C.c_void_p),
        ("d_hashDecisionPrefix", C.c_void_p), ("d_hash", C.c_void_p), ("d_hashCompactified", C.c_void_p),
        ("d_hashCompactifiedCounter", C.c_void_p), ("d_SDFBlocks", C.c_void_p), ("d_hashBucketMutex", C.c_void_p),
    ]


HASH_ENTRY_DTYPE = np.dtype([("pos", "<i4", 3), ("ptr", "<i4"), ("offset", "<u4"), ("_pad", "<u4", 3)])
VOXEL_DTYPE = np.dtype([("sdf", "<f4"), ("weight", "<f4"), ("color", "u1", 4)])
assert HASH_ENTRY_DTYPE.itemsize == 32 and VOXEL_DTYPE.itemsize == 12

lib.bf_last_error.restype = C.c_char_p


def bind_host_threads_to_device(device=0):
    """bf_bind_host_threads_to_device: all threads of this process onto the CPUs of the GPU's NUMA node; returns the cpu list ('' = unchanged)."""
    buf = C.create_string_buffer(1024)
    lib.bf_bind_host_threads_to_device(int(device), buf, C.c_size_t(len(buf)))
    return buf.value.decode()


lib.bf_version.restype = C.c_char_p


def check(rc):
    if rc != 0:
        raise BFError("libbf_hip status %d: %s" % (rc, lib.bf_last_error().decode()))


def debug_live_resources():
    """bf_debug_live_resources: (live owners, live device allocations, live device bytes, live pinned allocations + events + streams, acquisitions so far,
    failed releases) of this process"""
    out = (C.c_uint64 * 6)()
    check(lib.bf_debug_live_resources(out))
    return tuple(int(v) for v in out)


def debug_fail_acquire(nth):
    """bf_debug_fail_acquire: the nth acquisition from now on fails as out-of-memory, once (0: off)"""
    check(lib.bf_debug_fail_acquire(C.c_uint64(int(nth))))


def mat16(m):
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(16))
    return (C.c_float * 16)(*a.tolist())


def default_hash_params(num_buckets=800000, num_sdf_blocks=200000, voxel_size=0.010, max_integration_distance=3.0,
                        truncation=0.06, trunc_scale=0.02, weight_sample=1, weight_max=99999999, max_chain=7):
    """CUDASceneRepHashSDF::parametersFromGlobalAppState with zParametersDefault.txt values."""
    p = HashParams()
    eye = np.eye(4, dtype=np.float32).reshape(16)
    p.m_rigidTransform[:] = eye.tolist()
    p.m_rigidTransformInverse[:] = eye.tolist()
    p.m_hashNumBuckets = num_buckets
    p.m_hashBucketSize = HASH_BUCKET_SIZE
    p.m_hashMaxCollisionLinkedListSize = max_chain
    p.m_numSDFBlocks = num_sdf_blocks
    p.m_SDFBlockSize = SDF_BLOCK_SIZE
    p.m_virtualVoxelSize = voxel_size
    p.m_numOccupiedBlocks = 0
    p.m_maxIntegrationDistance = max_integration_distance
    p.m_truncScale = trunc_scale
    p.m_truncation = truncation
    p.m_integrationWeightSample = weight_sample
    p.m_integrationWeightMax = weight_max
    p.m_streamingVoxelExtents[:] = [1.0, 1.0, 1.0]
    p.m_streamingGridDimensions[:] = [257, 257, 257]
    p.m_streamingMinGridPos[:] = [-128, -128, -128]
    p.m_streamingInitialChunkListSize = 2000
    return p


def camera_params(width, height, fx, fy, mx, my, dmin=0.1, dmax=4.0):
    c = DepthCameraParams()
    c.fx, c.fy, c.mx, c.my = fx, fy, mx, my
    c.m_imageWidth, c.m_imageHeight = width, height
    c.m_sensorDepthWorldMin, c.m_sensorDepthWorldMax = dmin, dmax
    return c


def alloc_comm_capacity(W, H, voxel, world):
    """Keys per rank and operator for bf_scene_set_alloc_comm / bf_pipeline_set_comm: twice the estimate of the distinct in-frustum blocks the rays of a W x H frame
    cross (0.22 per pixel at 2 mm, scaling with 1 / voxel^2; tests/test_host_cpu.py holds it against measured key counts), divided over the ranks, as a power of
    two >= 65536."""
    est = 0.22 * W * H * (0.002 / voxel) ** 2
    cap = 1 << 16
    while cap < 2.0 * est / max(world, 1):
        cap <<= 1
    return cap


class SceneRepHashSDF:
    """Python view of `bf_scene` (== the reference's CUDASceneRepHashSDF)."""

    def __init__(self, params, stream=None):
        self._h = C.c_void_p()
        self.params = params
        check(lib.bf_scene_create(C.byref(params), C.byref(self._h)))
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if self._h and not getattr(self, "_borrowed", False):
            lib.bf_scene_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        check(lib.bf_scene_set_stream(self._h, C.c_void_p(stream_ptr)))

    def reset(self):
        check(lib.bf_scene_reset(self._h))

    @staticmethod
    def _data(depth, color):
        d = DepthCameraData()
        d.d_depthData = depth.data_ptr()
        d.d_colorData = color.data_ptr() if color is not None else None
        return d

    def integrate(self, cam_to_world, depth, color, cam):
        d = self._data(depth, color)
        check(lib.bf_scene_integrate(self._h, mat16(cam_to_world), C.byref(d), C.byref(cam), None))

    def deintegrate(self, cam_to_world, depth, color, cam):
        d = self._data(depth, color)
        check(lib.bf_scene_deintegrate(self._h, mat16(cam_to_world), C.byref(d), C.byref(cam), None))

    def set_overlap(self, enable=True):
        check(lib.bf_scene_set_overlap(self._h, int(enable)))

    def set_shard(self, rank, world):
        check(lib.bf_scene_set_shard(self._h, rank, world))

    def set_external_alloc(self, enable=True):
        check(lib.bf_scene_set_external_alloc(self._h, int(enable)))

    def set_alloc_comm(self, comm, capacity_keys=1 << 17):
        """The operators' own allocation with the ray march divided over the ranks of `comm` (capi.Comm or None): bf_scene_set_alloc_comm.  capacity_keys: see
        alloc_comm_capacity(W, H, voxel, world) (the default covers 640x480 @4 mm on one rank four times over)."""
        check(lib.bf_scene_set_alloc_comm(self._h, comm._h if comm is not None else None, int(capacity_keys)))
        self._alloc_comm = comm          # keep the callback alive

    def alloc_collect(self, cam_to_world, depth, cam, part, parts, keys, slots, count):
        """keys: torch int64 [capacity] cuda, slots: int32 [capacity], count: int32 [1] (see bf_scene_alloc_collect)"""
        d = self._data(depth, None)
        check(lib.bf_scene_alloc_collect(self._h, mat16(cam_to_world), C.byref(d), C.byref(cam), int(part), int(parts), C.c_void_p(keys.data_ptr()),
                                         C.c_void_p(slots.data_ptr()), C.c_void_p(count.data_ptr()), int(keys.numel())))

    def alloc_ingest(self, keys, count):
        check(lib.bf_scene_alloc_ingest(self._h, C.c_void_p(keys.data_ptr()), C.c_void_p(count.data_ptr()), int(keys.numel())))

    def alloc_place(self):
        check(lib.bf_scene_alloc_place(self._h))

    def alloc_sync(self):
        check(lib.bf_scene_alloc_sync(self._h))

    def set_arith(self, mode):
        """'fast' (the reference GPU build's -use_fast_math contract; library default) or 'exact' (IEEE op by op, bit-comparable with the oracle): bf_scene_set_arith"""
        check(lib.bf_scene_set_arith(self._h, {"exact": 0, "fast": 1}[mode]))

    def arith(self):
        m = C.c_int()
        check(lib.bf_scene_get_arith(self._h, C.byref(m)))
        return ("exact", "fast")[m.value]

    def reintegrate(self, old_cam_to_world, new_cam_to_world, depth, color, cam):
        """fused deintegrate(old) + integrate(new) of the same frame"""
        data = self._data(depth, color)
        check(lib.bf_scene_reintegrate(self._h, mat16(old_cam_to_world), mat16(new_cam_to_world), C.byref(data), C.byref(cam)))

    def run_batch(self, ops, cam):
        """ops: list of (kind, T0, T1 or None, depth, color) - kind "in" / 0 integrate(T0), "de" / 1 deIntegrate(T0), "re" / 2 deIntegrate(T0) + integrate(T1) -
        executed as ONE batch (bf_scene_run_batch): same volume as the same operators issued one by one, in that order."""
        assert 1 <= len(ops) <= SCENE_BATCH_MAX
        arr = (SceneBatchOp * len(ops))()
        for o, (kind, T0, T1, depth, color) in zip(arr, ops):
            o.kind = {"in": SCENE_OP_INTEGRATE, "de": SCENE_OP_DEINTEGRATE, "re": SCENE_OP_REINTEGRATE}.get(kind, kind)
            o.T0[:] = np.asarray(T0, np.float32).reshape(16).tolist()
            o.T1[:] = np.asarray(T1 if T1 is not None else T0, np.float32).reshape(16).tolist()
            o.data = self._data(depth, color)
            o.d_texels = None; o.wait_event = None
        check(lib.bf_scene_run_batch(self._h, arr, len(ops), C.byref(cam)))

    def garbage_collect(self):
        check(lib.bf_scene_garbage_collect(self._h))

    def compactify(self, cam_to_world, cam):
        check(lib.bf_scene_set_last_rigid_transform_and_compactify(self._h, mat16(cam_to_world), C.byref(cam)))

    def hash_data(self):
        hd = HashData()
        check(lib.bf_scene_get_hash_data(self._h, C.byref(hd)))
        return hd

    def hash_params(self):
        p = HashParams()
        check(lib.bf_scene_get_hash_params(self._h, C.byref(p)))
        return p

    def heap_free_count(self):
        v = C.c_uint32()
        check(lib.bf_scene_get_heap_free_count(self._h, C.byref(v)))
        return v.value

    def num_allocated_blocks(self):
        v = C.c_uint32()
        check(lib.bf_scene_get_num_allocated_blocks(self._h, C.byref(v)))
        return v.value

    def num_integrated_frames(self):
        v = C.c_uint32()
        check(lib.bf_scene_get_num_integrated_frames(self._h, C.byref(v)))
        return v.value

    def debug_hash(self):
        out = (C.c_uint32 * 6)()
        check(lib.bf_scene_debug_hash(self._h, out))
        return dict(occupied=out[0], heap_free=out[1], duplicate_keys=out[2], free_and_allocated=out[3], leaked=out[4],
                    dropped=out[5])

    def find_blocks(self, pos):
        """pos: torch int32 [n, 3] cuda (block coordinates) -> torch int32 [n]: ptr or FREE_ENTRY (bf_scene_debug_find_blocks)"""
        import torch
        out = torch.empty(pos.shape[0], dtype=torch.int32, device=pos.device)
        check(lib.bf_scene_debug_find_blocks(self._h, C.c_void_p(pos.data_ptr()), int(pos.shape[0]), C.c_void_p(out.data_ptr())))
        return out

    def kernel_timing(self, enable):
        check(lib.bf_scene_kernel_timing(self._h, int(enable)))

    def kernel_timing_read(self):
        n, ms = C.c_uint32(), C.c_float()
        check(lib.bf_scene_kernel_timing_read(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def kernel_timing_occupied(self):
        v = C.c_uint64(); n = C.c_uint32()
        check(lib.bf_scene_kernel_timing_occupied(self._h, C.byref(v), C.byref(n)))
        return v.value, n.value

    def kernel_timing_blocks(self):
        """(operator blocks [a fused launch counts both lists], blocks visited by plain launches, blocks visited by fused launches [union list], #operators)"""
        a = C.c_uint64(); b = C.c_uint64(); c = C.c_uint64(); n = C.c_uint32()
        check(lib.bf_scene_kernel_timing_blocks(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return a.value, b.value, c.value, n.value

    def kernel_timing_images(self):
        """frames (depth + colour images) the timed launches sampled: one per operator, n per batch of n"""
        n = C.c_uint32()
        check(lib.bf_scene_kernel_timing_images(self._h, C.byref(n)))
        return n.value

    # ---- test helpers: copy raw arrays back (hipMemcpy through torch) ----
    def download(self):
        """Returns (hash[numBuckets*4], heap[numSDFBlocks], heapCounter, voxels[numSDFBlocks*512]) as numpy."""
        import torch
        torch.cuda.synchronize()
        hd = self.hash_data()
        nE = self.params.m_hashNumBuckets * HASH_BUCKET_SIZE
        nB = self.params.m_numSDFBlocks
        hash_np = _d2h(hd.d_hash, nE * 32).view(HASH_ENTRY_DTYPE)
        heap_np = _d2h(hd.d_heap, nB * 4).view("<u4")
        heap_counter = int(_d2h(hd.d_heapCounter, 4).view("<u4")[0])
        vox_np = _d2h(hd.d_SDFBlocks, nB * VOX_PER_BLOCK * 12).view(VOXEL_DTYPE)
        return hash_np, heap_np, heap_counter, vox_np

    def download_compactified(self):
        import torch
        torch.cuda.synchronize()
        hd = self.hash_data()
        n = int(_d2h(hd.d_hashCompactifiedCounter, 4).view("<i4")[0])
        return _d2h(hd.d_hashCompactified, n * 32).view(HASH_ENTRY_DTYPE)


_hip = None


def _d2h(ptr, nbytes):
    """D2H of a raw device pointer into a fresh numpy byte array (through the library's own runtime, fenced)."""
    out = np.empty(nbytes, dtype=np.uint8)
    check(lib.bf_memcpy_d2h(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes)))
    return out


# --------------------------------------------------------------------------- cache + solver
class CachedFrame(C.Structure):
    _fields_ = [("d_depthDownsampled", C.c_void_p), ("d_cameraposDownsampled", C.c_void_p), ("d_intensityDownsampled", C.c_void_p),
                ("d_intensityDerivsDownsampled", C.c_void_p), ("d_normalsDownsampledUCHAR4", C.c_void_p),
                ("d_normalsDownsampled", C.c_void_p)]


class SolverConfig(C.Structure):
    _fields_ = [("optMaxResThresh", C.c_float), ("denseDistThresh", C.c_float), ("denseNormalThresh", C.c_float),
                ("denseColorThresh", C.c_float), ("denseColorGradientMin", C.c_float), ("denseDepthMin", C.c_float),
                ("denseDepthMax", C.c_float), ("denseOverlapCheckSubsampleFactor", C.c_uint32), ("verifyOptDistThresh", C.c_float),
                ("verifyOptPercentThresh", C.c_float), ("recordConvergence", C.c_int32)]


ENTRYJ_DTYPE = np.dtype([("imgIdx_i", "<u4"), ("imgIdx_j", "<u4"), ("pos_i", "<f4", 3), ("pos_j", "<f4", 3)])
assert ENTRYJ_DTYPE.itemsize == 32


def default_solver_config(record_convergence=False):
    """zParametersBundlingDefault.txt values."""
    c = SolverConfig()
    c.optMaxResThresh = 0.08
    c.denseDistThresh = 0.15
    c.denseNormalThresh = 0.97
    c.denseColorThresh = 0.1
    c.denseColorGradientMin = 0.005
    c.denseDepthMin = 0.5
    c.denseDepthMax = 4.0
    c.denseOverlapCheckSubsampleFactor = 4
    c.verifyOptDistThresh = 0.02
    c.verifyOptPercentThresh = 0.05
    c.recordConvergence = int(record_convergence)
    return c


def intrinsics_matrix(fx, fy, mx, my):
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, mx, my
    return K


class Cache:
    """Python view of `bf_cache` (== the reference's CUDACache)."""

    def __init__(self, depth_w, depth_h, w, h, max_images, input_intrinsics, color_sigma=2.5, depth_sigma_d=1.0, depth_sigma_r=0.05,
                 stream=None):
        self._h = C.c_void_p()
        self.w, self.h, self.max_images = w, h, max_images
        check(lib.bf_cache_create(depth_w, depth_h, w, h, max_images, mat16(input_intrinsics), C.c_float(color_sigma),
                                  C.c_float(depth_sigma_d), C.c_float(depth_sigma_r), C.byref(self._h)))
        if stream is not None:
            check(lib.bf_cache_set_stream(self._h, C.c_void_p(stream)))

    def close(self):
        if self._h:
            lib.bf_cache_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def store_frame(self, depth, color):
        dh, dw = depth.shape[:2]
        ch, cw = color.shape[:2]
        check(lib.bf_cache_store_frame(self._h, C.c_void_p(depth.data_ptr()), dw, dh, C.c_void_p(color.data_ptr()), cw, ch))

    def reset(self):
        check(lib.bf_cache_reset(self._h))

    def num_frames(self):
        v = C.c_uint32()
        check(lib.bf_cache_get_num_frames(self._h, C.byref(v)))
        return v.value

    def frames_gpu(self):
        p = C.c_void_p()
        check(lib.bf_cache_get_frames_gpu(self._h, C.byref(p)))
        return p.value

    def geometry(self):
        w, h = C.c_uint32(), C.c_uint32()
        k = (C.c_float * 4)()
        check(lib.bf_cache_get_geometry(self._h, C.byref(w), C.byref(h), k))
        return w.value, h.value, [k[0], k[1], k[2], k[3]]

    def download_frame(self, i):
        import torch
        torch.cuda.synchronize()
        f = CachedFrame()
        check(lib.bf_cache_get_frame(self._h, i, C.byref(f)))
        n = self.w * self.h
        return dict(
            depth=_d2h(f.d_depthDownsampled, n * 4).view("<f4").reshape(self.h, self.w),
            campos=_d2h(f.d_cameraposDownsampled, n * 16).view("<f4").reshape(self.h, self.w, 4),
            intensity=_d2h(f.d_intensityDownsampled, n * 4).view("<f4").reshape(self.h, self.w),
            derivs=_d2h(f.d_intensityDerivsDownsampled, n * 8).view("<f4").reshape(self.h, self.w, 2),
            normals_u=_d2h(f.d_normalsDownsampledUCHAR4, n * 4).reshape(self.h, self.w, 4),
            normals=_d2h(f.d_normalsDownsampled, n * 16).view("<f4").reshape(self.h, self.w, 4),
        )


class Solver:
    """Python view of `bf_solver` (== the reference's CUDASolverBundling)."""

    def __init__(self, max_images, max_residuals, cfg=None, stream=None):
        self._h = C.c_void_p()
        self.cfg = cfg or default_solver_config()
        check(lib.bf_solver_create(max_images, max_residuals, C.byref(self.cfg), C.byref(self._h)))
        if stream is not None:
            check(lib.bf_solver_set_stream(self._h, C.c_void_p(stream)))

    def close(self):
        if self._h:
            lib.bf_solver_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, corr, num_corr, valid, num_images, n_nonlin, n_lin, cache, weights_sparse, weights_dense_depth, weights_dense_color,
              rot, trans, use_pairwise=True, rebuild_jt=True, find_max_residual=False, revalidate_idx=0xFFFFFFFF):
        nw = len(weights_sparse)
        ws = (C.c_float * nw)(*weights_sparse)
        wd = (C.c_float * nw)(*weights_dense_depth)
        wc = (C.c_float * nw)(*weights_dense_color)
        if cache is not None:
            w, h, k = cache.geometry()
            frames, k4 = C.c_void_p(cache.frames_gpu()), (C.c_float * 4)(*k)
        else:
            w = h = 0
            frames, k4 = None, None
        check(lib.bf_solver_solve(self._h, C.c_void_p(corr.data_ptr()) if corr is not None else None, num_corr,
                                  C.c_void_p(valid.data_ptr()), num_images, n_nonlin, n_lin, frames, w, h, k4, ws, wd, wc, nw,
                                  int(use_pairwise), C.c_void_p(rot.data_ptr()), C.c_void_p(trans.data_ptr()), int(rebuild_jt),
                                  int(find_max_residual), C.c_uint32(revalidate_idx)))

    def max_residual(self):
        m, i = C.c_float(), C.c_int32()
        check(lib.bf_solver_get_max_residual(self._h, C.byref(m), C.byref(i)))
        return m.value, i.value

    def max_residual_pair(self, cur_frame, corr):
        idx = (C.c_uint32 * 2)()
        m, rm = C.c_float(), C.c_int()
        check(lib.bf_solver_get_max_residual_pair(self._h, cur_frame, C.c_void_p(corr.data_ptr()), idx, C.byref(m), C.byref(rm)))
        return (idx[0], idx[1]), m.value, bool(rm.value)

    def use_verification(self, corr, num_corr):
        out = C.c_int()
        check(lib.bf_solver_use_verification(self._h, C.c_void_p(corr.data_ptr()), num_corr, C.byref(out)))
        return bool(out.value)

    def convergence(self):
        buf = (C.c_float * 40)()
        n = C.c_uint32()
        check(lib.bf_solver_get_convergence(self._h, buf, 40, C.byref(n)))
        return [buf[i] for i in range(n.value)]

    def iteration_counts(self):
        buf = (C.c_int32 * 33)()
        check(lib.bf_solver_get_iteration_counts(self._h, buf, 33))
        return buf[0], [buf[1 + i] for i in range(buf[0])]

    def debug_dense_system(self, n):
        dim = 6 * n
        JtJ = np.zeros((dim, dim), dtype=np.float32)
        Jtr = np.zeros(dim, dtype=np.float32)
        npairs = C.c_int32()
        check(lib.bf_solver_debug_dense_system(self._h, JtJ.ctypes.data_as(C.c_void_p), Jtr.ctypes.data_as(C.c_void_p), n, C.byref(npairs)))
        return JtJ, Jtr, npairs.value

    def debug_system(self, n):
        """the last Gauss-Newton iteration's A (6N x 6N), b = -J^T F and M^-1 in the reference's layout"""
        dim = 6 * n
        A = np.zeros((dim, dim), dtype=np.float32)
        b = np.zeros(dim, dtype=np.float32)
        prec = np.zeros(dim, dtype=np.float32)
        check(lib.bf_solver_debug_system(self._h, A.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), prec.ctypes.data_as(C.c_void_p), n))
        return A, b, prec

    def slot_overflow(self):
        v = C.c_uint32()
        check(lib.bf_solver_get_slot_overflow(self._h, C.byref(v)))
        return v.value


def convert_matrices_to_poses(T, rot, trans, valid, stream=0):
    check(lib.bf_convert_matrices_to_poses(C.c_void_p(T.data_ptr()), T.shape[0], C.c_void_p(rot.data_ptr()), C.c_void_p(trans.data_ptr()),
                                           C.c_void_p(valid.data_ptr()), C.c_void_p(stream)))


def convert_poses_to_matrices(rot, trans, T, valid, stream=0):
    check(lib.bf_convert_poses_to_matrices(C.c_void_p(rot.data_ptr()), C.c_void_p(trans.data_ptr()), T.shape[0], C.c_void_p(T.data_ptr()),
                                           C.c_void_p(valid.data_ptr()), C.c_void_p(stream)))


# --------------------------------------------------------------------------- SIFT detection
KEYPOINT_DTYPE = np.dtype([("pos", "<f4", 2), ("scale", "<f4"), ("depth", "<f4")])


class Sift:
    """Python view of `bf_sift` (== the reference's SiftGPU detection object)."""

    def __init__(self, width, height, depth_w, depth_h, feature_count_threshold=150, depth_min=0.1, depth_max=4.0, min_key_scale=3.0,
                 max_keys=1024, stream=None):
        self._h = C.c_void_p()
        self.w, self.h, self.max_keys = width, height, max_keys
        check(lib.bf_sift_create(width, height, depth_w, depth_h, feature_count_threshold, C.c_float(depth_min), C.c_float(depth_max),
                                 C.c_float(min_key_scale), max_keys, C.byref(self._h)))
        if stream is not None:
            check(lib.bf_sift_set_stream(self._h, C.c_void_p(stream)))

    def close(self):
        if self._h:
            lib.bf_sift_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, intensity, depth, keys, descs, count):
        check(lib.bf_sift_run(self._h, C.c_void_p(intensity.data_ptr()), C.c_void_p(depth.data_ptr()), C.c_void_p(keys.data_ptr()),
                              C.c_void_p(descs.data_ptr()), C.c_void_p(count.data_ptr())))

    def debug_level(self, octave, index):
        out = np.empty(((self.h >> octave), (self.w >> octave)), dtype=np.float32)
        check(lib.bf_sift_debug_level(self._h, octave, index, out.ctypes.data_as(C.c_void_p)))
        return out

    def debug_counts(self):
        out = (C.c_int32 * 26)()
        check(lib.bf_sift_debug_counts(self._h, out))
        return dict(num_raw=out[0], num_feat=out[1], level0=[out[2 + i] for i in range(12)], level1=[out[14 + i] for i in range(12)])


def rgbx_to_intensity(color):
    """CUDAImageUtil convertToIntensity (CUDAImageUtil.cu:204-207) in float32, same op order."""
    c = color.astype(np.float32)
    return ((np.float32(0.299) * c[..., 0] + np.float32(0.587) * c[..., 1]) + np.float32(0.114) * c[..., 2]) / np.float32(255.0)


# --------------------------------------------------------------------------- keypoint / match store
class SiftImageGPU(C.Structure):
    _fields_ = [("d_keyPoints", C.c_void_p), ("d_keyPointDescs", C.c_void_p), ("d_numKeyPoints", C.c_void_p)]


def _h2d(ptr, arr):
    arr = np.ascontiguousarray(arr)
    check(lib.bf_memcpy_h2d(C.c_void_p(ptr), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes)))


def _f16(m):
    return (C.c_float * 16)(*np.asarray(m, np.float32).reshape(16))


class SiftManager:
    """Python view of `bf_siftmgr` (== the reference's SIFTImageManager + the matcher it feeds)."""
    MAX_RAW, MAX_FILT = 128, 25

    def __init__(self, max_images, max_keys=1024, stream=None):
        self._h = C.c_void_p()
        self.max_images, self.max_keys = max_images, max_keys
        check(lib.bf_siftmgr_create(max_images, max_keys, C.byref(self._h)))
        if stream is not None:
            check(lib.bf_siftmgr_set_stream(self._h, C.c_void_p(stream)))

    def close(self):
        if self._h:
            lib.bf_siftmgr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(lib.bf_siftmgr_reset(self._h))

    def create_image(self):
        img = SiftImageGPU()
        check(lib.bf_siftmgr_create_image(self._h, C.byref(img)))
        return img

    def finalize_image(self, num_keys=-1):
        check(lib.bf_siftmgr_finalize_image(self._h, int(num_keys)))

    def add_image_host(self, keys, descs):
        """createSIFTImageGPU + H2D upload + finalize (the fuseToGlobal / loadFromFile way of filling an image)."""
        img = self.create_image()
        keys = np.ascontiguousarray(keys, np.float32).reshape(-1, 4); descs = np.ascontiguousarray(descs, np.uint8).reshape(-1, 128)
        _h2d(img.d_keyPoints, keys); _h2d(img.d_keyPointDescs, descs)
        self.finalize_image(len(keys))

    def add_image_sift(self, sift, intensity, depth):
        """detectFeatures (Bundler.cpp:91-101): the detector writes keys, descriptors and the count straight into the store."""
        img = self.create_image()
        check(lib.bf_sift_run(sift._h, C.c_void_p(intensity.data_ptr()), C.c_void_p(depth.data_ptr()), C.c_void_p(img.d_keyPoints),
                              C.c_void_p(img.d_keyPointDescs), C.c_void_p(img.d_numKeyPoints)))
        self.finalize_image(-1)

    def num_images(self):
        n = C.c_uint32()
        check(lib.bf_siftmgr_get_num_images(self._h, C.byref(n)))
        return n.value

    def num_keypoints(self, first=0, count=None):
        count = self.num_images() - first if count is None else count
        out = np.zeros(count, np.int32)
        check(lib.bf_siftmgr_get_num_keypoints(self._h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def download_image(self, i):
        img = SiftImageGPU()
        check(lib.bf_siftmgr_get_image(self._h, i, C.byref(img)))
        n = max(int(self.num_keypoints(i, 1)[0]), 0)
        keys = _d2h(img.d_keyPoints, 16 * n).view(np.float32).reshape(n, 4)
        descs = _d2h(img.d_keyPointDescs, 128 * n).reshape(n, 128)
        return keys, descs

    def set_current_frame(self, i):
        check(lib.bf_siftmgr_set_current_frame(self._h, i))

    def current_frame(self):
        n = C.c_uint32()
        check(lib.bf_siftmgr_get_current_frame(self._h, C.byref(n)))
        return n.value

    def match(self, cur, start, num, dist_max=0.7, ratio_max=0.8):
        check(lib.bf_siftmgr_match(self._h, cur, start, num, C.c_float(dist_max), C.c_float(ratio_max)))

    def set_pair_stage(self, set, stream_ptr=None, speculative=0):
        """The pair kernels issued from now on work on result set `set` (0 / 1) and on the HIP stream `stream_ptr` (None: the manager's stream); speculative:
        they do not consult the valid flags of the previous images (commit_pairs clears those pairs afterwards).  The accessors of the per-pair lists name the
        selected set; ordering between the two streams is the caller's.  (0, None, 0) is the reference's behaviour."""
        check(lib.bf_siftmgr_set_pair_stage(self._h, int(set), None if stream_ptr is None else C.c_void_p(stream_ptr), int(speculative)))

    def commit_pairs(self, cur, start, num):
        """On the manager's stream: zero the raw and filtered match counts (of the selected set) of the invalid previous images in [start, num)."""
        check(lib.bf_siftmgr_commit_pairs(self._h, cur, start, num))

    def filter_keypoint_matches(self, cur, start, num, Kinv, min_matches=5, max_res2=0.0004):
        check(lib.bf_siftmgr_filter_keypoint_matches(self._h, cur, start, num, _f16(Kinv), min_matches, C.c_float(max_res2)))

    def filter_surface_area(self, cur, start, num, Kinv, area_thresh=0.032):
        check(lib.bf_siftmgr_filter_matches_by_surface_area(self._h, cur, start, num, _f16(Kinv), C.c_float(area_thresh)))

    def filter_dense_verify(self, cur, start, num, W, H, K, d_frames, dist_thresh=0.15, normal_thresh=0.97, color_thresh=0.1, err_thresh=0.075,
                            corr_thresh=0.02, dmin=0.1, dmax=3.0):
        check(lib.bf_siftmgr_filter_matches_by_dense_verify(self._h, cur, start, num, W, H, _f16(K), C.c_void_p(d_frames), C.c_float(dist_thresh),
                                                            C.c_float(normal_thresh), C.c_float(color_thresh), C.c_float(err_thresh),
                                                            C.c_float(corr_thresh), C.c_float(dmin), C.c_float(dmax)))

    def filter_frames(self, cur, start, num):
        last = C.c_uint32()
        check(lib.bf_siftmgr_filter_frames(self._h, cur, start, num, C.byref(last)))
        return last.value

    def filter_frames_async(self, cur, start, num):
        check(lib.bf_siftmgr_filter_frames_async(self._h, cur, start, num))

    def add_curr_to_residuals(self, cur, start, num, Kinv):
        check(lib.bf_siftmgr_add_curr_to_residuals(self._h, cur, start, num, _f16(Kinv)))

    def commit_frame(self, cur, start, num, Kinv):
        """filter_frames_async and add_curr_to_residuals in one launch"""
        check(lib.bf_siftmgr_commit_frame(self._h, cur, start, num, _f16(Kinv)))

    def sync_frame_result(self, cur):
        last = C.c_uint32(); nk = C.c_int32()
        check(lib.bf_siftmgr_sync_frame_result(self._h, cur, C.byref(last), C.byref(nk)))
        return last.value, nk.value

    def invalidate_image_to_image(self, i, j):
        check(lib.bf_siftmgr_invalidate_image_to_image(self._h, i, j))

    def check_for_invalid_frames(self, d_num_entries, num_vars, simple=False):
        f = lib.bf_siftmgr_check_for_invalid_frames_simple if simple else lib.bf_siftmgr_check_for_invalid_frames
        check(f(self._h, C.c_void_p(d_num_entries), num_vars))

    def verify_trajectory(self, num_images, d_traj, W, H, K, d_frames, dist_thresh=0.15, normal_thresh=0.97, color_thresh=0.1, err_thresh=0.05,
                          corr_thresh=0.001, dmin=0.1, dmax=3.0):
        v = C.c_int32()
        check(lib.bf_siftmgr_verify_trajectory(self._h, num_images, C.c_void_p(d_traj), W, H, _f16(K), C.c_void_p(d_frames), C.c_float(dist_thresh),
                                               C.c_float(normal_thresh), C.c_float(color_thresh), C.c_float(err_thresh), C.c_float(corr_thresh),
                                               C.c_float(dmin), C.c_float(dmax), C.byref(v)))
        return v.value

    def valid_images(self, count=None):
        count = self.num_images() if count is None else count
        out = np.zeros(count, np.int32)
        check(lib.bf_siftmgr_get_valid_images(self._h, out.ctypes.data_as(C.c_void_p), count))
        return out

    def set_valid_image(self, frame, valid):
        check(lib.bf_siftmgr_set_valid_image(self._h, frame, int(valid)))

    def update_gpu_valid_images(self):
        check(lib.bf_siftmgr_update_gpu_valid_images(self._h))

    def valid_images_gpu(self):
        p = C.c_void_p()
        check(lib.bf_siftmgr_get_valid_images_gpu(self._h, C.byref(p)))
        return p.value

    def num_global_correspondences(self):
        n = C.c_uint32()
        check(lib.bf_siftmgr_get_num_global_correspondences(self._h, C.byref(n)))
        return n.value

    def global_correspondences_gpu(self):
        p = C.c_void_p()
        check(lib.bf_siftmgr_get_global_correspondences_gpu(self._h, C.byref(p)))
        return p.value

    def download_global_correspondences(self):
        n = self.num_global_correspondences()
        corr = _d2h(self.global_correspondences_gpu(), 32 * n).view(ENTRYJ_DTYPE)
        p = C.c_void_p()
        check(lib.bf_siftmgr_get_global_correspondence_keys_gpu(self._h, C.byref(p)))
        keys = _d2h(p.value, 8 * n).view(np.uint32).reshape(n, 2)
        return corr, keys

    def set_global_correspondences(self, corr):
        corr = np.ascontiguousarray(corr)
        check(lib.bf_siftmgr_set_global_correspondences(self._h, corr.ctypes.data_as(C.c_void_p), len(corr)))

    def raw_matches(self, pair):
        n = C.c_int32(); idx = np.zeros((128, 2), np.uint32); dist = np.zeros(128, np.float32)
        check(lib.bf_siftmgr_get_raw_matches(self._h, pair, C.byref(n), idx.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p)))
        return n.value, idx, dist

    def filt_matches(self, pair):
        n = C.c_int32(); idx = np.zeros((25, 2), np.uint32); dist = np.zeros(25, np.float32)
        T = np.zeros((4, 4), np.float32); Ti = np.zeros((4, 4), np.float32)
        check(lib.bf_siftmgr_get_filt_matches(self._h, pair, C.byref(n), idx.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p),
                                              T.ctypes.data_as(C.c_void_p), Ti.ctypes.data_as(C.c_void_p)))
        return n.value, idx, dist, T, Ti

    def set_raw_matches(self, pair, n, idx=None, dist=None):
        """Overwrite the raw match list of one previous image: the count and (where given) the 128 index pairs / distances; shorter arrays are
        zero-padded.  No index is checked: the caller keeps every key index below num_images * max_keys."""
        i = d = None
        if idx is not None:
            idx = np.asarray(idx, np.uint32).reshape(-1, 2)
            i = np.zeros((self.MAX_RAW, 2), np.uint32); i[:len(idx)] = idx
        if dist is not None:
            dist = np.asarray(dist, np.float32).reshape(-1)
            d = np.zeros(self.MAX_RAW, np.float32); d[:len(dist)] = dist
        check(lib.bf_siftmgr_set_raw_matches(self._h, pair, int(n), None if i is None else i.ctypes.data_as(C.c_void_p),
                                             None if d is None else d.ctypes.data_as(C.c_void_p)))

    def set_filt_matches(self, pair, n, idx=None, dist=None, T=None, Tinv=None):
        """Overwrite the filtered match list of one previous image: the count and (where given) the 25 index pairs / distances and the two 4x4
        transforms; shorter arrays are zero-padded.  No index is checked."""
        i = d = t = ti = None
        if idx is not None:
            idx = np.asarray(idx, np.uint32).reshape(-1, 2)
            i = np.zeros((self.MAX_FILT, 2), np.uint32); i[:len(idx)] = idx
        if dist is not None:
            dist = np.asarray(dist, np.float32).reshape(-1)
            d = np.zeros(self.MAX_FILT, np.float32); d[:len(dist)] = dist
        if T is not None:
            t = np.ascontiguousarray(T, np.float32).reshape(16)
        if Tinv is not None:
            ti = np.ascontiguousarray(Tinv, np.float32).reshape(16)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(lib.bf_siftmgr_set_filt_matches(self._h, pair, int(n), p(i), p(d), p(t), p(ti)))

    def fuse_to_global(self, glob, K, d_transforms, Kinv, host=False):
        """fuseToGlobal on the device (default) or in the reference's host form (host=True); same results bit for bit"""
        fn = lib.bf_siftmgr_fuse_to_global_host if host else lib.bf_siftmgr_fuse_to_global
        check(fn(self._h, glob._h, _f16(K), C.c_void_p(d_transforms), _f16(Kinv)))

    def fuse_error(self):
        e = C.c_int()
        check(lib.bf_siftmgr_fuse_error(self._h, C.byref(e)))
        return e.value

    def set_fuse_lds_limit(self, keys):
        """the device fuse searches from LDS while at most `keys` keys have a valid correspondence (and they fit), from global memory beyond; 0: never from LDS"""
        check(lib.bf_siftmgr_set_fuse_lds_limit(self._h, int(keys)))

    def fuse_path(self):
        """the form the last device fuse ran in: 1 LDS, 0 global memory"""
        e = C.c_int()
        check(lib.bf_siftmgr_fuse_path(self._h, C.byref(e)))
        return e.value


# --------------------------------------------------------------------------- host-level operators (include/bf_pipeline.h)
class GlobalAppState(C.Structure):
    _fields_ = [
        ("s_sensorIdx", C.c_uint32), ("s_integrationWidth", C.c_uint32), ("s_integrationHeight", C.c_uint32),
        ("s_maxFrameFixes", C.c_uint32), ("s_topNActive", C.c_uint32), ("s_minPoseDistSqrt", C.c_float),
        ("s_sensorDepthMax", C.c_float), ("s_sensorDepthMin", C.c_float), ("s_renderDepthMax", C.c_float), ("s_renderDepthMin", C.c_float),
        ("s_hashNumBuckets", C.c_uint32), ("s_hashNumSDFBlocks", C.c_uint32), ("s_hashMaxCollisionLinkedListSize", C.c_uint32),
        ("s_SDFVoxelSize", C.c_float), ("s_SDFTruncation", C.c_float), ("s_SDFTruncationScale", C.c_float), ("s_SDFMaxIntegrationDistance", C.c_float),
        ("s_SDFIntegrationWeightSample", C.c_uint32), ("s_SDFIntegrationWeightMax", C.c_uint32),
        ("s_colorSigmaD", C.c_float), ("s_colorSigmaR", C.c_float), ("s_colorFilter", C.c_int32),
        ("s_integrationEnabled", C.c_int32), ("s_garbageCollectionEnabled", C.c_int32), ("s_reconstructionEnabled", C.c_int32), ("s_streamingEnabled", C.c_int32),
        ("s_bUseCameraCalibration", C.c_int32), ("s_binaryDumpSensorUseTrajectory", C.c_int32), ("s_garbageCollectionStarve", C.c_uint32),
        ("s_streamingVoxelExtents", C.c_float * 3), ("s_streamingGridDimensions", C.c_int32 * 3), ("s_streamingMinGridPos", C.c_int32 * 3),
        ("s_streamingInitialChunkListSize", C.c_uint32), ("s_numSolveFramesBeforeExit", C.c_uint32),
        ("s_binaryDumpSensorFile", C.c_char * 512),
        ("s_rayCastWidth", C.c_uint32), ("s_rayCastHeight", C.c_uint32),
        ("s_SDFRayIncrementFactor", C.c_float), ("s_SDFRayThresSampleDistFactor", C.c_float), ("s_SDFRayThresDistFactor", C.c_float),
        ("s_SDFUseGradients", C.c_int32),
        ("s_remappingDepthDiscontinuityThresOffset", C.c_float), ("s_remappingDepthDiscontinuityThresLin", C.c_float),
    ]


class GlobalBundlingState(C.Structure):
    _fields_ = [
        ("s_enableGlobalTimings", C.c_int32), ("s_enablePerFrameTimings", C.c_int32),
        ("s_maxNumImages", C.c_uint32), ("s_submapSize", C.c_uint32), ("s_widthSIFT", C.c_uint32), ("s_heightSIFT", C.c_uint32), ("s_maxNumKeysPerImage", C.c_uint32),
        ("s_numLocalNonLinIterations", C.c_uint32), ("s_numLocalLinIterations", C.c_uint32), ("s_numGlobalNonLinIterations", C.c_uint32),
        ("s_numGlobalLinIterations", C.c_uint32), ("s_downsampledWidth", C.c_uint32), ("s_downsampledHeight", C.c_uint32),
        ("s_verifySiftErrThresh", C.c_float), ("s_verifySiftCorrThresh", C.c_float), ("s_projCorrDistThres", C.c_float), ("s_projCorrNormalThres", C.c_float),
        ("s_projCorrColorThresh", C.c_float), ("s_surfAreaPcaThresh", C.c_float),
        ("s_recordSolverConvergence", C.c_int32), ("s_erodeSIFTdepth", C.c_int32),
        ("s_verifyOptErrThresh", C.c_float), ("s_verifyOptCorrThresh", C.c_float),
        ("s_verbose", C.c_int32), ("s_sendUplinkFeedbackImage", C.c_int32),
        ("s_depthSigmaD", C.c_float), ("s_depthSigmaR", C.c_float), ("s_depthFilter", C.c_int32),
        ("s_minNumMatchesLocal", C.c_uint32), ("s_minNumMatchesGlobal", C.c_uint32), ("s_useComprehensiveFrameInvalidation", C.c_int32),
        ("s_maxKabschResidual2", C.c_float), ("s_minKeyScale", C.c_float), ("s_siftMatchThresh", C.c_float), ("s_siftMatchRatioMaxLocal", C.c_float),
        ("s_siftMatchRatioMaxGlobal", C.c_float),
        ("s_useLocalVerify", C.c_int32), ("s_useLocalDense", C.c_int32), ("s_numOptPerResidualRemoval", C.c_uint32),
        ("s_colorDownSigma", C.c_float), ("s_depthDownSigmaD", C.c_float), ("s_depthDownSigmaR", C.c_float),
        ("s_optMaxResThresh", C.c_float), ("s_denseDistThresh", C.c_float), ("s_denseNormalThresh", C.c_float), ("s_denseColorThresh", C.c_float),
        ("s_denseColorGradientMin", C.c_float), ("s_denseDepthMin", C.c_float), ("s_denseDepthMax", C.c_float),
        ("s_denseOverlapCheckSubsampleFactor", C.c_uint32),
    ]


class RGBDSensorDesc(C.Structure):
    _fields_ = [("depthWidth", C.c_uint32), ("depthHeight", C.c_uint32), ("colorWidth", C.c_uint32), ("colorHeight", C.c_uint32),
                ("depthIntrinsics", C.c_float * 16), ("colorIntrinsics", C.c_float * 16), ("depthExtrinsics", C.c_float * 16), ("colorExtrinsics", C.c_float * 16)]


class FrameTiming(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("timeSensorProcess", "timeSiftDetection", "timeSiftMatching", "timeMatchFilter", "timeSolve", "timeReIntegrate",
                                         "timeReconstruct", "timeTotal")]


def default_app_state(path=None):
    g = GlobalAppState()
    if path is None:
        check(lib.bf_global_app_state_default(C.byref(g)))
    else:
        check(lib.bf_global_app_state_read(path.encode(), C.byref(g), None))
    return g


def default_bundling_state(path=None):
    g = GlobalBundlingState()
    if path is None:
        check(lib.bf_global_bundling_state_default(C.byref(g)))
    else:
        check(lib.bf_global_bundling_state_read(path.encode(), C.byref(g), None))
    return g


def sensor_desc(width, height, K, color_K=None, depth_extrinsics=None):
    """A sensor of one image size with depth intrinsics K (4x4).  By default its depth and colour cameras coincide (identity extrinsics, the same
    intrinsics); color_K gives the colour camera intrinsics of its own, depth_extrinsics (4x4, depth camera -> colour camera) a displaced depth camera."""
    s = RGBDSensorDesc()
    s.depthWidth = s.colorWidth = width
    s.depthHeight = s.colorHeight = height
    k = np.asarray(K, np.float32).reshape(16)
    kc = k if color_K is None else np.asarray(color_K, np.float32).reshape(16)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    ext = eye if depth_extrinsics is None else np.asarray(depth_extrinsics, np.float32).reshape(16)
    for i in range(16):
        s.depthIntrinsics[i] = float(k[i]); s.colorIntrinsics[i] = float(kc[i])
        s.depthExtrinsics[i] = float(ext[i]); s.colorExtrinsics[i] = float(eye[i])
    return s


# --------------------------------------------------------------------------- frame-ingest image operators (csrc/imageops.hip)
# torch device tensors in; an image's size is its tensor's (h, w) shape (uint8 colour: (h, w, 4)).  `stream`: a hipStream_t (0: the null stream).
def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def image_erode_depth_map(out, inp, structure_size=3, d_thresh=0.05, frac_req=0.3, stream=0):
    h, w = inp.shape[:2]
    check(lib.bf_image_erode_depth_map(_p(out), _p(inp), int(structure_size), w, h, C.c_float(d_thresh), C.c_float(frac_req), C.c_void_p(stream)))


def image_erode_depth_map_and_copy(out, inp, copy_src, copy_dst1, copy_dst2=None, structure_size=3, d_thresh=0.05, frac_req=0.3, stream=0):
    """the erosion with a pixel-wise copy of a 4-byte-per-pixel image of the same size riding along (copy_src -> copy_dst1 and, if given, copy_dst2)"""
    h, w = inp.shape[:2]
    check(lib.bf_image_erode_depth_map_and_copy(_p(out), _p(inp), int(structure_size), w, h, C.c_float(d_thresh), C.c_float(frac_req),
                                                _p(copy_src), _p(copy_dst1), _p(copy_dst2), C.c_void_p(stream)))


def image_gauss_filter_depth_map(out, inp, sigma_d, sigma_r, stream=0):
    h, w = inp.shape[:2]
    check(lib.bf_image_gauss_filter_depth_map(_p(out), _p(inp), C.c_float(sigma_d), C.c_float(sigma_r), w, h, C.c_void_p(stream)))


def image_gauss_filter_depth_map2(out, out2, inp, sigma_d, sigma_r, stream=0):
    h, w = inp.shape[:2]
    check(lib.bf_image_gauss_filter_depth_map2(_p(out), _p(out2), _p(inp), C.c_float(sigma_d), C.c_float(sigma_r), w, h, C.c_void_p(stream)))


def image_gauss_filter_intensity(out, inp, sigma_d, stream=0):
    h, w = inp.shape[:2]
    check(lib.bf_image_gauss_filter_intensity(_p(out), _p(inp), C.c_float(sigma_d), w, h, C.c_void_p(stream)))


def image_resample_float(out, inp, stream=0):
    (oh, ow), (ih, iw) = out.shape[:2], inp.shape[:2]
    check(lib.bf_image_resample_float(_p(out), ow, oh, _p(inp), iw, ih, C.c_void_p(stream)))


def image_resample_uchar4(out, inp, stream=0):
    (oh, ow), (ih, iw) = out.shape[:2], inp.shape[:2]
    check(lib.bf_image_resample_uchar4(_p(out), ow, oh, _p(inp), iw, ih, C.c_void_p(stream)))


def image_resample_to_intensity(out, inp, stream=0):
    (oh, ow), (ih, iw) = out.shape[:2], inp.shape[:2]
    check(lib.bf_image_resample_to_intensity(_p(out), ow, oh, _p(inp), iw, ih, C.c_void_p(stream)))


def image_interleave_texels(texels, depth, color, stream=0):
    """{depth f32 bits, colour RGBX8} per pixel: `texels` holds depth.numel() x 8 bytes"""
    check(lib.bf_image_interleave_texels(_p(texels), _p(depth), _p(color), depth.numel(), C.c_void_p(stream)))


# --------------------------------------------------------------------------- depth registration (csrc/calibrator.hip)
class ImageCalibrator:
    """Python view of `bf_image_calibrator` (== the reference's CUDAImageCalibrator): re-renders a depth image into the colour camera.  width x height: the
    depth image's size; `stream`: a hipStream_t (0: the null stream)."""

    def __init__(self, width, height, stream=0):
        self._h = C.c_void_p()
        self.w, self.h = int(width), int(height)
        check(lib.bf_image_calibrator_create(self.w, self.h, C.byref(self._h)))
        if stream:
            check(lib.bf_image_calibrator_set_stream(self._h, C.c_void_p(stream)))

    def close(self):
        if self._h:
            lib.bf_image_calibrator_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process(self, depth, color_intrinsics, depth_intrinsics_inv, depth_extrinsics, thresh_offset=0.012, thresh_lin=0.01):
        """depth: float32 torch device tensor (h, w), replaced in place by the depth seen from the colour camera (-inf where nothing was drawn).
        color_intrinsics: the colour camera's at the depth image's size; depth_extrinsics: depth camera -> colour camera (4x4 each)."""
        assert tuple(depth.shape) == (self.h, self.w) and depth.is_contiguous()
        check(lib.bf_image_calibrator_process(self._h, _p(depth), mat16(color_intrinsics), mat16(depth_intrinsics_inv), mat16(depth_extrinsics),
                                              C.c_float(thresh_offset), C.c_float(thresh_lin)))
        return depth


# --------------------------------------------------------------------------- sensor-format ingest (csrc/sensoringest.hip)
BF_ERR_NOT_ON_DEVICE = -6


class JpegComponent(C.Structure):
    _fields_ = [("h", C.c_uint32), ("v", C.c_uint32), ("tq", C.c_uint32), ("blocksX", C.c_uint32), ("blocksY", C.c_uint32), ("blockOffset", C.c_uint32),
                ("planeOffset", C.c_uint32), ("reserved", C.c_uint32)]


class JpegInfo(C.Structure):
    """bf_jpeg_info: a baseline JPEG frame between its entropy decode and its reconstruction (layout of the coefficient buffer: include/bf_hip.h)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("numComponents", C.c_uint32), ("hmax", C.c_uint32), ("vmax", C.c_uint32), ("mcusX", C.c_uint32),
                ("mcusY", C.c_uint32), ("restartInterval", C.c_uint32), ("numBlocks", C.c_uint32), ("planeBytes", C.c_uint32), ("comp", JpegComponent * 3),
                ("qt", (C.c_uint16 * 64) * 4), ("qtPresent", C.c_uint8 * 4)]


def image_convert_depth_u16(out, inp, depth_shift, stream=0):
    """u16 depth -> float32 metres (0 -> -inf); torch device tensors, out.numel() == inp.numel()"""
    check(lib.bf_image_convert_depth_u16(_p(out), _p(inp), C.c_float(depth_shift), inp.numel(), C.c_void_p(stream)))


def image_convert_rgb8_to_rgbx(out, inp, stream=0):
    """RGB8 (n x 3 bytes) -> RGBX8 with X = 255"""
    check(lib.bf_image_convert_rgb8_to_rgbx(_p(out), _p(inp), inp.numel() // 3, C.c_void_p(stream)))


def jpeg_reconstruct_device(info, coefficients, planes, rgbx, stream=0):
    """quantised coefficients (int16 device tensor) -> RGBX8 (h, w, 4); planes: info.planeBytes bytes of device scratch.  Returns False where the device
    declines the layout (BF_ERR_NOT_ON_DEVICE: decode on the host), raises on every other failure."""
    rc = lib.bf_jpeg_reconstruct_device(C.byref(info), _p(coefficients), _p(planes), _p(rgbx), C.c_void_p(stream))
    if rc == BF_ERR_NOT_ON_DEVICE:
        return False
    check(rc)
    return True


def image_convert_depth_to_u16(out, inp, depth_shift, stream=0):
    """float32 metres -> u16, the recording's rule (bf_image_convert_depth_to_u16); torch device tensors, out.numel() == inp.numel()"""
    check(lib.bf_image_convert_depth_to_u16(_p(out), _p(inp), C.c_float(depth_shift), inp.numel(), C.c_void_p(stream)))


def jpeg_forward_device(rgbx, width, height, quality, coefficients, stream=0):
    """RGBX8 device image -> quantised coefficients, int16 device tensor of ceil(w/8) * ceil(h/8) * 192 values in bf_jpeg_forward_host's layout"""
    check(lib.bf_jpeg_forward_device(_p(rgbx), int(width), int(height), int(quality), _p(coefficients), C.c_void_p(stream)))


def _raw_colour(colour, jpeg):
    """the colour argument of the *_raw_decoded / *_raw_device calls as (pointer, keep-alive)"""
    if isinstance(colour, np.ndarray):
        colour = np.ascontiguousarray(colour, np.int16 if jpeg is not None else np.uint8)
        return colour.ctypes.data_as(C.c_void_p), colour
    return C.c_void_p(colour.data_ptr()), colour


class ImageManager:
    """Python view of `bf_image_manager` (== the reference's CUDAImageManager): the frame ingest (erosion, depth filter, resampling) and the
    frames stored at integration resolution.  store_frames_on_gpu: 1 slabs of frames in device memory, 0 host copies (the reference's default),
    2 one device slot that every frame overwrites."""

    def __init__(self, gas, gbs, sensor, store_frames_on_gpu=1):
        self._h = C.c_void_p()
        self.sensor = sensor
        self.w, self.h = gas.s_integrationWidth, gas.s_integrationHeight
        check(lib.bf_image_manager_create(self.w, self.h, gbs.s_widthSIFT, gbs.s_heightSIFT, C.byref(sensor), C.byref(gbs), int(store_frames_on_gpu),
                                          C.byref(self._h)))

    def close(self):
        if self._h:
            lib.bf_image_manager_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_store_texels(self, enable=True):
        check(lib.bf_image_manager_set_store_texels(self._h, int(enable)))

    def set_camera_calibration(self, enable=True, thresh_offset=0.012, thresh_lin=0.01):
        """s_bUseCameraCalibration: register every frame's depth to the colour camera at ingest (before the first frame).  Returns whether it is active:
        a sensor with identity depth extrinsics has nothing to register and stays off."""
        check(lib.bf_image_manager_set_camera_calibration(self._h, int(enable), C.c_float(thresh_offset), C.c_float(thresh_lin)))
        return self.camera_calibration()

    def camera_calibration(self):
        a = C.c_int()
        check(lib.bf_image_manager_get_camera_calibration(self._h, C.byref(a)))
        return bool(a.value)

    def depth_intrinsics(self):
        """(K, K^-1) of the depth camera at integration resolution, 4x4 each, as the manager computed them"""
        k, ki = (C.c_float * 16)(), (C.c_float * 16)()
        check(lib.bf_image_manager_get_depth_intrinsics(self._h, k, ki))
        return np.array(k[:], np.float32).reshape(4, 4), np.array(ki[:], np.float32).reshape(4, 4)

    def sift_depth(self):
        """(width, height, 4x4 intrinsics) of the depth image the SIFT keys sample: the colour camera's intrinsics while registration is active"""
        w, h, k = C.c_uint32(), C.c_uint32(), (C.c_float * 16)()
        check(lib.bf_image_manager_get_sift_depth(self._h, C.byref(w), C.byref(h), k))
        return w.value, h.value, np.array(k[:], np.float32).reshape(4, 4)

    def reset(self):
        check(lib.bf_image_manager_reset(self._h))

    def process(self, depth, color):
        """host numpy frame (sensor resolution: depth float32 (h, w), colour uint8 (h, w, 4)) -> whether a frame was stored"""
        depth = np.ascontiguousarray(depth, np.float32); color = np.ascontiguousarray(color, np.uint8)
        got = C.c_int()
        check(lib.bf_image_manager_process(self._h, depth.ctypes.data_as(C.c_void_p), color.ctypes.data_as(C.c_void_p), C.byref(got)))
        return bool(got.value)

    def process_device(self, depth, color):
        """the same from torch device tensors"""
        got = C.c_int()
        check(lib.bf_image_manager_process_device(self._h, _p(depth), _p(color), C.byref(got)))
        return bool(got.value)

    def process_raw(self, depth_u16, depth_shift, colour, compression=0, jpeg=None):
        """A frame in sensor format, converted / reconstructed on the device (bf_image_manager_process_raw*).  depth_u16: uint16 (h, w).  colour: the stored
        bytes (`bytes` / uint8 array; compression 0 raw RGB8, 1 PNG, 2 JPEG), or - with `jpeg` a JpegInfo or colour an array that is not bytes-like input of a
        recording - already decoded buffers: host numpy (RGB8 uint8, or int16 coefficients with `jpeg`) or torch device tensors (depth_u16 then as a device tensor too)."""
        got = C.c_int()
        if isinstance(depth_u16, np.ndarray):
            d = np.ascontiguousarray(depth_u16, np.uint16)
            if isinstance(colour, (bytes, bytearray, memoryview)):
                buf = np.frombuffer(colour, np.uint8)
                check(lib.bf_image_manager_process_raw(self._h, d.ctypes.data_as(C.c_void_p), C.c_float(depth_shift), buf.ctypes.data_as(C.c_void_p), C.c_uint64(buf.size),
                                                       int(compression), C.byref(got)))
            else:
                ptr, _keep = _raw_colour(colour, jpeg)
                check(lib.bf_image_manager_process_raw_decoded(self._h, d.ctypes.data_as(C.c_void_p), C.c_float(depth_shift), ptr, C.byref(jpeg) if jpeg is not None else None,
                                                               C.byref(got)))
        else:
            ptr, _keep = _raw_colour(colour, jpeg)
            check(lib.bf_image_manager_process_raw_device(self._h, _p(depth_u16), C.c_float(depth_shift), ptr, C.byref(jpeg) if jpeg is not None else None, C.byref(got)))
        return bool(got.value)

    def get_input_gpu(self):
        """host copies of the last frame's sensor-resolution buffers: (raw depth, filtered depth, colour)"""
        import torch
        torch.cuda.synchronize()
        raw, filt, col = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib.bf_image_manager_get_input_gpu(self._h, C.byref(raw), C.byref(filt), C.byref(col)))
        s = self.sensor
        nd, nc = s.depthWidth * s.depthHeight, s.colorWidth * s.colorHeight
        return (_d2h(raw.value, nd * 4).view("<f4").reshape(s.depthHeight, s.depthWidth),
                _d2h(filt.value, nd * 4).view("<f4").reshape(s.depthHeight, s.depthWidth),
                _d2h(col.value, nc * 4).reshape(s.colorHeight, s.colorWidth, 4))

    def get_integrate_frame_cpu(self, frame):
        """host copies (depth float32 (h, w), colour uint8 (h, w, 4)) of a stored frame at integration resolution"""
        import torch
        torch.cuda.synchronize()
        d = np.zeros((self.h, self.w), np.float32); c = np.zeros((self.h, self.w, 4), np.uint8)
        check(lib.bf_image_manager_get_integrate_frame_cpu(self._h, frame, d.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)))
        return d, c

    def get_integrate_frame_texels(self, frame):
        """host copy (uint8 (h, w, 8)) of a stored frame's interleaved texels, or None where the manager keeps none"""
        import torch
        torch.cuda.synchronize()
        p = C.c_void_p()
        check(lib.bf_image_manager_get_integrate_frame_texels(self._h, frame, C.byref(p)))
        return None if not p.value else _d2h(p.value, self.w * self.h * 8).reshape(self.h, self.w, 8)

    def num_frames(self):
        n = C.c_uint32()
        check(lib.bf_image_manager_get_num_frames(self._h, C.byref(n)))
        return n.value

    def curr_frame_number(self):
        n = C.c_uint32()
        check(lib.bf_image_manager_get_curr_frame_number(self._h, C.byref(n)))
        return n.value


_ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)


class Comm:
    """Python view of `bf_comm` (include/bf_comm.h): the all-gather of the multi-GPU partition.

    Comm.rccl(world, rank, broadcast): RCCL, bootstrapped NCCL-style - rank 0 draws the unique id, `broadcast(bytes_or_None) -> bytes` hands it to every
    rank (e.g. through torch.distributed's store or a gloo broadcast).  Comm.torch_group(group): the all-gather through a torch.distributed process
    group (gloo: through host memory - how two ranks share the one GPU of a test box); collectives issued through one Comm must not interleave with
    other collectives on the same group from another thread - give the volume thread its own group (dist.new_group)."""

    def __init__(self):
        self._h = C.c_void_p()
        self._cb = None

    @classmethod
    def rccl(cls, world, rank, broadcast):
        c = cls()
        ident = (C.c_uint8 * 128)()
        if rank == 0:
            check(lib.bf_comm_unique_id(ident))
        raw = broadcast(bytes(ident) if rank == 0 else None)
        ident = (C.c_uint8 * 128).from_buffer_copy(raw)
        check(lib.bf_comm_create_rccl(ident, int(world), int(rank), C.byref(c._h)))
        return c

    @classmethod
    def torch_group(cls, group=None):
        import torch
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        nccl = dist.get_backend(group) == "nccl"

        def gather(user, d_send, d_recv, nbytes, stream):
            try:
                n = int(nbytes)
                check(lib.bf_stream_synchronize(C.c_void_p(stream)))
                send = torch.empty(n, dtype=torch.uint8, device="cuda" if nccl else "cpu")
                check(lib.bf_memcpy(C.c_void_p(send.data_ptr()), C.c_void_p(d_send), C.c_size_t(n)))
                if nccl:
                    out = torch.empty(world * n, dtype=torch.uint8, device="cuda")
                    dist.all_gather_into_tensor(out, send, group=group)
                    torch.cuda.synchronize()
                else:
                    parts = [torch.empty(n, dtype=torch.uint8) for _ in range(world)]
                    dist.all_gather(parts, send, group=group)
                    out = torch.cat(parts)
                check(lib.bf_memcpy(C.c_void_p(d_recv), C.c_void_p(out.data_ptr()), C.c_size_t(world * n)))
                return 0
            except Exception as e:          # never let an exception cross the C boundary
                import sys
                print("Comm.torch_group all-gather failed: %r" % (e,), file=sys.stderr)
                return 1
        c = cls()
        c._cb = _ALL_GATHER_FN(gather)
        check(lib.bf_comm_create_callback(c._cb, None, int(world), int(rank), C.byref(c._h)))
        return c

    def world(self):
        w, r = C.c_uint32(), C.c_uint32()
        check(lib.bf_comm_world(self._h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def all_gather(self, send, recv, stream=None):
        """send / recv: torch cuda uint8 tensors (recv = world x send)"""
        check(lib.bf_comm_all_gather(self._h, C.c_void_p(send.data_ptr()), C.c_void_p(recv.data_ptr()), C.c_uint64(send.numel()), C.c_void_p(stream)))

    def chunk_exchange(self, mine, stream=None):
        """One round of chunk packages: `mine` (uint8 numpy array) -> list of `world` arrays in owner order (bf_chunk_exchange)."""
        w, _ = self.world()
        mine = np.ascontiguousarray(mine, np.uint8)
        out = np.zeros(w * mine.size, np.uint8)
        check(lib.bf_chunk_exchange(self._h, mine.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_uint64(mine.size), C.c_void_p(stream)))
        return [np.ascontiguousarray(out[r * mine.size:(r + 1) * mine.size]) for r in range(w)]

    def close(self):
        if self._h:
            lib.bf_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    """Python view of `bf_pipeline`: the serial frame loop of DepthSensing.cpp (ingest -> bundling input -> re-integration ->
    integration of the current frame -> local / global optimisation)."""

    def __init__(self, gas, gbs, sensor):
        self._h = C.c_void_p()
        self.gas, self.gbs, self.sensor = gas, gbs, sensor
        check(lib.bf_pipeline_create(C.byref(gas), C.byref(gbs), C.byref(sensor), C.byref(self._h)))

    def close(self):
        if self._h:
            lib.bf_pipeline_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_volume_shard(self, rank, world):
        check(lib.bf_pipeline_set_volume_shard(self._h, rank, world))

    def set_volume_batching(self, enable=True):
        """one bf_scene_run_batch per frame (default) or one operator at a time: bf_pipeline_set_volume_batching"""
        check(lib.bf_pipeline_set_volume_batching(self._h, int(enable)))

    def set_comm(self, comm, capacity_keys=None):
        """Divide the allocation's ray march of every TSDF operator of this loop over the ranks of `comm` (bf_pipeline_set_comm; the volume must be
        sharded with set_volume_shard(rank, world) of the same communicator).  capacity_keys: keys per rank and operator; None sizes it from the integration
        resolution and the voxel size for ONE rank's share being the whole frame (alloc_comm_capacity with world = 1: never too small)."""
        if capacity_keys is None:
            capacity_keys = alloc_comm_capacity(self.gas.s_integrationWidth, self.gas.s_integrationHeight, self.gas.s_SDFVoxelSize, 1)
        check(lib.bf_pipeline_set_comm(self._h, comm._h if comm is not None else None, int(capacity_keys)))
        self._comm = comm

    def set_solve_lag(self, lag):
        """0: the reference's serial order (default).  1..s_submapSize: the chunk solves run on their own thread / stream and are applied exactly `lag`
        frames after the frame that closed the chunk (bf_pipeline_set_solve_lag)."""
        check(lib.bf_pipeline_set_solve_lag(self._h, int(lag)))

    def solve_lag(self):
        n = C.c_uint32()
        check(lib.bf_pipeline_get_solve_lag(self._h, C.byref(n)))
        return n.value

    def process_frame(self, depth, color):
        """depth float32 (H,W), color uint8 (H,W,4): host numpy arrays (PCIe path) or torch cuda tensors (HBM-resident path)."""
        got = C.c_int()
        if isinstance(depth, np.ndarray):
            depth = np.ascontiguousarray(depth, np.float32); color = np.ascontiguousarray(color, np.uint8)
            check(lib.bf_pipeline_process_frame(self._h, depth.ctypes.data_as(C.c_void_p), color.ctypes.data_as(C.c_void_p), C.byref(got)))
        else:
            check(lib.bf_pipeline_process_frame_device(self._h, C.c_void_p(depth.data_ptr()), C.c_void_p(color.data_ptr()), C.byref(got)))
        return bool(got.value)

    def process_frame_raw(self, depth_u16, depth_shift, colour, compression=0, jpeg=None):
        """One iteration of the frame loop with a frame in sensor format (bf_pipeline_process_frame_raw*): arguments as ImageManager.process_raw."""
        got = C.c_int()
        if isinstance(depth_u16, np.ndarray):
            d = np.ascontiguousarray(depth_u16, np.uint16)
            if isinstance(colour, (bytes, bytearray, memoryview)):
                buf = np.frombuffer(colour, np.uint8)
                check(lib.bf_pipeline_process_frame_raw(self._h, d.ctypes.data_as(C.c_void_p), C.c_float(depth_shift), buf.ctypes.data_as(C.c_void_p), C.c_uint64(buf.size),
                                                        int(compression), C.byref(got)))
            else:
                ptr, _keep = _raw_colour(colour, jpeg)
                check(lib.bf_pipeline_process_frame_raw_decoded(self._h, d.ctypes.data_as(C.c_void_p), C.c_float(depth_shift), ptr, C.byref(jpeg) if jpeg is not None else None,
                                                                C.byref(got)))
        else:
            ptr, _keep = _raw_colour(colour, jpeg)
            check(lib.bf_pipeline_process_frame_raw_device(self._h, C.c_void_p(depth_u16.data_ptr()), C.c_float(depth_shift), ptr, C.byref(jpeg) if jpeg is not None else None,
                                                           C.byref(got)))
        return bool(got.value)

    def process_end_of_sequence(self):
        n = C.c_uint32()
        check(lib.bf_pipeline_process_end_of_sequence(self._h, C.byref(n)))
        return n.value

    def synchronize(self):
        check(lib.bf_pipeline_synchronize(self._h))

    def num_frames(self):
        n = C.c_uint32()
        check(lib.bf_pipeline_get_num_frames(self._h, C.byref(n)))
        return n.value

    def integrated_trajectory(self):
        n = self.num_frames()
        out = np.zeros((max(n, 1), 4, 4), np.float32); cnt = C.c_uint32()
        check(lib.bf_pipeline_get_integrated_trajectory(self._h, out.ctypes.data_as(C.c_void_p), n, C.byref(cnt)))
        return out[:cnt.value]

    def optimized_trajectory(self):
        ob = C.c_void_p(); tm = C.c_void_p()
        check(lib.bf_pipeline_get_online_bundler(self._h, C.byref(ob)))
        check(lib.bf_online_bundler_get_trajectory_manager(ob, C.byref(tm)))
        n = self.num_frames()
        out = np.zeros((max(n, 1), 4, 4), np.float32); cnt = C.c_uint32()
        check(lib.bf_trajectory_manager_get_optimized_transforms(tm, out.ctypes.data_as(C.c_void_p), n, C.byref(cnt)))
        return out[:cnt.value]

    def counters(self):
        a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib.bf_pipeline_get_counters(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(integrate=a.value, deintegrate=b.value, local_solves=c.value, global_solves=d.value)

    def host_profile(self, reset=False):
        """Seconds the calling thread spent per part of the frame loop (accumulated) and the frame count: see bf_pipeline_get_host_profile."""
        out = (C.c_double * 8)()
        check(lib.bf_pipeline_get_host_profile(self._h, out, int(reset)))
        names = ("enqueue_match_chain", "ingest_detect_enqueue", "reintegrate_commands", "wait_match_result", "integrate_command", "solves", "wait_ingest", "frames")
        return dict(zip(names, [float(v) for v in out]))

    def volume_thread_profile(self, reset=False):
        b, n = C.c_double(), C.c_double()
        check(lib.bf_pipeline_get_volume_thread_profile(self._h, C.byref(b), C.byref(n), int(reset)))
        return dict(busy_seconds=b.value, operators=n.value)

    def enable_timings(self, on=True):
        check(lib.bf_pipeline_enable_timings(self._h, int(on)))

    def last_timing(self):
        t = FrameTiming()
        check(lib.bf_pipeline_get_last_timing(self._h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in FrameTiming._fields_}

    def set_render_state(self, state):
        check(lib.bf_pipeline_set_render_state(self._h, C.byref(state)))

    def render_size(self, mode=1):
        w, h = C.c_uint32(), C.c_uint32()
        check(lib.bf_pipeline_get_render_size(self._h, int(mode), C.byref(w), C.byref(h)))
        return w.value, h.value

    def render(self, mode=1, camera_to_world=None, tracking_lost=None):
        """bf_pipeline_render: the picture of s_RenderMode `mode` as uint8 (h, w, 4).  camera_to_world None: the pose of the last frame handed to the volume;
        tracking_lost None: from that frame's validity."""
        w, h = self.render_size(mode)
        out = np.zeros((h, w, 4), np.uint8)
        T = None if camera_to_world is None else _f16(camera_to_world)
        check(lib.bf_pipeline_render(self._h, int(mode), T, -1 if tracking_lost is None else int(bool(tracking_lost)), out.ctypes.data_as(C.c_void_p)))
        return out

    def render_top_down(self):
        """bf_pipeline_render_top_down: renderTopDown's reconstruction picture (pose and depth range from the render state's s_topVideo* keys)"""
        w, h = self.render_size(1)
        out = np.zeros((h, w, 4), np.uint8)
        check(lib.bf_pipeline_render_top_down(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def save_mesh(self, filename, transform=None):
        """bf_pipeline_save_mesh: the mesh of everything handed in so far as a PLY, extracted and welded on the device between two frames' batches.
        Returns (vertices, faces, triangles)."""
        nv, nf, nt = C.c_uint32(), C.c_uint32(), C.c_uint32()
        T = mat16(transform) if transform is not None else None
        check(lib.bf_pipeline_save_mesh(self._h, str(filename).encode(), T, C.byref(nv), C.byref(nf), C.byref(nt)))
        return nv.value, nf.value, nt.value

    def save_mesh_clean(self, filename, transform=None, min_faces=0, largest=False, normals=False):
        """bf_pipeline_save_mesh_clean: save_mesh with the mesh cleaned on the device between the weld and the file (components below min_faces faces dropped, only
        the largest kept, per-vertex normals written).  Returns (stats dict, triangles)."""
        p = MeshCleanParams(int(min_faces), int(bool(largest)), int(bool(normals))); st = MeshCleanStats(); nt = C.c_uint32()
        T = mat16(transform) if transform is not None else None
        check(lib.bf_pipeline_save_mesh_clean(self._h, str(filename).encode(), T, C.byref(p), C.byref(st), C.byref(nt)))
        return st.as_dict(), nt.value

    def save_mesh_simplified(self, filename, cell_size, transform=None, min_faces=0, largest=False, normals=False):
        """bf_pipeline_save_mesh_simplified: save_mesh_clean with the cleaned mesh's vertices clustered on a grid of cell_size metres on the device before the file
        is written.  Returns (clean stats dict, simplify stats dict, triangles)."""
        p = MeshCleanParams(int(min_faces), int(bool(largest)), int(bool(normals))); sp = MeshSimplifyParams(float(cell_size), int(bool(normals)))
        st = MeshCleanStats(); sst = MeshSimplifyStats(); nt = C.c_uint32()
        T = mat16(transform) if transform is not None else None
        check(lib.bf_pipeline_save_mesh_simplified(self._h, str(filename).encode(), T, C.byref(p), C.byref(sp), C.byref(st), C.byref(sst), C.byref(nt)))
        return st.as_dict(), sst.as_dict(), nt.value

    def measure_mesh(self, reference, max_distance, direction=0, sample_spacing=0.0, sample_mode=0, cell_size=None, transform=None, min_faces=0, largest=False):
        """bf_pipeline_measure_mesh: the scan's mesh (extracted, welded with the transform, cleaned and - cell_size given - simplified on the device) measured
        against reference = (positions [nv,3] float32, faces [nf,3] uint32) as host arrays; direction 0: the scan against the reference (accuracy), 1: the reference
        against the scan (completeness).  Returns (clean stats dict, simplify stats dict or None, distance stats dict, triangles)."""
        pos, fc = _host_mesh(reference)
        p = MeshCleanParams(int(min_faces), int(bool(largest)), 0); sp = None if cell_size is None else MeshSimplifyParams(float(cell_size), 0)
        dp = MeshDistanceParams(float(max_distance), float(sample_spacing), int(sample_mode))
        st = MeshCleanStats(); sst = MeshSimplifyStats(); dst = MeshDistanceStats(); nt = C.c_uint32()
        T = mat16(transform) if transform is not None else None
        check(lib.bf_pipeline_measure_mesh(self._h, T, C.byref(p), C.byref(sp) if sp is not None else None, pos.ctypes.data_as(C.c_void_p), fc.ctypes.data_as(C.c_void_p),
                                           C.c_uint32(len(pos)), C.c_uint32(len(fc)), C.byref(dp), C.c_int32(int(direction)), C.byref(st), C.byref(sst), C.byref(dst), C.byref(nt)))
        d = dst.as_dict(); d["max_distance"] = float(dp.maxDistance)
        return st.as_dict(), (sst.as_dict() if sp is not None else None), d, nt.value

    def mesh_recolour_defaults(self):
        """bf_pipeline_get_mesh_recolour_defaults: the MeshRecolourParams the pipeline uses where none are given"""
        rp = MeshRecolourParams()
        check(lib.bf_pipeline_get_mesh_recolour_defaults(self._h, C.byref(rp)))
        return rp

    def mesh_recolour_intrinsics(self):
        """bf_pipeline_get_mesh_recolour_intrinsics: the [4,4] intrinsics save_mesh_recoloured projects with"""
        K = (C.c_float * 16)()
        check(lib.bf_pipeline_get_mesh_recolour_intrinsics(self._h, K))
        return np.array(K[:], np.float32).reshape(4, 4)

    def mesh_recolour_frames_host(self, frame_stride=None, transform=None, trajectory=None, images=True):
        """what save_mesh_recoloured takes the colours from, as host arrays: (frames, intrinsics, width, height) with frames = [(depth, colour, meshToCamera,
        cameraCentre, skipped)] of the stored frames 0, stride, 2 * stride, ... that have a valid optimised pose (trajectory None: the current one), camera to mesh
        = transform * pose in binary32 with bf_device.h's product, through bf_mesh_recolour_frame_from_pose.  images False: the frame's number in place of its
        two images, (frame, meshToCamera, cameraCentre, skipped)"""
        stride = int(self.gbs.s_submapSize) if frame_stride is None else int(frame_stride)
        T = self.optimized_trajectory() if trajectory is None else np.asarray(trajectory, np.float32).reshape(-1, 4, 4)
        X = None if transform is None else np.asarray(transform, np.float32).reshape(4, 4)
        frames = []
        for f in range(0, len(T), stride):
            if np.isnan(T[f, 0, 0]) or T[f, 0, 0] == -np.inf:
                continue
            M = T[f]
            if X is not None:
                with np.errstate(all="ignore"):
                    M = ((X[:, 0:1] * M[0:1, :] + X[:, 1:2] * M[1:2, :]) + X[:, 2:3] * M[2:3, :]) + X[:, 3:4] * M[3:4, :]
            frames.append((self.integrate_frame_cpu(f) if images else (f,)) + mesh_recolour_frame_from_pose(M))
        im = C.c_void_p(); w = C.c_uint32(); h = C.c_uint32()
        check(lib.bf_pipeline_get_image_manager(self._h, C.byref(im)))
        check(lib.bf_image_manager_get_integration_size(im, C.byref(w), C.byref(h)))
        return frames, self.mesh_recolour_intrinsics(), w.value, h.value

    def save_mesh_recoloured(self, filename, transform=None, min_faces=0, largest=False, normals=False, params=None, frame_stride=None, cell_size=None):
        """bf_pipeline_save_mesh_recoloured: save_mesh_clean with the cleaned mesh's vertex colours taken on the device from the stored frames on the stride under the
        optimised trajectory, then (cell_size given) the simplification of the recoloured mesh.  params None: mesh_recolour_defaults(); frame_stride None:
        s_submapSize (the key frames).  Returns (clean stats dict, recolour stats dict, simplify stats dict or None, triangles)."""
        p = MeshCleanParams(int(min_faces), int(bool(largest)), int(bool(normals)))
        sp = None if cell_size is None else MeshSimplifyParams(float(cell_size), int(bool(normals)))
        st = MeshCleanStats(); rst = MeshRecolourStats(); sst = MeshSimplifyStats(); nt = C.c_uint32()
        T = mat16(transform) if transform is not None else None
        stride = int(self.gbs.s_submapSize) if frame_stride is None else int(frame_stride)
        check(lib.bf_pipeline_save_mesh_recoloured(self._h, str(filename).encode(), T, C.byref(p), None if params is None else C.byref(params), stride,
                                                   None if sp is None else C.byref(sp), C.byref(st), C.byref(rst), C.byref(sst), C.byref(nt)))
        return st.as_dict(), rst.as_dict(), (None if sp is None else sst.as_dict()), nt.value

    def mesh_texture_defaults(self):
        """bf_pipeline_get_mesh_texture_defaults: the MeshTextureParams the pipeline uses where none are given"""
        tp = MeshTextureParams()
        check(lib.bf_pipeline_get_mesh_texture_defaults(self._h, C.byref(tp)))
        return tp

    def save_mesh_textured(self, filename, transform=None, min_faces=0, largest=False, normals=False, params=None, frame_stride=None, recolour_first=False, cell_size=None):
        """bf_pipeline_save_mesh_textured: save_mesh_clean, then (recolour_first) the recolouring with the pipeline's defaults, then (cell_size given) the
        simplification, then the texture atlas of the mesh that is written from the stored frames on the stride: the PLY at filename and the atlas as a PNG next
        to it (the extension replaced by .png).  params None: mesh_texture_defaults(); frame_stride None: s_submapSize.  Returns (clean stats dict, recolour stats
        dict or None, simplify stats dict or None, texture stats dict, triangles)."""
        p = MeshCleanParams(int(min_faces), int(bool(largest)), int(bool(normals)))
        sp = None if cell_size is None else MeshSimplifyParams(float(cell_size), int(bool(normals)))
        st = MeshCleanStats(); rst = MeshRecolourStats(); sst = MeshSimplifyStats(); tst = MeshTextureStats(); nt = C.c_uint32()
        T = mat16(transform) if transform is not None else None
        stride = int(self.gbs.s_submapSize) if frame_stride is None else int(frame_stride)
        check(lib.bf_pipeline_save_mesh_textured(self._h, str(filename).encode(), T, C.byref(p), None if params is None else C.byref(params), stride, int(bool(recolour_first)),
                                                 None if sp is None else C.byref(sp), C.byref(st), C.byref(rst), C.byref(sst), C.byref(tst), C.byref(nt)))
        return st.as_dict(), (rst.as_dict() if recolour_first else None), (None if sp is None else sst.as_dict()), tst.as_dict(), nt.value

    def save_point_cloud(self, filename, frame_stride=None, cell_size=0.005, max_depth=3.5, max_points=0):
        """bf_pipeline_save_point_cloud: the stored frames on the stride under the optimised trajectory as a thinned point cloud PLY, built on the device.
        frame_stride None: s_submapSize (the key frames).  Returns (points, frames used)."""
        n, used = C.c_uint32(), C.c_uint32()
        stride = int(self.gbs.s_submapSize) if frame_stride is None else int(frame_stride)
        check(lib.bf_pipeline_save_point_cloud(self._h, str(filename).encode(), stride, C.c_float(cell_size), C.c_float(max_depth), int(max_points), C.byref(n), C.byref(used)))
        return n.value, used.value

    def set_record_state(self, state, threads=0, tmp_prefix=None):
        """bf_pipeline_set_record_state: before the first frame; with state.s_recordData every accepted frame is recorded (include/bf_record.h)"""
        check(lib.bf_pipeline_set_record_state(self._h, C.byref(state), int(threads), str(tmp_prefix).encode() if tmp_prefix is not None else None))

    def save_recording(self, filename=None, overwrite=False):
        """bf_pipeline_save_recording: the recorded frames that have an optimised pose, as a .sens.  filename None: s_recordDataFile.  Returns (name written, frames)."""
        name = C.create_string_buffer(4096); n = C.c_uint64()
        check(lib.bf_pipeline_save_recording(self._h, str(filename).encode() if filename is not None else None, int(bool(overwrite)), name, C.c_uint64(len(name)), C.byref(n)))
        return name.value.decode(), n.value

    def scene(self):
        """Borrowed SceneRepHashSDF view of the pipeline's voxel-hash volume."""
        h = C.c_void_p()
        check(lib.bf_pipeline_get_scene(self._h, C.byref(h)))
        s = SceneRepHashSDF.__new__(SceneRepHashSDF)
        s._h = h; s._borrowed = True
        hp = HashParams(); check(lib.bf_scene_get_hash_params(h, C.byref(hp))); s.params = hp
        return s

    def process_frame_chunked(self, depth, color, package, local_idx):
        """One iteration for the next frame of the stream with its chunk-local half taken from `package` (a ChunkWorker.run result,
        possibly of another rank): depth / colour are torch cuda tensors, package a contiguous uint8 numpy array."""
        got = C.c_int()
        check(lib.bf_pipeline_process_frame_chunked(self._h, C.c_void_p(depth.data_ptr()), C.c_void_p(color.data_ptr()),
                                                    package.ctypes.data_as(C.c_void_p), C.c_uint64(package.nbytes), int(local_idx), C.byref(got)))
        return bool(got.value)

    def integrate_frame_cpu(self, frame):
        """Host copies (depth float32 (h,w), colour uint8 (h,w,4)) of the frame stored for integration — getIntegrateFrame(i).getDepthFrameCPU() / getColorFrameCPU()."""
        im = C.c_void_p(); w = C.c_uint32(); h = C.c_uint32()
        check(lib.bf_pipeline_get_image_manager(self._h, C.byref(im)))
        check(lib.bf_image_manager_get_integration_size(im, C.byref(w), C.byref(h)))
        d = np.zeros((h.value, w.value), np.float32); c = np.zeros((h.value, w.value, 4), np.uint8)
        check(lib.bf_image_manager_get_integrate_frame_cpu(im, frame, d.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)))
        return d, c

    def camera_calibration(self):
        """whether the loop registers depth to the colour camera: gas.s_bUseCameraCalibration and a sensor with non-identity depth extrinsics"""
        im = C.c_void_p(); a = C.c_int()
        check(lib.bf_pipeline_get_image_manager(self._h, C.byref(im)))
        check(lib.bf_image_manager_get_camera_calibration(im, C.byref(a)))
        return bool(a.value)

    def bundler(self, which):
        ob = C.c_void_p(); b = C.c_void_p()
        check(lib.bf_pipeline_get_online_bundler(self._h, C.byref(ob)))
        check(lib.bf_online_bundler_get_bundler(ob, {"local": 0, "optLocal": 1, "global": 2}[which], C.byref(b)))
        return b

    def initialize_correspondence_evaluator(self, complete_trajectory, log_prefix=None):
        """OnlineBundler.cpp:81-90: evaluate the global key-frame matches against a reference trajectory (one 4x4 per INPUT frame)."""
        ob = C.c_void_p()
        check(lib.bf_pipeline_get_online_bundler(self._h, C.byref(ob)))
        t = np.ascontiguousarray(complete_trajectory, np.float32).reshape(-1, 16)
        check(lib.bf_online_bundler_initialize_correspondence_evaluator(ob, t.ctypes.data_as(C.POINTER(C.c_float)), len(t), (log_prefix or "").encode()))

    def finish_correspondence_evaluator_logging(self):
        ob = C.c_void_p()
        check(lib.bf_pipeline_get_online_bundler(self._h, C.byref(ob)))
        check(lib.bf_online_bundler_finish_correspondence_evaluator_logging(ob))

    def correspondence_evaluator(self):
        h = C.c_void_p()
        check(lib.bf_bundler_get_correspondence_evaluator(self.bundler("global"), C.byref(h)))
        return CorrespondenceEvaluator(handle=h) if h else None


class ChunkWorker:
    """Python view of `bf_chunk_worker`: the chunk-local half of the frame loop (SIFT, matching + filters inside the chunk, local
    solve, key-frame fusion) for one local chunk at a time -> a flat package (numpy uint8) for Pipeline.process_frame_chunked."""

    def __init__(self, gas, gbs, sensor):
        self._h = C.c_void_p()
        check(lib.bf_chunk_worker_create(C.byref(gas), C.byref(gbs), C.byref(sensor), C.byref(self._h)))
        n = C.c_uint64()
        check(lib.bf_chunk_worker_package_bytes(self._h, C.byref(n)))
        self.package_bytes = int(n.value)

    def close(self):
        if self._h:
            lib.bf_chunk_worker_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, chunk_index, frames, out=None):
        """frames: list of (depth, colour) torch cuda tensors, the chunk's frames in stream order (the first one is shared with the
        previous chunk).  Returns the package (uint8 numpy array of package_bytes)."""
        n = len(frames)
        dp = (C.c_void_p * n)(*[f[0].data_ptr() for f in frames])
        cp = (C.c_void_p * n)(*[f[1].data_ptr() for f in frames])
        pkg = out if out is not None else np.zeros(self.package_bytes, np.uint8)
        check(lib.bf_chunk_worker_run(self._h, int(chunk_index), n, dp, cp, pkg.ctypes.data_as(C.c_void_p)))
        return pkg


# --------------------------------------------------------------------------- marching cubes
class MarchingCubesParams(C.Structure):
    _fields_ = [("m_maxNumTriangles", C.c_uint32), ("m_sdfBlockSize", C.c_uint32), ("m_hashNumBuckets", C.c_uint32), ("m_hashBucketSize", C.c_uint32),
                ("m_threshMarchingCubes", C.c_float), ("m_threshMarchingCubes2", C.c_float)]


def marching_cubes_tables():
    """The generated case tables: (edgeTable[256] uint16, triTable[256,16] int8).  Host-only."""
    e = np.zeros(256, np.uint16); t = np.zeros(256 * 16, np.int8)
    check(lib.bf_marching_cubes_tables(e.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)))
    return e, t.reshape(256, 16)


class MarchingCubesHashSDF:
    """Python view of `bf_marching_cubes` (== the reference's CUDAMarchingCubesHashSDF)."""

    def __init__(self, max_triangles, num_buckets, voxel_size, thresh_factor=10.0):
        p = MarchingCubesParams(max_triangles, SDF_BLOCK_SIZE, num_buckets, HASH_BUCKET_SIZE, thresh_factor * voxel_size, thresh_factor * voxel_size)
        self.params = p
        self._h = C.c_void_p()
        check(lib.bf_marching_cubes_create(C.byref(p), C.byref(self._h)))

    def close(self):
        if self._h:
            lib.bf_marching_cubes_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def extract(self, scene, box=None):
        """extractIsoSurface over `scene` (a SceneRepHashSDF): returns (triangles [n,3,6] float32 = position + colour per vertex, number found)"""
        hd = scene.hash_data(); hp = scene.hash_params()
        mn = (C.c_float * 3)(*(box[0] if box else (0, 0, 0))); mx = (C.c_float * 3)(*(box[1] if box else (0, 0, 0)))
        check(lib.bf_marching_cubes_clear_mesh_buffer(self._h))
        check(lib.bf_marching_cubes_extract(self._h, C.byref(hd), C.byref(hp), mn, mx, int(box is not None)))
        n = C.c_uint32(); found = C.c_uint32()
        check(lib.bf_marching_cubes_get_triangles_gpu(self._h, None, C.byref(n), C.byref(found)))
        out = np.zeros((n.value, 3, 6), np.float32); cnt = C.c_uint32()
        check(lib.bf_marching_cubes_get_mesh(self._h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(cnt)))
        return out, found.value

    def save_mesh(self, filename, transform=None):
        nv = C.c_uint32(); nf = C.c_uint32()
        T = mat16(transform) if transform is not None else None
        check(lib.bf_marching_cubes_save_mesh(self._h, str(filename).encode(), T, C.byref(nv), C.byref(nf)))
        return nv.value, nf.value

    # ---- MI355X additions: the mesh without the triangles leaving HBM (csrc/meshweld.hip)
    @classmethod
    def from_global_app_state(cls, gas, max_triangles=0, thresh_factor=10.0):
        """parametersFromGlobalAppState: the thresholds are thresh_factor * s_SDFVoxelSize in binary32, as bf_pipeline_save_mesh computes them.  max_triangles 0: every
        extraction sizes the triangle buffer to the volume."""
        self = cls.__new__(cls)
        th = float(np.float32(thresh_factor) * np.float32(gas.s_SDFVoxelSize))
        self.params = MarchingCubesParams(max_triangles, SDF_BLOCK_SIZE, gas.s_hashNumBuckets, HASH_BUCKET_SIZE, th, th)
        self._h = C.c_void_p()
        check(lib.bf_marching_cubes_create(C.byref(self.params), C.byref(self._h)))
        return self

    def triangles_gpu(self):
        """(device pointer, triangles written, triangles the volume holds) of the last extraction"""
        ptr = C.c_void_p(); n = C.c_uint32(); found = C.c_uint32()
        check(lib.bf_marching_cubes_get_triangles_gpu(self._h, C.byref(ptr), C.byref(n), C.byref(found)))
        return ptr.value, n.value, found.value

    def extract_gpu(self, scene, box=None):
        """extract without the host copy (the host mesh buffer keeps what it held): returns (triangles written, triangles the volume holds)"""
        hd = scene.hash_data(); hp = scene.hash_params()
        mn = (C.c_float * 3)(*(box[0] if box else (0, 0, 0))); mx = (C.c_float * 3)(*(box[1] if box else (0, 0, 0)))
        check(lib.bf_marching_cubes_extract_gpu(self._h, C.byref(hd), C.byref(hp), mn, mx, int(box is not None)))
        _, n, found = self.triangles_gpu()
        return n, found

    def download_triangles(self):
        """host copy of the last extraction's device buffer, [n, 3, 6] float32"""
        ptr, n, _ = self.triangles_gpu()
        out = np.zeros((n, 3, 6), np.float32)
        if n:
            check(lib.bf_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes)))
        return out

    def weld(self, triangles=None, transform=None):
        """bf_marching_cubes_weld + download: (positions [nv,3] float32, colours [nv,3] float32, faces [nf,3] uint32).  triangles: a contiguous float32 torch cuda
        tensor [T,3,6], or None for the last extraction."""
        m = IndexedMesh()
        T = mat16(transform) if transform is not None else None
        if triangles is None:
            check(lib.bf_marching_cubes_weld(self._h, None, 0, T, C.byref(m)))
        else:
            assert triangles.is_contiguous() and triangles.numel() % 18 == 0
            check(lib.bf_marching_cubes_weld(self._h, C.c_void_p(triangles.data_ptr()), triangles.numel() // 18, T, C.byref(m)))
        pos = np.zeros((m.numVertices, 3), np.float32); col = np.zeros((m.numVertices, 3), np.float32); faces = np.zeros((m.numFaces, 3), np.uint32)
        check(lib.bf_marching_cubes_download_indexed(self._h, pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), faces.ctypes.data_as(C.c_void_p)))
        return pos, col, faces

    def save_mesh_gpu(self, filename, transform=None):
        """weld of the last extraction on the device + PLY: (vertices, faces)"""
        nv = C.c_uint32(); nf = C.c_uint32()
        T = mat16(transform) if transform is not None else None
        check(lib.bf_marching_cubes_save_mesh_gpu(self._h, str(filename).encode(), T, C.byref(nv), C.byref(nf)))
        return nv.value, nf.value


    # ---- MI355X additions: the indexed mesh cleaned in HBM (csrc/meshclean.hip)
    def clean(self, mesh=None, min_faces=0, largest=False, normals=False):
        """bf_marching_cubes_clean + download: (positions, colours, normals or None, faces, stats dict).  mesh: (positions [nv,3] float32, colours [nv,3] float32,
        faces [nf,3] uint32) as contiguous torch cuda tensors, or None for the last weld."""
        p = MeshCleanParams(int(min_faces), int(bool(largest)), int(bool(normals)))
        out = CleanMesh(); st = MeshCleanStats()
        if mesh is None:
            check(lib.bf_marching_cubes_clean(self._h, None, C.byref(p), C.byref(out), C.byref(st)))
        else:
            pos, col, faces = mesh
            assert pos.is_contiguous() and col.is_contiguous() and faces.is_contiguous() and pos.numel() == col.numel() and pos.numel() % 3 == 0 and faces.numel() % 3 == 0
            m = IndexedMesh(pos.data_ptr() or None, col.data_ptr() or None, faces.data_ptr() or None, pos.numel() // 3, faces.numel() // 3)
            check(lib.bf_marching_cubes_clean(self._h, C.byref(m), C.byref(p), C.byref(out), C.byref(st)))
        nv, nf = out.numVertices, out.numFaces
        hp = np.zeros((nv, 3), np.float32); hc = np.zeros((nv, 3), np.float32); hf = np.zeros((nf, 3), np.uint32)
        hn = np.zeros((nv, 3), np.float32) if normals else None
        check(lib.bf_marching_cubes_download_clean(self._h, hp.ctypes.data_as(C.c_void_p), hc.ctypes.data_as(C.c_void_p), hn.ctypes.data_as(C.c_void_p) if normals else None,
                                                   hf.ctypes.data_as(C.c_void_p)))
        return hp, hc, hn, hf, st.as_dict()

    def clean_labels(self, num_vertices):
        """the component label of the first num_vertices input vertices of the last clean (uint32)"""
        out = np.zeros(int(num_vertices), np.uint32)
        check(lib.bf_marching_cubes_clean_labels(self._h, out.ctypes.data_as(C.c_void_p), len(out)))
        return out

    def save_mesh_clean(self, filename, transform=None, min_faces=0, largest=False, normals=False):
        """weld of the last extraction + clean on the device + PLY (with normals: bf_write_ply_indexed_normals): the stats dict"""
        p = MeshCleanParams(int(min_faces), int(bool(largest)), int(bool(normals))); st = MeshCleanStats()
        T = mat16(transform) if transform is not None else None
        check(lib.bf_marching_cubes_save_mesh_clean(self._h, str(filename).encode(), T, C.byref(p), C.byref(st)))
        return st.as_dict()

    # ---- MI355X additions: the indexed mesh simplified in HBM by vertex clustering (csrc/meshsimplify.hip)
    def simplify(self, mesh=None, cell_size=0.01, normals=False):
        """bf_marching_cubes_simplify + download: (positions, colours, normals or None, faces, stats dict).  mesh: (positions [nv,3] float32, colours [nv,3] float32,
        faces [nf,3] uint32) as contiguous torch cuda tensors, or None for the result of the last clean."""
        p = MeshSimplifyParams(float(cell_size), int(bool(normals)))
        out = CleanMesh(); st = MeshSimplifyStats()
        if mesh is None:
            check(lib.bf_marching_cubes_simplify(self._h, None, C.byref(p), C.byref(out), C.byref(st)))
        else:
            pos, col, faces = mesh
            assert pos.is_contiguous() and col.is_contiguous() and faces.is_contiguous() and pos.numel() == col.numel() and pos.numel() % 3 == 0 and faces.numel() % 3 == 0
            m = IndexedMesh(pos.data_ptr() or None, col.data_ptr() or None, faces.data_ptr() or None, pos.numel() // 3, faces.numel() // 3)
            check(lib.bf_marching_cubes_simplify(self._h, C.byref(m), C.byref(p), C.byref(out), C.byref(st)))
        return self.download_simplified(out.numVertices, out.numFaces, normals) + (st.as_dict(),)

    def download_simplified(self, nv, nf, normals=False):
        """bf_marching_cubes_download_simplified: (positions, colours, normals or None, faces) of the last simplify, whose counts the caller knows"""
        hp = np.zeros((nv, 3), np.float32); hc = np.zeros((nv, 3), np.float32); hf = np.zeros((nf, 3), np.uint32)
        hn = np.zeros((nv, 3), np.float32) if normals else None
        check(lib.bf_marching_cubes_download_simplified(self._h, hp.ctypes.data_as(C.c_void_p), hc.ctypes.data_as(C.c_void_p), hn.ctypes.data_as(C.c_void_p) if normals else None,
                                                        hf.ctypes.data_as(C.c_void_p)))
        return hp, hc, hn, hf

    def simplify_map(self, num_vertices):
        """per input vertex of the last simplify (the first num_vertices of them) its output id, or 0xFFFFFFFF where its cluster is not in the output (uint32)"""
        out = np.zeros(int(num_vertices), np.uint32)
        check(lib.bf_marching_cubes_simplify_map(self._h, out.ctypes.data_as(C.c_void_p), len(out)))
        return out

    def save_mesh_simplified(self, filename, cell_size, transform=None, min_faces=0, largest=False, normals=False):
        """weld of the last extraction + clean + simplify on the device + PLY (with normals: bf_write_ply_indexed_normals): (clean stats dict, simplify stats dict)"""
        p = MeshCleanParams(int(min_faces), int(bool(largest)), int(bool(normals))); sp = MeshSimplifyParams(float(cell_size), int(bool(normals)))
        st = MeshCleanStats(); sst = MeshSimplifyStats()
        T = mat16(transform) if transform is not None else None
        check(lib.bf_marching_cubes_save_mesh_simplified(self._h, str(filename).encode(), T, C.byref(p), C.byref(sp), C.byref(st), C.byref(sst)))
        return st.as_dict(), sst.as_dict()

    # ---- MI355X additions: the distance of a mesh to a reference surface in HBM (csrc/meshdistance.hip)
    def distance(self, a, b, max_distance, sample_spacing=0.0, sample_mode=0, download=True):
        """bf_marching_cubes_distance (+ download): (distance float64, nearest face uint32, weight float64, stats dict), or the stats dict alone without download.
        a, b: (positions [nv,3] float32, faces [nf,3] uint32) as contiguous torch cuda tensors; a None: the result of the latest of the object's simplify, clean
        and weld.  Mesh a is sampled (sample_mode 0: its vertices; 1: its surface every sample_spacing metres) and measured against the surface b."""
        p = MeshDistanceParams(float(max_distance), float(sample_spacing), int(sample_mode)); st = MeshDistanceStats()
        keep = []

        def mesh(m):
            pos, faces = m
            assert pos.is_contiguous() and faces.is_contiguous() and pos.numel() % 3 == 0 and faces.numel() % 3 == 0
            keep.append(m)
            return IndexedMesh(pos.data_ptr() or None, None, faces.data_ptr() or None, pos.numel() // 3, faces.numel() // 3)
        mb = mesh(b)
        ma = mesh(a) if a is not None else None
        check(lib.bf_marching_cubes_distance(self._h, C.byref(ma) if ma is not None else None, C.byref(mb), C.byref(p), C.byref(st)))
        d = st.as_dict(); d["max_distance"] = float(p.maxDistance)
        return self.download_distance(d["numSamples"]) + (d,) if download else d

    def download_distance(self, num_samples):
        """bf_marching_cubes_download_distance: (distance, nearest face, weight) of the first num_samples samples of the last measurement"""
        n = int(num_samples)
        hd = np.zeros(n, np.float64); hf = np.zeros(n, np.uint32); hw = np.zeros(n, np.float64)
        check(lib.bf_marching_cubes_download_distance(self._h, hd.ctypes.data_as(C.c_void_p), hf.ctypes.data_as(C.c_void_p), hw.ctypes.data_as(C.c_void_p), C.c_uint32(n)))
        return hd, hf, hw

    # ---- MI355X additions: the mesh's vertex colours taken from the key frames in HBM (csrc/meshrecolour.hip)
    def recolour(self, mesh, frames, width, height, intrinsics, params):
        """bf_marching_cubes_recolour + download: (colours [nv,3] float32, views [nv] uint32, stats dict).  mesh: (positions, colours, normals, faces) as contiguous
        torch cuda tensors (faces may be None), or None for the last clean (or the last simplify if later); frames: a recolour_frames() array whose images are
        device pointers; params: a MeshRecolourParams."""
        out = CleanMesh(); st = MeshRecolourStats()
        K = mat16(intrinsics)
        if mesh is None:
            check(lib.bf_marching_cubes_recolour(self._h, None, frames, len(frames), int(width), int(height), K, C.byref(params), C.byref(out), C.byref(st)))
        else:
            pos, col, nrm, faces = mesh
            assert pos.is_contiguous() and col.is_contiguous() and (nrm is None or nrm.is_contiguous()) and pos.numel() == col.numel() and pos.numel() % 3 == 0
            m = CleanMesh(pos.data_ptr() or None, col.data_ptr() or None, None if nrm is None else (nrm.data_ptr() or None), None if faces is None else (faces.data_ptr() or None),
                          pos.numel() // 3, 0 if faces is None else faces.numel() // 3)
            check(lib.bf_marching_cubes_recolour(self._h, C.byref(m), frames, len(frames), int(width), int(height), K, C.byref(params), C.byref(out), C.byref(st)))
        self._recoloured = out
        return self.download_recoloured(out.numVertices, 0)[1], self.recolour_views(out.numVertices), st.as_dict()

    def simplify_recoloured(self, cell_size=0.01, normals=False):
        """bf_marching_cubes_simplify of the last recolour's mesh (its own colour array as the input's colours) + download, as simplify()"""
        r = self._recoloured
        m = IndexedMesh(r.d_positions, r.d_colors, r.d_faces, r.numVertices, r.numFaces)
        p = MeshSimplifyParams(float(cell_size), int(bool(normals))); out = CleanMesh(); st = MeshSimplifyStats()
        check(lib.bf_marching_cubes_simplify(self._h, C.byref(m), C.byref(p), C.byref(out), C.byref(st)))
        return self.download_simplified(out.numVertices, out.numFaces, normals) + (st.as_dict(),)

    def download_recoloured(self, nv, nf, normals=False):
        """bf_marching_cubes_download_recoloured: (positions, colours, normals or None, faces) of the last recolour, whose counts the caller knows"""
        hp = np.zeros((nv, 3), np.float32); hc = np.zeros((nv, 3), np.float32); hf = np.zeros((nf, 3), np.uint32)
        hn = np.zeros((nv, 3), np.float32) if normals else None
        check(lib.bf_marching_cubes_download_recoloured(self._h, hp.ctypes.data_as(C.c_void_p), hc.ctypes.data_as(C.c_void_p), hn.ctypes.data_as(C.c_void_p) if normals else None,
                                                        hf.ctypes.data_as(C.c_void_p) if nf else None))
        return hp, hc, hn, hf

    def recolour_views(self, num_vertices):
        """the number of views of the first num_vertices vertices of the last recolour (uint32)"""
        out = np.zeros(int(num_vertices), np.uint32)
        check(lib.bf_marching_cubes_recolour_views(self._h, out.ctypes.data_as(C.c_void_p), len(out)))
        return out

    def save_mesh_recoloured(self, filename, frames, width, height, intrinsics, params, transform=None, min_faces=0, largest=False, normals=False, cell_size=None):
        """weld of the last extraction + clean + recolour (+ simplify on a grid of cell_size, if given) on the device + PLY: (clean stats dict, recolour stats dict,
        simplify stats dict or None).  The frames' poses are camera to mesh: the transform already applied."""
        p = MeshCleanParams(int(min_faces), int(bool(largest)), int(bool(normals)))
        sp = None if cell_size is None else MeshSimplifyParams(float(cell_size), int(bool(normals)))
        st = MeshCleanStats(); rst = MeshRecolourStats(); sst = MeshSimplifyStats()
        T = mat16(transform) if transform is not None else None
        check(lib.bf_marching_cubes_save_mesh_recoloured(self._h, str(filename).encode(), T, C.byref(p), frames, len(frames), int(width), int(height), mat16(intrinsics), C.byref(params),
                                                         None if sp is None else C.byref(sp), C.byref(st), C.byref(rst), C.byref(sst)))
        return st.as_dict(), rst.as_dict(), (None if sp is None else sst.as_dict())

    # ---- MI355X additions: a texture atlas for the mesh from the key frames in HBM (csrc/meshtexture.hip)
    def texture(self, mesh, frames, width, height, intrinsics, params):
        """bf_marching_cubes_texture + download: (atlas [H,A,4] uint8, faceFrame [nf] int32, faceUV [nf,6] float32, stats dict).  mesh: (positions, colours, faces) as
        contiguous torch cuda tensors, or None for the last clean (or the last simplify if later); frames: a recolour_frames() array whose images are device
        pointers; params: a MeshTextureParams."""
        st = MeshTextureStats()
        K = mat16(intrinsics)
        if mesh is None:
            check(lib.bf_marching_cubes_texture(self._h, None, frames, len(frames), int(width), int(height), K, C.byref(params), C.byref(st)))
        else:
            pos, col, faces = mesh
            assert pos.is_contiguous() and col.is_contiguous() and faces.is_contiguous() and pos.numel() == col.numel() and pos.numel() % 3 == 0 and faces.numel() % 3 == 0
            m = CleanMesh(pos.data_ptr() or None, col.data_ptr() or None, None, faces.data_ptr() or None, pos.numel() // 3, faces.numel() // 3)
            check(lib.bf_marching_cubes_texture(self._h, C.byref(m), frames, len(frames), int(width), int(height), K, C.byref(params), C.byref(st)))
        return self.download_texture(st.atlasWidth, st.atlasHeight, st.numFaces) + (st.as_dict(),)

    def download_texture(self, atlas_width, atlas_height, nf):
        """bf_marching_cubes_download_texture: (atlas, faceFrame, faceUV) of the last texture, whose sizes the caller knows"""
        atlas = np.zeros((atlas_height, atlas_width, 4), np.uint8); ff = np.zeros(nf, np.int32); uv = np.zeros((nf, 6), np.float32)
        check(lib.bf_marching_cubes_download_texture(self._h, atlas.ctypes.data_as(C.c_void_p), ff.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p)))
        return atlas, ff, uv

    def save_mesh_textured(self, filename, frames, width, height, intrinsics, params, transform=None, min_faces=0, largest=False, normals=False, recolour_params=None, cell_size=None):
        """weld of the last extraction + clean (+ recolour with recolour_params, + simplify on a grid of cell_size) + texture on the device + the PLY and the PNG
        next to it: (clean stats dict, recolour stats dict or None, simplify stats dict or None, texture stats dict).  The frames' poses are camera to mesh: the
        transform already applied."""
        p = MeshCleanParams(int(min_faces), int(bool(largest)), int(bool(normals)))
        sp = None if cell_size is None else MeshSimplifyParams(float(cell_size), int(bool(normals)))
        st = MeshCleanStats(); rst = MeshRecolourStats(); sst = MeshSimplifyStats(); tst = MeshTextureStats()
        T = mat16(transform) if transform is not None else None
        check(lib.bf_marching_cubes_save_mesh_textured(self._h, str(filename).encode(), T, C.byref(p), frames, len(frames), int(width), int(height), mat16(intrinsics), C.byref(params),
                                                       None if recolour_params is None else C.byref(recolour_params), None if sp is None else C.byref(sp), C.byref(st), C.byref(rst),
                                                       C.byref(sst), C.byref(tst)))
        return st.as_dict(), (None if recolour_params is None else rst.as_dict()), (None if sp is None else sst.as_dict()), tst.as_dict()


class MeshTextureParams(C.Structure):
    _fields_ = [("depthMin", C.c_float), ("depthMax", C.c_float), ("depthTolerance", C.c_float), ("depthToleranceLin", C.c_float), ("minCos", C.c_float), ("patchSize", C.c_uint32),
                ("atlasWidth", C.c_uint32)]


class MeshTextureStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("numFaces", "numFacesTextured", "numFacesUntextured", "numFramesUsed", "numFramesSkipped", "atlasWidth", "atlasHeight")] + \
               [(n, C.c_uint64) for n in ("numTexelsFromFrames", "numTexelsFromVertices", "numTexelsUnused")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def mesh_texture_atlas_height(num_faces, params):
    """bf_mesh_texture_atlas_height: the atlas height of the layout for num_faces faces.  Host-only."""
    h = C.c_uint32()
    check(lib.bf_mesh_texture_atlas_height(int(num_faces), C.byref(params), C.byref(h)))
    return h.value


def mesh_texture_host(positions, colors, faces, frames, width, height, intrinsics, params):
    """bf_mesh_texture_host, the definition on one core: (atlas [H,A,4] uint8, faceFrame [nf] int32, faceUV [nf,6] float32, stats dict).  frames: (depth [h,w]
    float32, colour [h,w,4] uint8, meshToCamera, cameraCentre, skipped) tuples of host arrays.  Host-only."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); col = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    fc = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    keep = [(np.ascontiguousarray(d, np.float32), np.ascontiguousarray(c, np.uint8)) for d, c, _, _, _ in frames]
    for d, c in keep:
        assert d.shape == (height, width) and c.shape == (height, width, 4)
    fr = recolour_frames([(d.ctypes.data, c.ctypes.data, W, o, s) for (d, c), (_, _, W, o, s) in zip(keep, frames)])
    st = MeshTextureStats()
    K = mat16(intrinsics)
    atlas = np.zeros((mesh_texture_atlas_height(len(fc), params), int(params.atlasWidth), 4), np.uint8); ff = np.zeros(len(fc), np.int32); uv = np.zeros((len(fc), 6), np.float32)
    check(lib.bf_mesh_texture_host(pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), fc.ctypes.data_as(C.c_void_p), len(pos), len(fc), fr, len(frames), int(width), int(height), K,
                                   C.byref(params), atlas.ctypes.data_as(C.c_void_p), ff.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p), C.byref(st)))
    return atlas, ff, uv, st.as_dict()


def write_ply_textured(filename, texture_name, positions, normals, colors, faces, face_uv):
    """bf_write_ply_textured: the PLY of an indexed mesh with per-face texture coordinates ([nf,6] float32) into the picture texture_name.  Host-only."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); col = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    fc = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3); uv = np.ascontiguousarray(face_uv, np.float32).reshape(-1, 6)
    assert len(uv) == len(fc) and len(col) == len(pos) and (nrm is None or len(nrm) == len(pos))
    check(lib.bf_write_ply_textured(str(filename).encode(), str(texture_name).encode(), pos.ctypes.data_as(C.c_void_p), None if nrm is None else nrm.ctypes.data_as(C.c_void_p),
                                    col.ctypes.data_as(C.c_void_p), fc.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p), len(pos), len(fc)))


class MeshRecolourParams(C.Structure):
    _fields_ = [("depthMin", C.c_float), ("depthMax", C.c_float), ("depthTolerance", C.c_float), ("depthToleranceLin", C.c_float), ("minCos", C.c_float), ("mode", C.c_int32)]


class MeshRecolourStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("numVertices", "numRecoloured", "numUnseen", "numFramesUsed", "numFramesSkipped", "maxViews")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class MeshRecolourFrame(C.Structure):
    _fields_ = [("d_depth", C.c_void_p), ("d_colorRGBX", C.c_void_p), ("meshToCamera", C.c_float * 16), ("cameraCentre", C.c_float * 3), ("skipped", C.c_int32)]


# the rule codes of a (vertex, frame) pair, BF_RECOLOUR_* (the first rule that fails; 0: a view)
RECOLOUR_CODES = ("VIEW", "NORMAL", "RANGE", "IMAGE", "FACING", "OCCLUDED", "COLOUR")


def mesh_recolour_frame_from_pose(camera_to_mesh):
    """bf_mesh_recolour_frame_from_pose: (meshToCamera [4,4] float32, cameraCentre [3] float32, skipped).  Host-only."""
    f = MeshRecolourFrame()
    check(lib.bf_mesh_recolour_frame_from_pose(mat16(camera_to_mesh), C.byref(f)))
    return np.array(f.meshToCamera[:], np.float32).reshape(4, 4), np.array(f.cameraCentre[:], np.float32), bool(f.skipped)


def recolour_frames(frames):
    """a ctypes array of bf_mesh_recolour_frame from (depth pointer, colour pointer, meshToCamera, cameraCentre, skipped) tuples; the pointers are integers (device
    pointers for the device route, host pointers for mesh_recolour_host) or None"""
    arr = (MeshRecolourFrame * len(frames))()
    for k, (d, c, W, o, skipped) in enumerate(frames):
        arr[k].d_depth = d; arr[k].d_colorRGBX = c; arr[k].skipped = int(bool(skipped))
        arr[k].meshToCamera[:] = np.asarray(W, np.float32).reshape(16).tolist(); arr[k].cameraCentre[:] = np.asarray(o, np.float32).reshape(3).tolist()
    return arr


def mesh_recolour_host(positions, normals, colors, frames, width, height, intrinsics, params, codes=False):
    """bf_mesh_recolour_host, the definition on one core: (colours, views, stats dict[, codes [nv, K] uint8]).  frames: (depth [h,w] float32, colour [h,w,4] uint8,
    meshToCamera, cameraCentre, skipped) tuples of host arrays.  Host-only."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); col = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    keep = [(np.ascontiguousarray(d, np.float32), np.ascontiguousarray(c, np.uint8)) for d, c, _, _, _ in frames]
    for d, c in keep:
        assert d.shape == (height, width) and c.shape == (height, width, 4)
    fr = recolour_frames([(d.ctypes.data, c.ctypes.data, W, o, s) for (d, c), (_, _, W, o, s) in zip(keep, frames)])
    oc = np.zeros_like(col); views = np.zeros(len(pos), np.uint32); st = MeshRecolourStats()
    cd = np.full((len(pos), len(frames)), 255, np.uint8) if codes else None
    check(lib.bf_mesh_recolour_host(pos.ctypes.data_as(C.c_void_p), None if nrm is None else nrm.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), len(pos), fr, len(frames),
                                    int(width), int(height), mat16(intrinsics), C.byref(params), oc.ctypes.data_as(C.c_void_p), views.ctypes.data_as(C.c_void_p),
                                    cd.ctypes.data_as(C.c_void_p) if codes else None, C.byref(st)))
    return (oc, views, st.as_dict()) + ((cd,) if codes else ())


class IndexedMesh(C.Structure):
    _fields_ = [("d_positions", C.c_void_p), ("d_colors", C.c_void_p), ("d_faces", C.c_void_p), ("numVertices", C.c_uint32), ("numFaces", C.c_uint32)]


class CleanMesh(C.Structure):
    _fields_ = [("d_positions", C.c_void_p), ("d_colors", C.c_void_p), ("d_normals", C.c_void_p), ("d_faces", C.c_void_p), ("numVertices", C.c_uint32), ("numFaces", C.c_uint32)]


class MeshCleanParams(C.Structure):
    _fields_ = [("minComponentFaces", C.c_uint32), ("keepLargestOnly", C.c_int32), ("computeNormals", C.c_int32)]


class MeshCleanStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("numVerticesIn", "numFacesIn", "numVerticesOut", "numFacesOut", "numComponents", "numComponentsKept", "numIsolatedVertices",
                                          "largestComponentFaces")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class MeshSimplifyParams(C.Structure):
    _fields_ = [("cellSize", C.c_float), ("computeNormals", C.c_int32)]


class MeshSimplifyStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("numVerticesIn", "numFacesIn", "numClusters", "numVerticesOut", "numFacesOut", "numFacesCollapsed", "numFacesDuplicate", "largestCluster")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def mesh_simplify_host(positions, colors, faces, cell_size, normals=False):
    """bf_mesh_simplify_host, the definition on one core: (positions, colours, normals or None, faces, stats dict, map).  Host-only."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); col = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    fc = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    assert len(pos) == len(col)
    p = MeshSimplifyParams(float(cell_size), int(bool(normals))); st = MeshSimplifyStats()
    op = np.zeros_like(pos); oc = np.zeros_like(col); on = np.zeros_like(pos); of = np.zeros_like(fc); mp = np.zeros(len(pos), np.uint32)
    check(lib.bf_mesh_simplify_host(pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), fc.ctypes.data_as(C.c_void_p), len(pos), len(fc), C.byref(p),
                                    op.ctypes.data_as(C.c_void_p), oc.ctypes.data_as(C.c_void_p), on.ctypes.data_as(C.c_void_p), of.ctypes.data_as(C.c_void_p),
                                    mp.ctypes.data_as(C.c_void_p), len(pos), len(fc), C.byref(st)))
    nv, nf = st.numVerticesOut, st.numFacesOut
    return op[:nv].copy(), oc[:nv].copy(), (on[:nv].copy() if normals else None), of[:nf].copy(), st.as_dict(), mp


class MeshDistanceParams(C.Structure):
    _fields_ = [("maxDistance", C.c_float), ("sampleSpacing", C.c_float), ("sampleMode", C.c_int32)]


class MeshDistanceStats(C.Structure):
    _fields_ = [("numSamples", C.c_uint64), ("numWithin", C.c_uint64), ("numBeyond", C.c_uint64), ("numDegenerateA", C.c_uint32), ("numDegenerateB", C.c_uint32),
                ("maxWithin", C.c_double), ("sumW", C.c_int64), ("sumWD", C.c_int64), ("sumWD2", C.c_int64), ("sumWBeyond", C.c_int64),
                ("scaleW", C.c_int32), ("scaleWD", C.c_int32), ("scaleWD2", C.c_int32), ("reserved", C.c_int32), ("histogram", C.c_int64 * 1024)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("reserved", "histogram")}
        d["histogram"] = np.array(self.histogram, np.int64)
        return d


def mesh_distance_summary(stats, thresholds=()):
    """the figures a caller takes from a bf_mesh_distance_stats dict: mean, rms, max, median and p90 (to the upper edge of their histogram bin of maxDistance /
    1024), the share of the weight that lies beyond, and per threshold in metres the share of the weight within it (to a bin).  max_distance: stats' own key,
    set by the callers below.  Plain binary64 over the exact integer sums."""
    w = stats["sumW"] / 2.0 ** stats["scaleW"]; wb = stats["sumWBeyond"] / 2.0 ** stats["scaleW"]
    D = stats["max_distance"]
    hist = stats["histogram"].astype(np.float64) / 2.0 ** stats["scaleW"]
    cum = np.cumsum(hist)

    def pct(q):
        return float("nan") if w <= 0 else (int(np.searchsorted(cum, q * w, "left")) + 1) * D / 1024.0
    out = {"samples": stats["numSamples"], "mean": stats["sumWD"] / 2.0 ** stats["scaleWD"] / w if w > 0 else float("nan"),
           "rms": float(np.sqrt(stats["sumWD2"] / 2.0 ** stats["scaleWD2"] / w)) if w > 0 else float("nan"), "median": pct(0.5), "p90": pct(0.9), "max": stats["maxWithin"],
           "beyond_share": wb / (w + wb) if w + wb > 0 else 0.0}
    for t in thresholds:
        k = min(1024, int(np.floor(t * 1024.0 / D)))
        out["within_%g" % t] = float(cum[k - 1] / (w + wb)) if k >= 1 and w + wb > 0 else 0.0
    return out


def _host_mesh(m):
    pos = np.ascontiguousarray(m[0], np.float32).reshape(-1, 3); fc = np.ascontiguousarray(m[1], np.uint32).reshape(-1, 3)
    return pos, fc


def mesh_distance_host(a, b, max_distance, sample_spacing=0.0, sample_mode=0):
    """bf_mesh_distance_host, the definition on one core: (distance float64, nearest face uint32, weight float64, stats dict) of mesh a = (positions, faces)
    against the surface b = (positions, faces).  Host-only."""
    pa, fa = _host_mesh(a); pb, fb = _host_mesh(b)
    p = MeshDistanceParams(float(max_distance), float(sample_spacing), int(sample_mode)); st = MeshDistanceStats()
    n = C.c_uint64()
    check(lib.bf_mesh_distance_sample_count_host(pa.ctypes.data_as(C.c_void_p), fa.ctypes.data_as(C.c_void_p), C.c_uint32(len(pa)), C.c_uint32(len(fa)), C.byref(p), C.byref(n)))
    n = n.value
    hd = np.zeros(n, np.float64); hf = np.zeros(n, np.uint32); hw = np.zeros(n, np.float64)
    check(lib.bf_mesh_distance_host(pa.ctypes.data_as(C.c_void_p), fa.ctypes.data_as(C.c_void_p), C.c_uint32(len(pa)), C.c_uint32(len(fa)), pb.ctypes.data_as(C.c_void_p),
                                    fb.ctypes.data_as(C.c_void_p), C.c_uint32(len(pb)), C.c_uint32(len(fb)), C.byref(p), hd.ctypes.data_as(C.c_void_p), hf.ctypes.data_as(C.c_void_p),
                                    hw.ctypes.data_as(C.c_void_p), C.c_uint32(n), C.byref(st)))
    d = st.as_dict(); d["max_distance"] = float(p.maxDistance)
    return hd, hf, hw, d


def write_ply_indexed_error(filename, positions, faces, distance, max_distance):
    """bf_write_ply_indexed_error: the mesh with its vertex-mode distance as a colour ramp (blue 0, green, red max_distance; beyond: magenta).  Host-only."""
    pos, fc = _host_mesh((positions, faces))
    d = np.ascontiguousarray(distance, np.float64)
    assert len(d) == len(pos)
    check(lib.bf_write_ply_indexed_error(str(filename).encode(), pos.ctypes.data_as(C.c_void_p), fc.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_float(max_distance),
                                         C.c_uint32(len(pos)), C.c_uint32(len(fc))))


def mesh_clean_host(positions, colors, faces, min_faces=0, largest=False, normals=False):
    """bf_mesh_clean_host, the definition on one core: (positions, colours, normals or None, faces, stats dict, labels).  Host-only."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); col = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    fc = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    assert len(pos) == len(col)
    p = MeshCleanParams(int(min_faces), int(bool(largest)), int(bool(normals))); st = MeshCleanStats()
    op = np.zeros_like(pos); oc = np.zeros_like(col); on = np.zeros_like(pos); of = np.zeros_like(fc); lab = np.zeros(len(pos), np.uint32)
    check(lib.bf_mesh_clean_host(pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), fc.ctypes.data_as(C.c_void_p), len(pos), len(fc), C.byref(p),
                                 op.ctypes.data_as(C.c_void_p), oc.ctypes.data_as(C.c_void_p), on.ctypes.data_as(C.c_void_p), of.ctypes.data_as(C.c_void_p),
                                 lab.ctypes.data_as(C.c_void_p), len(pos), len(fc), C.byref(st)))
    nv, nf = st.numVerticesOut, st.numFacesOut
    return op[:nv].copy(), oc[:nv].copy(), (on[:nv].copy() if normals else None), of[:nf].copy(), st.as_dict(), lab


def write_ply_indexed_normals(filename, positions, normals, colors, faces):
    """bf_write_ply_indexed_normals: the PLY of an indexed mesh with per-vertex normals ([nv,3] float32; None: the file of write_ply_indexed).  Host-only."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); col = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    fc = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    assert len(pos) == len(col) and (nrm is None or len(nrm) == len(pos))
    check(lib.bf_write_ply_indexed_normals(str(filename).encode(), pos.ctypes.data_as(C.c_void_p), None if nrm is None else nrm.ctypes.data_as(C.c_void_p),
                                           col.ctypes.data_as(C.c_void_p), fc.ctypes.data_as(C.c_void_p), len(pos), len(fc)))


def write_ply_indexed(filename, positions, colors, faces):
    """bf_write_ply_indexed: the PLY of an indexed mesh (positions / colours [nv,3] float32, faces [nf,3] uint32).  Host-only."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); col = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
    fc = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    assert len(pos) == len(col)
    check(lib.bf_write_ply_indexed(str(filename).encode(), pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), fc.ctypes.data_as(C.c_void_p), len(pos), len(fc)))


# --------------------------------------------------------------------------- CorrespondenceEvaluator
class CorrEvaluation(C.Structure):
    _fields_ = [("numCorrect", C.c_uint32), ("numDetected", C.c_uint32), ("numTotal", C.c_uint32)]

    def precision(self):
        lib.bf_corr_evaluation_get_precision.restype = C.c_float
        return float(lib.bf_corr_evaluation_get_precision(C.byref(self)))

    def recall(self):
        lib.bf_corr_evaluation_get_recall.restype = C.c_float
        return float(lib.bf_corr_evaluation_get_recall(C.byref(self)))

    def as_tuple(self):
        return (self.numCorrect, self.numDetected, self.numTotal)


class CorrEvalParams(C.Structure):
    _fields_ = [("depthMin", C.c_float), ("depthMax", C.c_float), ("distThresh", C.c_float), ("normalThresh", C.c_float), ("colorThresh", C.c_float)]


class CorrespondenceEvaluator:
    """Python view of `bf_correspondence_evaluator` (== class CorrespondenceEvaluator, CorrespondenceEvaluator.h:39): precision / recall
    of the current frame's image-to-image matches against a reference trajectory."""

    def __init__(self, trajectory=None, log_prefix=None, handle=None):
        self._borrowed = handle is not None
        if handle is not None:
            self._h = handle
            return
        t = np.ascontiguousarray(trajectory, np.float32).reshape(-1, 16)
        self._h = C.c_void_p()
        check(lib.bf_correspondence_evaluator_create(t.ctypes.data_as(C.POINTER(C.c_float)), len(t), (log_prefix or "").encode(), C.byref(self._h)))

    def close(self):
        if self._h and not self._borrowed:
            lib.bf_correspondence_evaluator_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evaluate(self, mgr, cache, sift_intrinsics_inv, filtered, recompute_cache, clear_cache, corr_type, params=None, stream=0):
        p = params or CorrEvalParams(0.5, 4.0, 0.15, 0.97, 0.1)          # zParametersBundlingDefault.txt:26-27,55-57
        out = CorrEvaluation()
        check(lib.bf_correspondence_evaluator_evaluate(self._h, mgr._h, cache._h, _f16(sift_intrinsics_inv), C.byref(p), int(filtered), int(recompute_cache),
                                                       int(clear_cache), corr_type.encode(), C.c_void_p(stream), C.byref(out)))
        return out

    def finish_logging(self):
        check(lib.bf_correspondence_evaluator_finish_logging_to_file(self._h))

    def total(self, corr_type):
        out = CorrEvaluation()
        check(lib.bf_correspondence_evaluator_get_total(self._h, corr_type.encode(), C.byref(out)))
        return out

    def overlap_counts(self, num_frames, with_flags=True):
        c = np.zeros((num_frames, 4), np.uint32); f = np.zeros(num_frames, np.uint8)
        check(lib.bf_correspondence_evaluator_get_overlap_counts(self._h, c.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p) if with_flags else None, num_frames))
        return c, f


# --------------------------------------------------------------------------- ray cast
class RayCastParams(C.Structure):
    _fields_ = [("m_viewMatrix", C.c_float * 16), ("m_viewMatrixInverse", C.c_float * 16),
                ("mx", C.c_float), ("my", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("m_width", C.c_uint32), ("m_height", C.c_uint32), ("m_numOccupiedSDFBlocks", C.c_uint32), ("m_maxNumVertices", C.c_uint32),
                ("m_splatMinimum", C.c_int32), ("m_minDepth", C.c_float), ("m_maxDepth", C.c_float),
                ("m_rayIncrement", C.c_float), ("m_thresSampleDist", C.c_float), ("m_thresDist", C.c_float),
                ("m_useGradients", C.c_int32), ("dummy0", C.c_uint32)]


class RayCastData(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("d_depth", "d_depth4", "d_normals", "d_colors", "d_rayIntervalSplatMin", "d_rayIntervalSplatMax")]


def write_processed_summary(path, heap_free_count, optimized_trajectory, aborted=False):
    """processed.txt of StopScanningAndExit (DepthSensing.cpp:921-957) -> the `valid` verdict"""
    T = np.ascontiguousarray(optimized_trajectory, np.float32).reshape(-1, 16)
    v = C.c_int()
    check(lib.bf_write_processed_summary(str(path).encode(), C.c_uint32(int(heap_free_count)), T.ctypes.data_as(C.c_void_p), C.c_uint32(len(T)), int(aborted), C.byref(v)))
    return bool(v.value)


def ray_cast_params_from_global_app_state(gas, intrinsics):
    """CUDARayCastSDF::parametersFromGlobalAppState (CUDARayCastSDF.h:24-52)"""
    p = RayCastParams()
    check(lib.bf_ray_cast_params_from_global_app_state(C.byref(gas), _f16(intrinsics), C.byref(p)))
    return p


class RayCastSDF:
    """Python view of `bf_ray_cast` (== class CUDARayCastSDF)."""

    def __init__(self, params, stream=None):
        self._h = C.c_void_p()
        check(lib.bf_ray_cast_create(C.byref(params), C.byref(self._h)))
        if stream is not None:
            check(lib.bf_ray_cast_set_stream(self._h, C.c_void_p(stream)))

    def close(self):
        if self._h:
            lib.bf_ray_cast_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def params(self):
        p = RayCastParams()
        check(lib.bf_ray_cast_get_params(self._h, C.byref(p)))
        return p

    def update_min_max(self, dmin, dmax):
        check(lib.bf_ray_cast_update_min_max(self._h, C.c_float(dmin), C.c_float(dmax)))

    def set_intrinsics(self, width, height, K):
        check(lib.bf_ray_cast_set_intrinsics(self._h, width, height, _f16(K)))

    def render(self, scene, cam, last_rigid_transform):
        """render(hashData, hashParams, lastRigidTransform) on a SceneRepHashSDF whose frustum list was made for `cam` (after an
        integrate, or scene.compactify(T, cam))."""
        hd = scene.hash_data(); hp = scene.hash_params()
        check(lib.bf_ray_cast_render(self._h, C.byref(hd), C.byref(hp), C.byref(cam), _f16(last_rigid_transform)))

    def convert_to_camera_space(self, cam):
        check(lib.bf_ray_cast_convert_to_camera_space(self._h, C.byref(cam)))

    def download(self):
        """dict of host images: depth (H,W), depth4 / normals / colors (H,W,4), ray_min / ray_max (H,W)"""
        import torch
        torch.cuda.synchronize()
        p = self.params(); d = RayCastData()
        check(lib.bf_ray_cast_get_data(self._h, C.byref(d)))
        n = p.m_width * p.m_height
        f1 = lambda ptr: _d2h(ptr, n * 4).view("<f4").reshape(p.m_height, p.m_width).copy()
        f4 = lambda ptr: _d2h(ptr, n * 16).view("<f4").reshape(p.m_height, p.m_width, 4).copy()
        return dict(depth=f1(d.d_depth), depth4=f4(d.d_depth4), normals=f4(d.d_normals), colors=f4(d.d_colors),
                    ray_min=f1(d.d_rayIntervalSplatMin), ray_max=f1(d.d_rayIntervalSplatMax))


# --------------------------------------------------------------------------- frame rendering (include/bf_render.h, csrc/render.hip)
class RenderState(C.Structure):
    """bf_render_state: the rendering keys of zParametersDefault.txt"""
    _fields_ = [("s_materialShininess", C.c_float),
                ("s_materialAmbient", C.c_float * 4), ("s_materialDiffuse", C.c_float * 4), ("s_materialSpecular", C.c_float * 4),
                ("s_lightAmbient", C.c_float * 4), ("s_lightDiffuse", C.c_float * 4), ("s_lightSpecular", C.c_float * 4),
                ("s_lightDirection", C.c_float * 3),
                ("s_RenderMode", C.c_uint32),
                ("s_renderingDepthDiscontinuityThresOffset", C.c_float), ("s_renderingDepthDiscontinuityThresLin", C.c_float),
                ("s_generateVideo", C.c_int32), ("s_generateVideoDir", C.c_char * 256),
                ("s_topVideoTransformWorld", C.c_float * 16), ("s_topVideoCameraPose", C.c_float * 4), ("s_topVideoMinMax", C.c_float * 2)]


def default_render_state(path=None, with_missing=False):
    """bf_render_state_default, or bf_render_state_read of a parameter file (with_missing: also the number of fields the file does not name)"""
    g = RenderState(); n = C.c_uint32()
    if path is None:
        check(lib.bf_render_state_default(C.byref(g)))
    else:
        check(lib.bf_render_state_read(str(path).encode(), C.byref(g), C.byref(n)))
    return (g, n.value) if with_missing else g


# --------------------------------------------------------------------------- recording (include/bf_record.h)
class RecordState(C.Structure):
    """bf_record_state: the recording keys of zParametersDefault.txt"""
    _fields_ = [("s_recordData", C.c_int32), ("s_recordCompression", C.c_int32), ("s_recordDataWidth", C.c_uint32), ("s_recordDataHeight", C.c_uint32),
                ("s_recordDataFile", C.c_char * 512)]


def default_record_state(path=None, with_missing=False):
    """bf_record_state_default, or bf_record_state_read of a parameter file (with_missing: also the number of fields the file does not name)"""
    g = RecordState(); n = C.c_uint32()
    if path is None:
        check(lib.bf_record_state_default(C.byref(g)))
    else:
        check(lib.bf_record_state_read(str(path).encode(), C.byref(g), C.byref(n)))
    return (g, n.value) if with_missing else g


def ray_cast_intrinsics_inv(params):
    out = (C.c_float * 16)()
    check(lib.bf_ray_cast_intrinsics_inv(C.byref(params), out))
    return np.array(list(out), np.float32).reshape(4, 4)


def write_png_rgba8(path, rgba):
    a = np.ascontiguousarray(rgba, np.uint8)
    assert a.ndim == 3 and a.shape[2] == 4
    check(lib.bf_write_png_rgba8(str(path).encode(), a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0]))


class FrameRenderer:
    """Python view of `bf_frame_renderer`: DX11RGBDRenderer::RenderDepthMap + DX11PhongLighting::render + DX11QuadDrawer::RenderQuad on a width x height image."""

    def __init__(self, width, height, stream=0):
        self._h = C.c_void_p()
        self.w, self.h = int(width), int(height)
        check(lib.bf_frame_renderer_create(self.w, self.h, C.byref(self._h)))
        if stream:
            check(lib.bf_frame_renderer_set_stream(self._h, C.c_void_p(stream)))

    def close(self):
        if self._h:
            lib.bf_frame_renderer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shade(self, depth, colors, intrinsics_inv, state=None, use_material=False, tracking_lost=False, thresh_offset=None, thresh_lin=None):
        """depth: float32 device tensor (h, w) or a device pointer; colors: float32 (h, w, 4) likewise.  The thresholds default to the state's."""
        st = state if state is not None else default_render_state()
        off = st.s_renderingDepthDiscontinuityThresOffset if thresh_offset is None else thresh_offset
        lin = st.s_renderingDepthDiscontinuityThresLin if thresh_lin is None else thresh_lin
        dp = C.c_void_p(depth) if isinstance(depth, int) else _p(depth)
        cp = C.c_void_p(colors) if isinstance(colors, int) else _p(colors)
        check(lib.bf_frame_renderer_shade(self._h, dp, cp, _f16(intrinsics_inv), C.byref(st), int(bool(use_material)), int(bool(tracking_lost)), C.c_float(off), C.c_float(lin)))

    def depth_hsv(self, depth, dmin, dmax):
        check(lib.bf_frame_renderer_depth_hsv(self._h, _p(depth), C.c_float(dmin), C.c_float(dmax)))

    def rgbx(self, img):
        check(lib.bf_frame_renderer_rgbx(self._h, _p(img)))

    def download_rgba8(self):
        out = np.zeros((self.h, self.w, 4), np.uint8)
        check(lib.bf_frame_renderer_download_rgba8(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def download_target(self):
        """the float4 target (GetColorsSRV) as float32 (h, w, 4); call after download_rgba8 or a synchronisation of the stream"""
        t = C.c_void_p(); r = C.c_void_p()
        check(lib.bf_frame_renderer_get_images(self._h, C.byref(t), C.byref(r)))
        return _d2h(t.value, self.w * self.h * 16).view("<f4").reshape(self.h, self.w, 4).copy()


# --------------------------------------------------------------------------- the point cloud (include/bf_pointcloud.h)
class PointCloudParams(C.Structure):
    _fields_ = [("maxPoints", C.c_uint32), ("maxFramePixels", C.c_uint32), ("cellSize", C.c_float), ("maxDepth", C.c_float)]


class PointCloudView(C.Structure):
    _fields_ = [("d_positions", C.c_void_p), ("d_normals", C.c_void_p), ("d_colors", C.c_void_p), ("numPoints", C.c_uint32)]


def write_ply_points(filename, positions, normals, colors):
    """bf_write_ply_points: positions / normals [n,3] float32, colours [n,4] uint8.  Host-only."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    col = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
    assert len(pos) == len(nrm) == len(col)
    check(lib.bf_write_ply_points(str(filename).encode(), pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), len(pos)))


def point_cloud_build_host(depths, colors, transforms, intrinsics_inv, cell_size=0.005, max_depth=3.5, capacity=None):
    """bf_point_cloud_build_host: the definition as the sequential loop on one core (no device).  depths: float32 (h, w) arrays, colors: uint8 (h, w, 4),
    transforms: (n, 4, 4).  Returns (positions, normals, colours, count); with a capacity below the count the arrays hold the first `capacity` points."""
    ds = [np.ascontiguousarray(d, np.float32) for d in depths]; cs = [np.ascontiguousarray(c, np.uint8) for c in colors]
    n = len(ds)
    assert len(cs) == n
    h, w = ds[0].shape if n else (0, 0)
    assert all(d.shape == (h, w) for d in ds) and all(c.shape == (h, w, 4) for c in cs)
    T = np.ascontiguousarray(transforms, np.float32).reshape(-1, 16)
    assert len(T) == n
    dp = (C.c_void_p * max(n, 1))(*[d.ctypes.data for d in ds]); cp = (C.c_void_p * max(n, 1))(*[c.ctypes.data for c in cs])
    cnt = C.c_uint32()
    args = (dp, cp, n, w, h, _f16(intrinsics_inv), T.ctypes.data_as(C.c_void_p), C.c_float(cell_size), C.c_float(max_depth))
    if capacity is None:
        check(lib.bf_point_cloud_build_host(*args, 0, None, None, None, C.byref(cnt)))
        capacity = cnt.value
    pos = np.zeros((capacity, 3), np.float32); nrm = np.zeros((capacity, 3), np.float32); col = np.zeros((capacity, 4), np.uint8)
    check(lib.bf_point_cloud_build_host(*args, int(capacity), pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), C.byref(cnt)))
    m = min(capacity, cnt.value)
    return pos[:m], nrm[:m], col[:m], cnt.value


class PointCloud:
    """Python view of `bf_point_cloud`: RGBDSensor::recordPointCloud per frame, thinned on the device to one point per cell as it grows."""

    def __init__(self, max_points, max_frame_pixels, cell_size=0.005, max_depth=3.5, stream=0):
        self._h = C.c_void_p()
        self.params = PointCloudParams(int(max_points), int(max_frame_pixels), float(cell_size), float(max_depth))
        check(lib.bf_point_cloud_create(C.byref(self.params), C.byref(self._h)))
        if stream:
            check(lib.bf_point_cloud_set_stream(self._h, C.c_void_p(stream)))

    def close(self):
        if self._h:
            lib.bf_point_cloud_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(lib.bf_point_cloud_reset(self._h))

    def add_frame(self, depth, color, intrinsics_inv, transform):
        """depth: float32 cuda tensor (h, w); color: uint8 cuda tensor (h, w, 4).  Returns the number of points the frame appended."""
        h, w = int(depth.shape[0]), int(depth.shape[1])
        assert tuple(color.shape) == (h, w, 4) and depth.is_contiguous() and color.is_contiguous()
        n = C.c_uint32()
        check(lib.bf_point_cloud_add_frame(self._h, _p(depth), _p(color), w, h, _f16(intrinsics_inv), _f16(transform), C.byref(n)))
        return n.value

    def view(self):
        v = PointCloudView()
        check(lib.bf_point_cloud_get_gpu(self._h, C.byref(v)))
        return v

    def num_points(self):
        return self.view().numPoints

    def download(self):
        """(positions (n, 3) float32, normals (n, 3) float32, colours (n, 4) uint8)"""
        n = self.num_points()
        pos = np.zeros((n, 3), np.float32); nrm = np.zeros((n, 3), np.float32); col = np.zeros((n, 4), np.uint8)
        cnt = C.c_uint32()
        check(lib.bf_point_cloud_download(self._h, pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), n, C.byref(cnt)))
        assert cnt.value == n
        return pos, nrm, col

    def save(self, filename):
        n = C.c_uint32()
        check(lib.bf_point_cloud_save(self._h, str(filename).encode(), C.byref(n)))
        return n.value
