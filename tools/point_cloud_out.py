"""--point-cloud / --point-cloud-host of tools/run_sens.py and tools/run_sequence.py: the scan's point cloud after the end of the sequence, by the frame loop's own
call (bf_pipeline_save_point_cloud: the stored frames thinned on the device) or by the host route (frames copied out, bf_point_cloud_build_host on one core), with
the counts and the seconds of each so that the two can be put side by side."""
import ctypes as C
import time

import numpy as np

import bundlefusion_amd as bf


def add_arguments(ap):
    ap.add_argument("--point-cloud", default=None, metavar="FILE", help="write the point cloud of the key frames as a PLY after the end of the sequence (bf_pipeline_save_point_cloud)")
    ap.add_argument("--point-cloud-stride", type=int, default=0, metavar="N", help="every N-th frame (default: s_submapSize, the key frames)")
    ap.add_argument("--point-cloud-cell", type=float, default=0.005, metavar="M", help="one point per cell of M metres (<= 0: no thinning)")
    ap.add_argument("--point-cloud-max-depth", type=float, default=3.5, help="points at or beyond this camera depth are dropped")
    ap.add_argument("--point-cloud-max-points", type=int, default=0, help="capacity of the cloud (default: 4 Mi points)")
    ap.add_argument("--point-cloud-host", default=None, metavar="FILE", help="the same file by the host route (one core), for comparison")


def _frames_on_stride(p, stride):
    T = p.optimized_trajectory()
    return T, [f for f in range(0, len(T), stride) if not (np.isnan(T[f, 0, 0]) or T[f, 0, 0] == -np.inf)]


def _kinv(p):
    lib, check = bf.capi.lib, bf.capi.check
    im = C.c_void_p(); Kinv = (C.c_float * 16)()
    check(lib.bf_pipeline_get_image_manager(p._h, C.byref(im)))
    check(lib.bf_image_manager_get_depth_intrinsics(im, None, Kinv))
    return im, np.array(list(Kinv), np.float32).reshape(4, 4)


def _device_stages(p, a, stride, path):
    """the stages of the device route one by one, on an accumulator of their own over the pipeline's stored frames (the same file again)"""
    import torch
    lib, check = bf.capi.lib, bf.capi.check
    im, Kinv = _kinv(p)
    T, idx = _frames_on_stride(p, stride)
    w, h = p.gas.s_integrationWidth, p.gas.s_integrationHeight
    pc = bf.capi.PointCloud(a.point_cloud_max_points or (4 << 20), w * h, a.point_cloud_cell, a.point_cloud_max_depth)
    count = bf.capi.PointCloud(w * h, w * h, 0.0, a.point_cloud_max_depth)          # no thinning: what a frame adds is its number of candidates
    ptrs = []
    for f in idx:
        d, c = C.c_void_p(), C.c_void_p()
        check(lib.bf_image_manager_get_integrate_frame_gpu(im, f, C.byref(d), C.byref(c)))
        ptrs.append((d, c))
    candidates = 0
    for (d, c), f in zip(ptrs, idx):
        n = C.c_uint32()
        count.reset()
        check(lib.bf_point_cloud_add_frame(count._h, d, c, w, h, bf.capi._f16(Kinv), bf.capi._f16(T[f]), C.byref(n)))
        candidates += n.value
    count.close()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for (d, c), f in zip(ptrs, idx):
        check(lib.bf_point_cloud_add_frame(pc._h, d, c, w, h, bf.capi._f16(Kinv), bf.capi._f16(T[f]), None))          # (waits for its stream: the count)
    t1 = time.perf_counter()
    pos, nrm, col = pc.download()
    t2 = time.perf_counter()
    bf.capi.write_ply_points(path, pos, nrm, col)
    t3 = time.perf_counter()
    pc.close()
    print("point cloud (device route, stage by stage): %d frames, %d candidates, %d points; adds %.4f s (%.3f ms per frame), download %.4f s, write %.4f s"
          % (len(idx), candidates, len(pos), t1 - t0, 1e3 * (t1 - t0) / max(len(idx), 1), t2 - t1, t3 - t2))


def _host(p, a, stride, path):
    _, Kinv = _kinv(p)
    t0 = time.perf_counter()
    T, idx = _frames_on_stride(p, stride)
    ds, cs = zip(*[p.integrate_frame_cpu(f) for f in idx]) if idx else ((), ())
    t1 = time.perf_counter()
    pos, nrm, col, n = bf.capi.point_cloud_build_host(ds, cs, T[idx], Kinv, a.point_cloud_cell, a.point_cloud_max_depth)          # two passes: the count, then the arrays
    t2 = time.perf_counter()
    bf.capi.write_ply_points(path, pos, nrm, col)
    t3 = time.perf_counter()
    print("point cloud (host route) %s: %d frames, %d points; frame download %.3f s, loop on one core %.3f s (two passes: count, then arrays), write %.3f s, total %.3f s"
          % (path, len(idx), n, t1 - t0, t2 - t1, t3 - t2, t3 - t0))


def write(p, a):
    """p: the Pipeline after process_end_of_sequence / synchronize; a: the parsed arguments"""
    stride = a.point_cloud_stride or int(p.gbs.s_submapSize)
    if a.point_cloud:
        t0 = time.perf_counter()
        n, used = p.save_point_cloud(a.point_cloud, stride, a.point_cloud_cell, a.point_cloud_max_depth, a.point_cloud_max_points)
        dt = time.perf_counter() - t0
        print("point cloud (device route) %s: %d points from %d frames (stride %d, cell %g m, max depth %g m); bf_pipeline_save_point_cloud %.3f s"
              % (a.point_cloud, n, used, stride, a.point_cloud_cell, a.point_cloud_max_depth, dt))
        if not p.camera_calibration():
            _device_stages(p, a, stride, a.point_cloud)
    if a.point_cloud_host:
        if p.camera_calibration():
            raise SystemExit("--point-cloud-host: the registered depth lives in the colour camera, whose inverse intrinsics this tool does not read; use --point-cloud")
        _host(p, a, stride, a.point_cloud_host)
