"""--mesh / --mesh-host of tools/run_sens.py and tools/run_sequence.py: the scan's PLY after the end of the sequence, by the frame loop's own command
(bf_pipeline_save_mesh: extraction and weld on the device) or by the host route (bf_marching_cubes_extract + bf_marching_cubes_save_mesh), with the counts
and the seconds of each so that the two can be put side by side."""
import ctypes as C
import time

import numpy as np

import bundlefusion_amd as bf


def add_arguments(ap):
    ap.add_argument("--mesh", default=None, metavar="PATH", help="write the mesh as a PLY after the end of the sequence (bf_pipeline_save_mesh: welded on the device)")
    ap.add_argument("--mesh-host", default=None, metavar="PATH", help="the same file by the host route (extract + save_mesh on one core), for comparison")


def _device_stages(p, path):
    """the stages of the device route one by one, on an object of their own over the pipeline's scene (the same file again)"""
    lib, check = bf.capi.lib, bf.capi.check
    mc = bf.capi.MarchingCubesHashSDF.from_global_app_state(p.gas)
    sc = p.scene()
    t0 = time.perf_counter()
    n, found = mc.extract_gpu(sc)
    t1 = time.perf_counter()
    m = bf.capi.IndexedMesh()
    check(lib.bf_marching_cubes_weld(mc._h, None, 0, None, C.byref(m)))          # (waits for its stream)
    t2 = time.perf_counter()
    pos = np.empty((m.numVertices, 3), np.float32); col = np.empty((m.numVertices, 3), np.float32); faces = np.empty((m.numFaces, 3), np.uint32)
    check(lib.bf_marching_cubes_download_indexed(mc._h, pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), faces.ctypes.data_as(C.c_void_p)))
    bf.capi.write_ply_indexed(path, pos, col, faces)
    t3 = time.perf_counter()
    mc.close()
    print("mesh (device route, stage by stage): extract %.4f s, weld %.4f s, download + write %.4f s" % (t1 - t0, t2 - t1, t3 - t2))


def _host(p, path):
    sc = p.scene()
    cap = 3000000                                            # s_marchingCubesMaxNumTriangles; a host has to guess, and to ask again if the volume holds more
    while True:
        mc = bf.capi.MarchingCubesHashSDF.from_global_app_state(p.gas, max_triangles=cap)
        t0 = time.perf_counter()
        tris, found = mc.extract(sc)
        t1 = time.perf_counter()
        if found <= cap:
            break
        mc.close(); cap = found
    nv, nf = mc.save_mesh(path)
    t2 = time.perf_counter()
    mc.close()
    print("mesh (host route) %s: %d vertices, %d faces, %d triangles; extract + copy %.3f s, weld + write %.3f s, total %.3f s" % (path, nv, nf, found, t1 - t0, t2 - t1, t2 - t0))


def write(p, a):
    """p: the Pipeline after process_end_of_sequence / synchronize; a: the parsed arguments"""
    if a.mesh:
        t0 = time.perf_counter()
        nv, nf, nt = p.save_mesh(a.mesh)
        dt = time.perf_counter() - t0
        print("mesh (device route) %s: %d vertices, %d faces, %d triangles; bf_pipeline_save_mesh %.3f s" % (a.mesh, nv, nf, nt, dt))
        _device_stages(p, a.mesh)
    if a.mesh_host:
        _host(p, a.mesh_host)
