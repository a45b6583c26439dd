"""--mesh / --mesh-host of tools/run_sens.py and tools/run_sequence.py: the scan's PLY after the end of the sequence, by the frame loop's own command
(bf_pipeline_save_mesh: extraction and weld on the device) or by the host route (bf_marching_cubes_extract + bf_marching_cubes_save_mesh), with the counts
and the seconds of each so that the two can be put side by side.  --mesh-min-faces / --mesh-largest / --mesh-normals clean the mesh before it is written
(bf_pipeline_save_mesh_clean on the device route, bf_mesh_clean_host on the host route) and print the cleaning's stats.  --mesh-simplify-cell METRES clusters
the cleaned mesh's vertices on a grid of that size before it is written (bf_pipeline_save_mesh_simplified on the device route, bf_mesh_simplify_host on the host
route; normals, if asked for, are the simplified mesh's) and prints the simplification's stats and its time.  --mesh-recolour takes the cleaned mesh's vertex
colours from the stored frames on --mesh-recolour-stride under the optimised trajectory (bf_pipeline_save_mesh_recoloured on the device route,
bf_mesh_recolour_host on the host route; --mesh-recolour-best: the best view in place of the blend), before the simplification if one is asked for, and prints
the recolouring's stats, its time and the mean absolute colour difference across the cleaned mesh's edges before and after, for both modes.  --mesh-texture
(device route) writes the mesh with a texture atlas from the same frames (bf_pipeline_save_mesh_textured: the PLY and a PNG next to it; after the recolouring and
the simplification if those are asked for) and prints the texture's stats, the times of its stages, the one-core
route's time and whether its atlas is the device's, and the held-out colour measurement of profiles/mesh_texture.md.  --mesh-evaluate measures the mesh the
other options describe (cleaned, simplified) against synth.room_mesh(), the true surface of the synthetic room, in both directions on the device
(bf_pipeline_measure_mesh: scan -> reference is the accuracy, reference -> scan the completeness) and prints mean, RMS, median, 90th percentile, max, the share
within one voxel and the share beyond --mesh-evaluate-max; --mesh-evaluate-against PLY measures against a mesh on disk instead; --mesh-evaluate-spacing sets the
surface sampling (the reference is always sampled on its surface; the scan by its vertices unless --mesh-evaluate-surface); --mesh-error-ply PATH writes the
measured mesh with its distance as a colour ramp; with --mesh-host the one-core route (bf_mesh_distance_host) runs the scan -> reference direction on the same arrays for comparison."""
import ctypes as C
import time

import numpy as np

import bundlefusion_amd as bf


def add_arguments(ap):
    ap.add_argument("--mesh", default=None, metavar="PATH", help="write the mesh as a PLY after the end of the sequence (bf_pipeline_save_mesh: welded on the device)")
    ap.add_argument("--mesh-host", default=None, metavar="PATH", help="the same file by the host route (extract + save_mesh on one core), for comparison")
    ap.add_argument("--mesh-min-faces", type=int, default=0, metavar="N", help="drop connected pieces of the mesh with fewer than N faces, and vertices no face uses")
    ap.add_argument("--mesh-largest", action="store_true", help="keep only the largest connected piece of the mesh")
    ap.add_argument("--mesh-normals", action="store_true", help="write area-weighted per-vertex normals into the PLY")
    ap.add_argument("--mesh-simplify-cell", type=float, default=0.0, metavar="METRES", help="simplify the (cleaned) mesh before it is written: one vertex per grid cell of this size")
    ap.add_argument("--mesh-recolour", action="store_true", help="take the (cleaned) mesh's vertex colours from the stored frames under the optimised trajectory")
    ap.add_argument("--mesh-recolour-stride", type=int, default=0, metavar="N", help="recolour from every Nth frame (default: s_submapSize, the key frames)")
    ap.add_argument("--mesh-texture", action="store_true", help="write the mesh with a texture atlas from the stored frames (a PNG next to the PLY); the stride is --mesh-recolour-stride")
    ap.add_argument("--mesh-evaluate", action="store_true", help="measure the mesh against the true surface of the synthetic room (synth.room_mesh()), both directions")
    ap.add_argument("--mesh-evaluate-against", default=None, metavar="PLY", help="measure the mesh against this PLY instead")
    ap.add_argument("--mesh-evaluate-max", type=float, default=0.1, metavar="METRES", help="maxDistance of the measurement: samples farther than this count as beyond (default 0.1)")
    ap.add_argument("--mesh-evaluate-spacing", type=float, default=0.01, metavar="METRES", help="sampleSpacing of the surface sampling (default 0.01)")
    ap.add_argument("--mesh-evaluate-surface", action="store_true", help="sample the scan's surface too (area-weighted) instead of taking its vertices")
    ap.add_argument("--mesh-error-ply", default=None, metavar="PATH", help="write the measured mesh with its vertices' distance to the reference as a colour ramp")
    ap.add_argument("--mesh-recolour-best", action="store_true", help="each vertex takes its best view (greatest weight) instead of the weighted blend of all views")


def _cleaning(a):
    return a.mesh_min_faces > 0 or a.mesh_largest or a.mesh_normals


def _stats_line(st):
    return ("%d -> %d vertices, %d -> %d faces; %d components, %d kept, largest %d faces, %d isolated vertices"
            % (st["numVerticesIn"], st["numVerticesOut"], st["numFacesIn"], st["numFacesOut"], st["numComponents"], st["numComponentsKept"], st["largestComponentFaces"],
               st["numIsolatedVertices"]))


def _simplify_line(st):
    return ("%d -> %d vertices, %d -> %d faces; %d clusters, largest %d vertices, %d faces collapsed, %d duplicate"
            % (st["numVerticesIn"], st["numVerticesOut"], st["numFacesIn"], st["numFacesOut"], st["numClusters"], st["largestCluster"], st["numFacesCollapsed"],
               st["numFacesDuplicate"]))


def _recolour_line(st):
    return ("%d of %d vertices recoloured, %d unseen; %d frames used, %d skipped, at most %d views"
            % (st["numRecoloured"], st["numVertices"], st["numUnseen"], st["numFramesUsed"], st["numFramesSkipped"], st["maxViews"]))


def _recolour_params(p, a, mode=None):
    rp = p.mesh_recolour_defaults()
    rp.mode = (1 if a.mesh_recolour_best else 0) if mode is None else mode
    return rp


def _stride(p, a):
    return a.mesh_recolour_stride if a.mesh_recolour_stride > 0 else int(p.gbs.s_submapSize)


def edge_colour_difference(col, faces):
    """the mean over the mesh's edges (every face's three, shared ones once) and the three channels of |colour(a) - colour(b)|"""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    e.sort(axis=1)
    e = np.unique(e, axis=0)
    return float(np.abs(col[e[:, 0]].astype(np.float64) - col[e[:, 1]].astype(np.float64)).mean()) if len(e) else 0.0


def _device_frames(p, a, offset=0):
    """the frames bf_pipeline_save_mesh_recoloured uses, as a table of device pointers: (table, intrinsics, width, height); offset: the frames offset, offset +
    stride, ... in their place"""
    lib, check = bf.capi.lib, bf.capi.check
    host, K, w, h = p.mesh_recolour_frames_host(_stride(p, a), images=False)
    if offset:
        every, K, w, h = p.mesh_recolour_frames_host(1, images=False)
        host = [f for f in every if f[0] % _stride(p, a) == offset]
    im = C.c_void_p()
    check(lib.bf_pipeline_get_image_manager(p._h, C.byref(im)))
    rows = []
    for f, W, o, skipped in host:
        d, c = C.c_void_p(), C.c_void_p()
        check(lib.bf_image_manager_get_integrate_frame_gpu(im, f, C.byref(d), C.byref(c)))
        rows.append((d.value, c.value, W, o, skipped))
    return bf.capi.recolour_frames(rows), K, w, h


def _device_stages_recolour(p, path, a):
    """the stages of the recoloured device route one by one, on an object of their own over the pipeline's scene (the same file again), and the claim: the colour
    difference across the cleaned mesh's edges before and after, for both modes"""
    lib, check = bf.capi.lib, bf.capi.check
    mc = bf.capi.MarchingCubesHashSDF.from_global_app_state(p.gas)
    t0 = time.perf_counter()
    mc.extract_gpu(p.scene())
    t1 = time.perf_counter()
    check(lib.bf_marching_cubes_weld(mc._h, None, 0, None, None))
    t2 = time.perf_counter()
    prm = bf.capi.MeshCleanParams(a.mesh_min_faces, int(a.mesh_largest), 1); cm = bf.capi.CleanMesh(); st = bf.capi.MeshCleanStats()
    check(lib.bf_marching_cubes_clean(mc._h, None, C.byref(prm), C.byref(cm), C.byref(st)))
    check(lib.bf_marching_cubes_clean_labels(mc._h, None, 0))                    # waits for the object's stream: the normals' kernels have ended
    t3 = time.perf_counter()
    frames, K, w, h = _device_frames(p, a)
    t4 = time.perf_counter()
    rm = bf.capi.CleanMesh(); rst = bf.capi.MeshRecolourStats(); rp = _recolour_params(p, a)
    check(lib.bf_marching_cubes_recolour(mc._h, None, frames, len(frames), w, h, bf.capi.mat16(K), C.byref(rp), C.byref(rm), C.byref(rst)))          # (waits for its stream)
    t5 = time.perf_counter()
    pos, col, nrm, faces = mc.download_recoloured(rm.numVertices, rm.numFaces, True)
    old = np.empty((cm.numVertices, 3), np.float32)
    check(lib.bf_marching_cubes_download_clean(mc._h, None, old.ctypes.data_as(C.c_void_p), None, None))
    other = bf.capi.CleanMesh(); orp = _recolour_params(p, a, 1 - rp.mode)
    check(lib.bf_marching_cubes_recolour(mc._h, None, frames, len(frames), w, h, bf.capi.mat16(K), C.byref(orp), C.byref(other), None))
    ocol = mc.download_recoloured(rm.numVertices, 0)[1]
    names = ("blend", "best view")
    print("mesh colour difference across the cleaned mesh's edges (mean |difference| per channel, colours in [0, 1]): voxel colours %.6f, recoloured (%s) %.6f, recoloured (%s) %.6f"
          % (edge_colour_difference(old, faces), names[rp.mode], edge_colour_difference(col, faces), names[1 - rp.mode], edge_colour_difference(ocol, faces)))
    both = faces[(mc.recolour_views(rm.numVertices) > 0)[faces].all(1)]          # (the views of the other mode's run: the same pairs are views in both modes)
    print("  ... over the edges of the faces whose three vertices have a view: voxel colours %.6f, recoloured (%s) %.6f, recoloured (%s) %.6f"
          % (edge_colour_difference(old, both), names[rp.mode], edge_colour_difference(col, both), names[1 - rp.mode], edge_colour_difference(ocol, both)))
    t6 = time.perf_counter()
    check(lib.bf_marching_cubes_recolour(mc._h, None, frames, len(frames), w, h, bf.capi.mat16(K), C.byref(rp), C.byref(rm), None))
    t7 = time.perf_counter()
    if a.mesh_simplify_cell > 0:
        mc._recoloured = rm
        spos, scol, snrm, sfaces, sst = mc.simplify_recoloured(a.mesh_simplify_cell, a.mesh_normals)
        t8 = time.perf_counter()
        bf.capi.write_ply_indexed_normals(path, spos, snrm, scol, sfaces)
        t9 = time.perf_counter()
        print("mesh (device route, stage by stage): extract %.4f s, weld %.4f s, clean + normals %.4f s, frame table %.4f s, recolour %.4f s (again %.4f s), simplify + download %.4f s, write %.4f s"
              % (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t7 - t6, t8 - t7, t9 - t8))
    else:
        bf.capi.write_ply_indexed_normals(path, pos, nrm if a.mesh_normals else None, col, faces)
        t8 = time.perf_counter()
        print("mesh (device route, stage by stage): extract %.4f s, weld %.4f s, clean + normals %.4f s, frame table %.4f s, recolour %.4f s (again %.4f s), write %.4f s"
              % (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t7 - t6, t8 - t7))
    mc.close()


def _texture_line(st):
    return ("%d of %d faces textured, %d not; %d frames used, %d skipped; atlas %d x %d: %d texels from frames, %d from vertices, %d unused"
            % (st["numFacesTextured"], st["numFaces"], st["numFacesUntextured"], st["numFramesUsed"], st["numFramesSkipped"], st["atlasWidth"], st["atlasHeight"],
               st["numTexelsFromFrames"], st["numTexelsFromVertices"], st["numTexelsUnused"]))


def _textured(p, a):
    """the textured save from the frame loop, the simplified save as its reference point in the same process, the stages one by one on an object of their own, the
    one-core route, and the held-out measurement"""
    import torch
    lib, check, capi = bf.capi.lib, bf.capi.check, bf.capi
    cell = a.mesh_simplify_cell if a.mesh_simplify_cell > 0 else None
    t0 = time.perf_counter()
    st, rst, sst, tst, nt = p.save_mesh_textured(a.mesh, None, a.mesh_min_faces, a.mesh_largest, a.mesh_normals, None, _stride(p, a), a.mesh_recolour, cell)
    dt = time.perf_counter() - t0
    print("mesh (device route) %s: %d triangles; cleaned: %s;%s%s textured: %s; bf_pipeline_save_mesh_textured %.3f s"
          % (a.mesh, nt, _stats_line(st), " recoloured: %s;" % _recolour_line(rst) if rst else "", " simplified at %g m: %s;" % (cell, _simplify_line(sst)) if sst else "",
             _texture_line(tst), dt))
    if cell:
        t0 = time.perf_counter()
        p.save_mesh_simplified(a.mesh + ".untextured.ply", cell, None, a.mesh_min_faces, a.mesh_largest, a.mesh_normals)
        print("  the reference point, bf_pipeline_save_mesh_simplified of the same mesh in the same process: %.3f s" % (time.perf_counter() - t0))
    mc = capi.MarchingCubesHashSDF.from_global_app_state(p.gas)
    t0 = time.perf_counter()
    mc.extract_gpu(p.scene())
    t1 = time.perf_counter()
    check(lib.bf_marching_cubes_weld(mc._h, None, 0, None, None))
    prm = capi.MeshCleanParams(a.mesh_min_faces, int(a.mesh_largest), 0); mesh = capi.CleanMesh()
    check(lib.bf_marching_cubes_clean(mc._h, None, C.byref(prm), C.byref(mesh), None))
    if cell:
        sp = capi.MeshSimplifyParams(cell, 0)
        check(lib.bf_marching_cubes_simplify(mc._h, None, C.byref(sp), C.byref(mesh), None))
        check(lib.bf_marching_cubes_simplify_map(mc._h, None, 0))                # waits for the stream
    else:
        check(lib.bf_marching_cubes_clean_labels(mc._h, None, 0))                # waits for the stream
    t2 = time.perf_counter()
    frames, K, w, h = _device_frames(p, a)
    tp = p.mesh_texture_defaults(); ts = capi.MeshTextureStats()
    times = []
    for _ in range(2):
        t3 = time.perf_counter()
        check(lib.bf_marching_cubes_texture(mc._h, None, frames, len(frames), w, h, capi.mat16(K), C.byref(tp), C.byref(ts)))          # (waits for its stream)
        times.append(time.perf_counter() - t3)
    t4 = time.perf_counter()
    atlas, ff, uv = mc.download_texture(ts.atlasWidth, ts.atlasHeight, ts.numFaces)
    t5 = time.perf_counter()
    capi.write_png_rgba8(a.mesh + ".stages.png", atlas)
    t6 = time.perf_counter()
    print("mesh (device route, stage by stage): extract %.4f s, weld + clean%s %.4f s; texture (select + fill + one wait) %.4f s (first call, buffers allocated) and %.4f s; "
          "download of the atlas %.4f s, PNG write %.4f s" % (t1 - t0, " + simplify" if cell else "", t2 - t1, times[0], times[1], t5 - t4, t6 - t5))
    # the one-core route on the same mesh and frames
    nv, nf = mesh.numVertices, mesh.numFaces
    pos = np.empty((nv, 3), np.float32); col = np.empty((nv, 3), np.float32); faces = np.empty((nf, 3), np.uint32)
    for dst, src in ((pos, mesh.d_positions), (col, mesh.d_colors), (faces, mesh.d_faces)):
        if dst.nbytes:
            check(lib.bf_memcpy_d2h(dst.ctypes.data_as(C.c_void_p), C.c_void_p(src), C.c_size_t(dst.nbytes)))
    hframes = p.mesh_recolour_frames_host(_stride(p, a))[0]
    t7 = time.perf_counter()
    hatlas, hff, huv, hst = capi.mesh_texture_host(pos, col, faces, hframes, w, h, K, tp)
    t8 = time.perf_counter()
    same = np.array_equal(hatlas, atlas) and np.array_equal(hff, ff) and np.array_equal(huv.view(np.uint32), uv.view(np.uint32)) and hst == ts.as_dict()
    print("mesh (host route) textured on one core (bf_mesh_texture_host): %.3f s; atlas, face frames, texture coordinates and stats %s the device's" % (t8 - t7, "are" if same else "ARE NOT"))
    # held out: the atlas from the frames on the stride, from the frames half a stride later, and from no frame; a texel came from a frame where the atlas does
    # not change with the vertex colours (all 0 against all 1)
    dpos = torch.from_numpy(pos).cuda(); dfaces = torch.from_numpy(faces.view(np.int32)).cuda(); dcol = torch.from_numpy(col).cuda()
    black = torch.zeros_like(dcol); white = torch.ones_like(dcol)
    none = capi.recolour_frames([])

    def run(colours, table):
        return mc.texture((dpos, colours, dfaces), table, w, h, K, tp)[0]

    later = _device_frames(p, a, _stride(p, a) // 2)[0]
    first, second, plain = run(dcol, frames), run(dcol, later), run(dcol, none)
    in_first = (run(black, frames) == run(white, frames)).all(2) & (first[:, :, 3] == 255); in_second = (run(black, later) == run(white, later)).all(2) & (second[:, :, 3] == 255)
    both = in_first & in_second
    n = int(both.sum())
    diff = lambda x, y: float(np.abs(x[both][:, :3].astype(np.int32) - y[both][:, :3].astype(np.int32)).mean()) if n else 0.0
    print("mesh texture held out: %d frames on the stride, %d half a stride later; %d texels come from frames in both atlases (of %d and %d); mean |byte difference| first vs second %.4f, "
          "interpolated vertex colours vs second %.4f" % (len(frames), len(later), n, int(in_first.sum()), int(in_second.sum()), diff(first, second),
                                                      diff(plain, second)))
    mc.close()


def _device_stages(p, path, a):
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
    if a.mesh_simplify_cell > 0:
        prm = bf.capi.MeshCleanParams(a.mesh_min_faces, int(a.mesh_largest), 0); st = bf.capi.MeshCleanStats()
        check(lib.bf_marching_cubes_clean(mc._h, None, C.byref(prm), None, C.byref(st)))
        check(lib.bf_marching_cubes_clean_labels(mc._h, None, 0))                # waits for the object's stream: the clean's last kernels have ended
        t3 = time.perf_counter()
        sp = bf.capi.MeshSimplifyParams(a.mesh_simplify_cell, int(a.mesh_normals)); sm = bf.capi.CleanMesh(); sst = bf.capi.MeshSimplifyStats()
        check(lib.bf_marching_cubes_simplify(mc._h, None, C.byref(sp), C.byref(sm), C.byref(sst)))
        check(lib.bf_marching_cubes_simplify_map(mc._h, None, 0))                # waits for the stream: the normals' kernels have ended
        t4 = time.perf_counter()
        pos, col, nrm, faces = mc.download_simplified(sm.numVertices, sm.numFaces, a.mesh_normals)
        bf.capi.write_ply_indexed_normals(path, pos, nrm, col, faces)
        t5 = time.perf_counter()
        print("mesh (device route, stage by stage): extract %.4f s, weld %.4f s, clean %.4f s, simplify %.4f s, download + write %.4f s" % (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4))
    elif not _cleaning(a):
        pos = np.empty((m.numVertices, 3), np.float32); col = np.empty((m.numVertices, 3), np.float32); faces = np.empty((m.numFaces, 3), np.uint32)
        check(lib.bf_marching_cubes_download_indexed(mc._h, pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), faces.ctypes.data_as(C.c_void_p)))
        bf.capi.write_ply_indexed(path, pos, col, faces)
        t3 = time.perf_counter()
        print("mesh (device route, stage by stage): extract %.4f s, weld %.4f s, download + write %.4f s" % (t1 - t0, t2 - t1, t3 - t2))
    else:
        prm = bf.capi.MeshCleanParams(a.mesh_min_faces, int(a.mesh_largest), int(a.mesh_normals)); cm = bf.capi.CleanMesh(); st = bf.capi.MeshCleanStats()
        check(lib.bf_marching_cubes_clean(mc._h, None, C.byref(prm), C.byref(cm), C.byref(st)))
        check(lib.bf_marching_cubes_clean_labels(mc._h, None, 0))                # waits for the object's stream: the clean's last kernels have ended
        t3 = time.perf_counter()
        pos = np.empty((cm.numVertices, 3), np.float32); col = np.empty((cm.numVertices, 3), np.float32); faces = np.empty((cm.numFaces, 3), np.uint32)
        nrm = np.empty((cm.numVertices, 3), np.float32) if a.mesh_normals else None
        check(lib.bf_marching_cubes_download_clean(mc._h, pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p) if a.mesh_normals else None,
                                                   faces.ctypes.data_as(C.c_void_p)))
        bf.capi.write_ply_indexed_normals(path, pos, nrm, col, faces)
        t4 = time.perf_counter()
        print("mesh (device route, stage by stage): extract %.4f s, weld %.4f s, clean %.4f s, download + write %.4f s" % (t1 - t0, t2 - t1, t3 - t2, t4 - t3))
    mc.close()


def _host(p, path, a):
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
    print("mesh (host route) %s: %d vertices, %d faces, %d triangles; extract + copy %.3f s, weld + write %.3f s, total %.3f s" % (path, nv, nf, found, t1 - t0, t2 - t1, t2 - t0))
    if a.mesh_recolour:
        pos, col, faces = mc.weld()
        t3 = time.perf_counter()
        cp, cc, cn, cf, st, _ = bf.capi.mesh_clean_host(pos, col, faces, a.mesh_min_faces, a.mesh_largest, True)
        t4 = time.perf_counter()
        frames, K, w, h = p.mesh_recolour_frames_host(_stride(p, a))
        t5 = time.perf_counter()
        rc, _, rst = bf.capi.mesh_recolour_host(cp, cn, cc, frames, w, h, K, _recolour_params(p, a))
        t6 = time.perf_counter()
        print("mesh (host route) cleaned on one core: %s; clean %.3f s" % (_stats_line(st), t4 - t3))
        print("mesh (host route) recoloured on one core: %s; frames to the host %.3f s, recolour %.3f s" % (_recolour_line(rst), t5 - t4, t6 - t5))
        if a.mesh_simplify_cell > 0:
            sp, sc_, sn, sf, sst, _ = bf.capi.mesh_simplify_host(cp, rc, cf, a.mesh_simplify_cell, a.mesh_normals)
            t7 = time.perf_counter()
            bf.capi.write_ply_indexed_normals(path, sp, sn, sc_, sf)
            print("mesh (host route) simplified on one core: %s; simplify %.3f s, write %.3f s" % (_simplify_line(sst), t7 - t6, time.perf_counter() - t7))
        else:
            bf.capi.write_ply_indexed_normals(path, cp, cn if a.mesh_normals else None, rc, cf)
            print("mesh (host route) write %.3f s" % (time.perf_counter() - t6))
    elif a.mesh_simplify_cell > 0:
        pos, col, faces = mc.weld()
        t3 = time.perf_counter()
        cp, cc, _, cf, st, _ = bf.capi.mesh_clean_host(pos, col, faces, a.mesh_min_faces, a.mesh_largest, False)
        t4 = time.perf_counter()
        sp, sc_, sn, sf, sst, _ = bf.capi.mesh_simplify_host(cp, cc, cf, a.mesh_simplify_cell, a.mesh_normals)
        t5 = time.perf_counter()
        bf.capi.write_ply_indexed_normals(path, sp, sn, sc_, sf)
        t6 = time.perf_counter()
        print("mesh (host route) cleaned on one core: %s; clean %.3f s" % (_stats_line(st), t4 - t3))
        print("mesh (host route) simplified on one core: %s; simplify %.3f s, write %.3f s" % (_simplify_line(sst), t5 - t4, t6 - t5))
    elif _cleaning(a):
        pos, col, faces = mc.weld()                          # the arrays of the host weld (the device weld of the same extraction holds the same bits)
        t3 = time.perf_counter()
        cp, cc, cn, cf, st, _ = bf.capi.mesh_clean_host(pos, col, faces, a.mesh_min_faces, a.mesh_largest, a.mesh_normals)
        t4 = time.perf_counter()
        bf.capi.write_ply_indexed_normals(path, cp, cn, cc, cf)
        t5 = time.perf_counter()
        print("mesh (host route) cleaned on one core: %s; clean %.3f s, write %.3f s" % (_stats_line(st), t4 - t3, t5 - t4))
    mc.close()


def read_ply_mesh(path):
    """(positions [nv,3] float32, faces [nf,3] uint32) of a binary little-endian PLY as this library writes them (float / uchar vertex properties, faces as a
    uchar-counted int list, optionally followed by a uchar-counted float list)"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and "format binary_little_endian 1.0" in lines, "not a binary little-endian PLY"
    nv = nf = 0; fields = []; section = None; face_lists = 0
    for ln in lines:
        t = ln.split()
        if t[:1] == ["element"]:
            section = t[1]
            if section == "vertex": nv = int(t[2])
            if section == "face": nf = int(t[2])
        elif t[:1] == ["property"] and section == "vertex":
            fields.append((t[2], {"float": "<f4", "uchar": "u1", "int": "<i4", "double": "<f8"}[t[1]]))
        elif t[:2] == ["property", "list"] and section == "face":
            face_lists += 1
    vt = np.dtype(fields)
    v = np.frombuffer(body, vt, nv)
    ft = np.dtype([("n", "u1"), ("v", "<u4", 3)] + ([("m", "u1"), ("uv", "<f4", 6)] if face_lists == 2 else []))
    f = np.frombuffer(body, ft, nf, nv * vt.itemsize)
    assert (f["n"] == 3).all(), "a face that is not a triangle"
    return np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32), np.ascontiguousarray(f["v"], np.uint32)


def _distance_line(name, st, voxel):
    s = bf.capi.mesh_distance_summary(st, (voxel,))
    return ("%s: %d samples (%d faces of the samples' mesh and %d of the surface degenerate); mean %.5f m, rms %.5f m, median %.5f m, 90 %% %.5f m, max %.5f m; within one voxel (%g m) %.4f; "
            "beyond %g m %.4f" % (name, s["samples"], st["numDegenerateA"], st["numDegenerateB"], s["mean"], s["rms"], s["median"], s["p90"], s["max"], voxel, s["within_%g" % voxel],
                                  st["max_distance"], s["beyond_share"]))


def _evaluate(p, a):
    """the measurement from the frame loop in both directions, then stage by stage on an object of its own (the error PLY from there), then the one-core route"""
    import torch
    from bundlefusion_amd import synth
    capi = bf.capi
    ref = read_ply_mesh(a.mesh_evaluate_against) if a.mesh_evaluate_against else synth.room_mesh()
    what = a.mesh_evaluate_against or "synth.room_mesh()"
    # the reconstruction lives in its first camera's frame; the room's surface in the scene's: the first frame's true pose takes the scan there (a PLY on disk is
    # taken to be in the scan's frame already)
    first = getattr(a, "first", 0)
    T = None if a.mesh_evaluate_against else synth.trajectory_pose(first, bob=getattr(a, "bob", 0.0))
    D, spacing, voxel = a.mesh_evaluate_max, a.mesh_evaluate_spacing, float(p.gas.s_SDFVoxelSize)
    cell = a.mesh_simplify_cell if a.mesh_simplify_cell > 0 else None
    smode, sspacing = (1, spacing) if a.mesh_evaluate_surface else (0, 0.0)
    t0 = time.perf_counter()
    cst, sst, acc, nt = p.measure_mesh(ref, D, 0, sspacing, smode, cell, T, a.mesh_min_faces, a.mesh_largest)
    t1 = time.perf_counter()
    _, _, com, _ = p.measure_mesh(ref, D, 1, spacing, 1, cell, T, a.mesh_min_faces, a.mesh_largest)
    t2 = time.perf_counter()
    print("mesh evaluation against %s (%d vertices, %d faces), %d triangles; cleaned: %s;%s" % (what, len(ref[0]), len(ref[1]), nt, _stats_line(cst),
                                                                                               " simplified at %g m: %s;" % (cell, _simplify_line(sst)) if sst else ""))
    print("  " + _distance_line("accuracy (scan -> reference, %s)" % ("surface every %g m" % spacing if smode else "vertices"), acc, voxel) + "; bf_pipeline_measure_mesh %.3f s" % (t1 - t0))
    print("  " + _distance_line("completeness (reference -> scan, surface every %g m)" % spacing, com, voxel) + "; bf_pipeline_measure_mesh %.3f s" % (t2 - t1))
    # stage by stage
    mc = capi.MarchingCubesHashSDF.from_global_app_state(p.gas)
    t0 = time.perf_counter()
    mc.extract_gpu(p.scene())
    capi.check(capi.lib.bf_marching_cubes_weld(mc._h, None, 0, capi.mat16(T) if T is not None else None, None))
    pos, col, _, faces, _ = mc.clean(None, a.mesh_min_faces, a.mesh_largest, False)
    if cell:
        pos, col, _, faces, _ = mc.simplify(None, cell, False)
    t1 = time.perf_counter()
    refd = (torch.from_numpy(ref[0]).cuda(), torch.from_numpy(ref[1].view(np.int32)).cuda())
    scand = (torch.from_numpy(pos).cuda(), torch.from_numpy(faces.view(np.int32)).cuda())
    times = []
    for _ in range(2):
        t2 = time.perf_counter()
        st0 = mc.distance(None, refd, D, sspacing, smode, download=False)
        times.append(time.perf_counter() - t2)
    t3 = time.perf_counter()
    st1 = mc.distance(refd, scand, D, spacing, 1, download=False)
    t4 = time.perf_counter()
    print("mesh evaluation (device route, stage by stage): extract + weld + clean%s + download %.4f s; scan -> reference %.4f s (first call, buffers allocated) and %.4f s; reference -> scan %.4f s"
          % (" + simplify" if cell else "", t1 - t0, times[0], times[1], t4 - t3))
    if a.mesh_error_ply:
        d = mc.distance(None, refd, D, 0.0, 0)[0]
        capi.write_ply_indexed_error(a.mesh_error_ply, pos, faces, d, D)
        print("mesh error PLY %s: %d vertices coloured blue (0) through green to red (%g m), %d beyond in magenta" % (a.mesh_error_ply, len(d), D, int(np.isinf(d).sum())))
    mc.close()
    if a.mesh_host:
        # one direction only: the one-core route walks the rings of its grid out to maxDistance for every sample that has nothing near it, which the millions
        # of surface samples of the reference -> scan direction make minutes
        t5 = time.perf_counter()
        h0 = capi.mesh_distance_host((pos, faces), ref, D, sspacing, smode)
        t6 = time.perf_counter()
        same = np.array_equal(h0[3]["histogram"], st0["histogram"]) and {k: v for k, v in h0[3].items() if k != "histogram"} == {k: v for k, v in st0.items() if k != "histogram"}
        print("mesh evaluation (host route) on one core (bf_mesh_distance_host): scan -> reference %.3f s; its summary %s the device's" % (t6 - t5, "is" if same else "IS NOT"))


def write(p, a):
    """p: the Pipeline after process_end_of_sequence / synchronize; a: the parsed arguments"""
    if a.mesh_evaluate or a.mesh_evaluate_against:
        _evaluate(p, a)
    if a.mesh and a.mesh_texture:
        _textured(p, a)
        return
    if a.mesh:
        t0 = time.perf_counter()
        if a.mesh_recolour:
            st, rst, sst, nt = p.save_mesh_recoloured(a.mesh, None, a.mesh_min_faces, a.mesh_largest, a.mesh_normals, _recolour_params(p, a), _stride(p, a),
                                                      a.mesh_simplify_cell if a.mesh_simplify_cell > 0 else None)
            dt = time.perf_counter() - t0
            print("mesh (device route) %s: %d triangles; cleaned: %s; recoloured: %s;%s bf_pipeline_save_mesh_recoloured %.3f s"
                  % (a.mesh, nt, _stats_line(st), _recolour_line(rst), " simplified at %g m: %s;" % (a.mesh_simplify_cell, _simplify_line(sst)) if sst else "", dt))
            _device_stages_recolour(p, a.mesh, a)
            if a.mesh_host:
                _host(p, a.mesh_host, a)
            return
        if a.mesh_simplify_cell > 0:
            st, sst, nt = p.save_mesh_simplified(a.mesh, a.mesh_simplify_cell, None, a.mesh_min_faces, a.mesh_largest, a.mesh_normals)
            dt = time.perf_counter() - t0
            print("mesh (device route) %s: %d triangles; cleaned: %s; simplified at %g m: %s; bf_pipeline_save_mesh_simplified %.3f s"
                  % (a.mesh, nt, _stats_line(st), a.mesh_simplify_cell, _simplify_line(sst), dt))
        elif _cleaning(a):
            st, nt = p.save_mesh_clean(a.mesh, None, a.mesh_min_faces, a.mesh_largest, a.mesh_normals)
            dt = time.perf_counter() - t0
            print("mesh (device route) %s: %d triangles; %s; bf_pipeline_save_mesh_clean %.3f s" % (a.mesh, nt, _stats_line(st), dt))
        else:
            nv, nf, nt = p.save_mesh(a.mesh)
            dt = time.perf_counter() - t0
            print("mesh (device route) %s: %d vertices, %d faces, %d triangles; bf_pipeline_save_mesh %.3f s" % (a.mesh, nv, nf, nt, dt))
        _device_stages(p, a.mesh, a)
    if a.mesh_host:
        _host(p, a.mesh_host, a)
