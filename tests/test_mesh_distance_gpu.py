"""GPU tests (-m gpu) of the device mesh distance (csrc/meshdistance.hip) and of the entry points built on it, against the numpy restatement
tests/mesh_distance_ref.py (a brute-force minimum over all faces) and the host route.  Bar: distances and weights compared as uint64 bit patterns; faces, stats and
histograms exactly - tolerance 0.

Sizes: the kernels work in 64-lane waves and 256-thread workgroups, scan the faces' sample counts and the grid's table slots in tiles of 1024 and the tile sums 256
at a time.  63 / 64 / 65 faces are either side of a wave, 257 just above a workgroup, 1025 just above a tile; more than 262 144 faces of A, and a table of more than
262 144 slots, are past one step of the tile scan.  The shapes are the smallest that reach each mechanism, not the scan's."""
import gc as _gc

import numpy as np
import pytest

from bundlefusion_amd import synth
from tests import mesh_distance_ref as ref
from tests import test_mesh_weld_gpu as weld_gpu
from tests.test_mesh_distance_cpu import (D_FAMILY, MODES, SIZES, boundary_case, degenerate_case, distant_vertex_case, large_face_case, overflow_case, refusal_cases, sliver_cases,
                                          surface_b, tie_case, want)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc(gpu):
    return gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)


def _upload(mesh):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(mesh[0], np.float32).reshape(-1, 3)).cuda(), torch.from_numpy(np.ascontiguousarray(mesh[1], np.uint32).reshape(-1, 3).view(np.int32)).cuda())


def _distance(mc, A, B, D, spacing=0.0, mode=0):
    return mc.distance(_upload(A) if A is not None else None, _upload(B), D, spacing, mode)


@pytest.mark.parametrize("mode,spacing", MODES)
def test_distance_planted_families(mc, mode, spacing):
    Bd = _upload(surface_b())
    for T in SIZES:
        A, w = want(T, mode, spacing)
        err = ref.same(mc.distance(_upload(A), Bd, D_FAMILY, spacing, mode), w)
        assert err is None, (T, mode, spacing, err)


def test_distance_planted_edge_cases(gpu, mc):
    """the CPU test's cases on the device: the inclusive boundary, the tie, the degenerate faces on either side, the empty inputs, the top of the sums' range"""
    A, B = boundary_case()
    got = _distance(mc, A, B, 0.25)
    assert ref.same(got, ref.distance(A, B, 0.25)) is None and (got[0] == 0.25).all()
    below = float(np.nextafter(np.float32(0.25), np.float32(0.0)))
    got = _distance(mc, A, B, below)
    assert ref.same(got, ref.distance(A, B, below)) is None and got[3]["numBeyond"] == 200
    A, B = tie_case()
    got = _distance(mc, A, B, 1.0)
    assert ref.same(got, ref.distance(A, B, 1.0)) is None and list(got[1]) == [3, 3]
    mesh = degenerate_case()
    A = (np.random.default_rng(5).uniform(-0.6, 0.6, (300, 3)).astype(np.float32), np.zeros((0, 3), np.uint32))
    got = _distance(mc, A, mesh, 0.4)
    assert ref.same(got, ref.distance(A, mesh, 0.4)) is None and got[3]["numDegenerateB"] == 3
    got = _distance(mc, mesh, ref.sheet(3, z=0.1), 0.4, 0.1, 1)
    assert ref.same(got, ref.distance(mesh, ref.sheet(3, z=0.1), 0.4, 0.1, 1)) is None and got[3]["numDegenerateA"] == 3
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    for mode in (0, 1):
        assert ref.same(_distance(mc, empty, surface_b(), 0.5, 0.1, mode), ref.distance(empty, surface_b(), 0.5, 0.1, mode)) is None
        got = _distance(mc, surface_b(), empty, 0.5, 0.3, mode)
        assert ref.same(got, ref.distance(surface_b(), empty, 0.5, 0.3, mode)) is None and got[3]["numBeyond"] == got[3]["numSamples"] > 0
    A, B = overflow_case()
    got = _distance(mc, A, B, 64.0, 0.0, 1)
    assert ref.same(got, ref.distance(A, B, 64.0, 0.0, 1)) is None and 2 ** 61 < got[3]["sumWD2"] < 2 ** 62
    room = synth.room_mesh()
    got = _distance(mc, room, room, 0.1)
    assert ref.same(got, ref.distance(room, room, 0.1)) is None and (got[0] == 0.0).all()


def test_distance_faces_past_one_step_of_the_tile_scan(mc):
    """263 538 faces of A in surface mode, one sample each: more than 262 144 samples, and 258 tiles of sample counts"""
    A = ref.sheet(363, size=2.0, x0=-1.0, y0=-1.0)
    B = ref.soup(20, 9)
    assert len(A[1]) > 262144
    got = _distance(mc, A, B, 0.2, 0.0, 1)
    w = ref.distance(A, B, 0.2, 0.0, 1)
    assert ref.same(got, w) is None and w[3]["numSamples"] == len(A[1]) and 0 < w[3]["numWithin"] < len(A[1])


def test_distance_crowded_cell_twice(gpu, mc):
    """5000 faces of B and 100 000 samples in one cell of the grid: two runs give the same bits, those of the host route.  (The search walks a cell's list from
    global memory in one piece: there is no LDS chunk for 5000 faces to cross; what the case holds is 100 000 threads on one list filled by 5000 contending
    atomics, in whatever order those left it.)"""
    rng = np.random.default_rng(12)
    centre = rng.uniform(0.06, 0.44, (5000, 1, 3))
    B = ((centre + rng.uniform(-0.01, 0.01, (5000, 3, 3))).reshape(-1, 3).astype(np.float32), np.arange(15000, dtype=np.uint32).reshape(-1, 3))
    A = (rng.uniform(0.05, 0.45, (100000, 3)).astype(np.float32), np.zeros((0, 3), np.uint32))
    assert (np.floor(B[0].astype(np.float64) / (0.5 * 1.0009765625)) == 0).all() and (np.floor(A[0].astype(np.float64) / (0.5 * 1.0009765625)) == 0).all()
    Ad, Bd = _upload(A), _upload(B)
    a = mc.distance(Ad, Bd, 0.5); b = mc.distance(Ad, Bd, 0.5)
    assert ref.same(b, a) is None and ref.same(a, gpu.capi.mesh_distance_host(A, B, 0.5)) is None
    assert a[3]["numWithin"] == 100000 and len(np.unique(a[1])) > 2000


def test_distance_large_face_and_distant_vertex_stay_bounded(gpu):
    """one 6 m oblique face at D = 0.05 is listed in the cells its plane crosses, not in the 1.7 million of its bounding box; a vertex 900 m away costs nothing.
    Bound: a (face, cell) pair costs 4 bytes and at most 4 table slots of 16 bytes, a face 36 bytes and a sample 20; the oblique face is some 2 10^5 pairs: 16 MiB
    covers both cases with the fixed 9 KiB of accumulators.  A dense grid over the distant vertex's bounding box would be terabytes."""
    _gc.collect()
    live = gpu.capi.debug_live_resources()
    m = gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)
    base = gpu.capi.debug_live_resources()[2]
    A, B = large_face_case()
    got = _distance(m, A, B, 0.05)
    assert ref.same(got, ref.distance(A, B, 0.05)) is None and 380 <= got[3]["numWithin"] <= 420
    assert gpu.capi.debug_live_resources()[2] - base < 16 << 20
    A, w = want(257, 0, 0.0)
    assert ref.same(_distance(m, A, distant_vertex_case(), D_FAMILY), w) is None
    assert gpu.capi.debug_live_resources()[2] - base < 16 << 20
    m.close()
    _gc.collect()
    assert gpu.capi.debug_live_resources()[:4] == live[:4] and gpu.capi.debug_live_resources()[5] == 0


def test_distance_small_after_large_and_refusals(gpu, mc):
    large, w_large = want(1025, 1, 0.2)
    assert ref.same(_distance(mc, large, surface_b(), D_FAMILY, 0.2, 1), w_large) is None
    live = gpu.capi.debug_live_resources()
    small, w = want(65, 1, 0.2)
    assert ref.same(_distance(mc, small, surface_b(), D_FAMILY, 0.2, 1), w) is None
    assert gpu.capi.debug_live_resources()[:4] == live[:4]          # the larger buffers serve the smaller mesh
    n = len(w[0])
    for name, A, B, D, spacing, mode in refusal_cases():
        with pytest.raises(Exception):
            _distance(mc, A, B, D, spacing, mode)
        # the last result is still there, unchanged
        assert ref.same(mc.download_distance(n) + (w[3],), w) is None, name
    assert gpu.capi.debug_live_resources()[:4] == live[:4]


def test_distance_refuses_more_than_300_000_000_faces_with_the_last_result_intact(gpu, mc):
    """the count is refused before any array is read, so the meshes of a small case do, with numFaces overwritten: in A, then in B"""
    import ctypes as C
    capi = gpu.capi
    small, w = want(65, 0, 0.0)
    Ad, Bd = _upload(small), _upload(surface_b())
    assert ref.same(mc.distance(Ad, Bd, D_FAMILY), w) is None
    live = capi.debug_live_resources()
    for which in (0, 1):
        meshes = [capi.IndexedMesh(t[0].data_ptr(), None, t[1].data_ptr(), t[0].numel() // 3, t[1].numel() // 3) for t in (Ad, Bd)]
        meshes[which].numFaces = 300000001
        p = capi.MeshDistanceParams(D_FAMILY, 0.0, 0); st = capi.MeshDistanceStats()
        st.numSamples = 7777
        assert capi.lib.bf_marching_cubes_distance(mc._h, C.byref(meshes[0]), C.byref(meshes[1]), C.byref(p), C.byref(st)) == -1
        assert st.numSamples == 7777 and b"too many faces" in capi.lib.bf_last_error()
        assert ref.same(mc.download_distance(len(w[0])) + (w[3],), w) is None
    assert capi.debug_live_resources()[:4] == live[:4]


def test_distance_long_slivers(gpu, mc):
    """faces whose normal cannot be trusted are listed in every cell of their box: the device, the host route and the brute-force minimum agree"""
    for A, B, D in sliver_cases():
        assert ref.same(_distance(mc, A, B, D), ref.distance(A, B, D)) is None


def test_distance_without_a_mesh_refuses_a_null_input(gpu):
    m = gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)
    with pytest.raises(Exception, match="weld"):
        m.distance(None, _upload(surface_b()), 0.1)
    m.close()


# --------------------------------------------------------------------------- behind the weld, the clean and the simplify
CELL = 0.05


def _figures(gpu, name, st):
    s = gpu.capi.mesh_distance_summary(st, (0.02,))
    print("%s: %d samples, mean %.4f rms %.4f median %.4f p90 %.4f max %.4f m, within 2 cm %.3f, beyond %.4f"
          % (name, s["samples"], s["mean"], s["rms"], s["median"], s["p90"], s["max"], s["within_0.02"], s["beyond_share"]))


def test_distance_behind_the_weld_the_clean_and_the_simplify_on_a_volume(gpu):
    """the three-frame 160 x 120 volume at 2 cm of tests/test_mesh_weld_gpu.py: `a` NULL takes the weld's, then the clean's, then the simplification's mesh"""
    gs, p = weld_gpu._volume(gpu)
    m = gpu.capi.MarchingCubesHashSDF(600000, p.m_hashNumBuckets, 0.02)
    n, found = m.extract_gpu(gs)
    assert n == found > 5000
    room = synth.room_mesh()
    roomd = _upload(room)
    welded = m.weld(None)
    got = m.distance(None, roomd, 0.1)
    assert ref.same(got, gpu.capi.mesh_distance_host((welded[0], welded[2]), room, 0.1)) is None and got[3]["numSamples"] == len(welded[0])
    cleaned = m.clean(None, 41, False, False)
    cmesh = (cleaned[0], cleaned[3])
    # cleaned against the room, both directions, both sample modes: the device equals the host route on the downloaded arrays.  No quality threshold: the figures
    # are printed, nobody has measured them before
    for mode, spacing in ((0, 0.0), (1, 0.01)):
        got = m.distance(None, roomd, 0.1, spacing, mode)
        assert ref.same(got, gpu.capi.mesh_distance_host(cmesh, room, 0.1, spacing, mode)) is None
        _figures(gpu, "cleaned -> room (mode %d)" % mode, got[3])
    got = m.distance(roomd, _upload(cmesh), 0.1, 0.02, 1)
    assert ref.same(got, gpu.capi.mesh_distance_host(room, cmesh, 0.1, 0.02, 1)) is None
    _figures(gpu, "room -> cleaned (three frames see little of it)", got[3])
    simp = m.simplify(None, CELL, False)
    got = m.distance(None, _upload(cmesh), 0.1)
    assert ref.same(got, gpu.capi.mesh_distance_host((simp[0], simp[3]), cmesh, 0.1)) is None
    _figures(gpu, "simplified (5 cm) -> cleaned", got[3])
    # a cluster's representative is the mean of members that lie on the input surface: within the diagonal of its cell (tests/test_mesh_simplify_gpu.py's bound)
    assert got[3]["numBeyond"] == 0 and got[3]["numSamples"] == len(simp[0]) > 0 and got[3]["maxWithin"] <= np.sqrt(3.0) * (CELL + 2e-6)
    m.close()


# --------------------------------------------------------------------------- the frame loop
MIN_FACES = 100
D_LOOP = 0.1


def _run_pipeline(gpu, measure):
    """the 25-frame configuration of tests/test_mesh_simplify_gpu.py::_run_pipeline; measure: measure the mesh after frame 12 and after the last frame"""
    import torch
    from tests.test_mesh_simplify_gpu import _pipeline
    gp, gas, frames = _pipeline(gpu)
    room = synth.room_mesh()
    results = []
    for k, (d, c, T, _) in enumerate(frames):
        assert gp.process_frame(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda())
        if measure and k == 12:
            results.append(gp.measure_mesh(room, D_LOOP, 0, cell_size=CELL, min_faces=MIN_FACES))
    if measure:
        results.append(gp.measure_mesh(room, D_LOOP, 0, cell_size=CELL, min_faces=MIN_FACES))
        results.append(gp.measure_mesh(room, D_LOOP, 1, 0.02, 1, min_faces=MIN_FACES))
    gp.synchronize()
    return gp, gas, results


def test_pipeline_measure_mesh_leaves_the_reconstruction_alone(gpu):
    """one run measures the mesh after frame 12 and after the last frame, the other never: the same trajectories, bf_scene_debug_hash, heap free count, allocated
    blocks and counters; the final stats are the stand-alone route's (extract -> weld -> clean -> simplify -> distance)"""
    plain, _, _ = _run_pipeline(gpu, False)
    a = weld_gpu._volume_state(plain)
    plain.close()
    gp, gas, results = _run_pipeline(gpu, True)
    b = weld_gpu._volume_state(gp)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
    assert np.array_equal(bits(a["traj"]), bits(b["traj"])) and np.array_equal(bits(a["opt"]), bits(b["opt"]))
    assert a["dbg"] == b["dbg"] and a["heap_free"] == b["heap_free"] and a["blocks"] == b["blocks"] and a["counters"] == b["counters"]
    room = synth.room_mesh()
    m = gpu.capi.MarchingCubesHashSDF.from_global_app_state(gas, max_triangles=3000000)
    n, found = m.extract_gpu(gp.scene())
    assert n == found > 5000
    m.weld(None)
    cleaned = m.clean(None, MIN_FACES, False, False)
    simp = m.simplify(None, CELL, False)
    own = m.distance(None, _upload(room), D_LOOP)
    cst, sst, dst, nt = results[1]
    assert nt == found and cst == cleaned[4] and sst == simp[4] and ref.same(own[:3] + (dst,), own) is None and dst["numSamples"] == len(simp[0]) > 0
    own = m.distance(_upload(room), _upload((cleaned[0], cleaned[3])), D_LOOP, 0.02, 1)
    assert results[2][1] is None and ref.same(own[:3] + (results[2][2],), own) is None
    assert 0 < results[0][2]["numSamples"] != dst["numSamples"]
    _figures(gpu, "25 frames, simplified scan -> room", dst); _figures(gpu, "25 frames, room -> cleaned scan", results[2][2])
    c = weld_gpu._volume_state(gp)
    assert c["dbg"] == b["dbg"] and c["heap_free"] == b["heap_free"] and c["blocks"] == b["blocks"]
    m.close()
    gp.close()


def test_pipeline_measure_mesh_refuses_a_sharded_volume(gpu):
    from tests.test_mesh_simplify_gpu import _pipeline
    gp, _, _ = _pipeline(gpu)
    gp.set_volume_shard(0, 2)
    with pytest.raises(Exception, match="shard"):
        gp.measure_mesh(synth.room_mesh(), D_LOOP)
    gp.close()
