"""CPU tests of the mesh distance's host side: bf_mesh_distance_host (the definition on one core over its own grid) against the numpy restatement
tests/mesh_distance_ref.py (a brute-force minimum over all faces) - distances and weights compared as uint64 bit patterns, faces, stats and histograms exactly:
tolerance 0 -, the planted edge cases, the refusals, synth.room_mesh() against the renderer, and the error PLY.  The cases are those of
tests/test_mesh_distance_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import mesh_distance_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "bundlefusion_amd", "lib")
SIZES = [1, 63, 64, 65, 257, 1025]
MODES = [(0, 0.0), (1, 0.0), (1, 0.2)]          # (sampleMode, sampleSpacing): vertices; one sample per face; up to 25 per face
D_FAMILY = 0.15


@pytest.fixture(scope="module")
def capi(built):
    from bundlefusion_amd import capi
    return capi


_WANT = {}


def surface_b():
    """the 300-face soup every family is measured against"""
    if "B" not in _WANT:
        _WANT["B"] = ref.soup(300, 1)
    return _WANT["B"]


def want(T, mode, spacing):
    """mesh A of T faces and the restatement's result against surface_b(), computed once and shared (read-only) by the tests of this process"""
    key = (T, mode, spacing)
    if key not in _WANT:
        A = ref.soup(T, 100 + T)
        _WANT[key] = (A, ref.distance(A, surface_b(), D_FAMILY, spacing, mode))
    return _WANT[key]


def test_library_exports_every_symbol_of_the_distance(built):
    """the rule of tests/test_host_cpu.py::test_library_exports_every_declared_symbol, for the header the distance adds to"""
    lib = C.CDLL(os.path.join(LIBDIR, "libbf_hip.so"))
    expect = ["bf_marching_cubes_distance", "bf_marching_cubes_download_distance", "bf_marching_cubes_measure_mesh", "bf_mesh_distance_host", "bf_mesh_distance_sample_count_host", "bf_write_ply_indexed_error"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bf_hip.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"BF_API\s+[\w\s\*]+?\b(bf_\w+)\s*\(", txt)))
    assert all(n in names for n in expect)
    assert not [n for n in names if not hasattr(lib, n)]


@pytest.mark.parametrize("mode,spacing", MODES)
def test_distance_host_vs_restatement(capi, mode, spacing):
    """soups on both sides of zero (cells come from floor, not from truncation): both sample modes, sizes either side of a wave, a workgroup and a tile"""
    for T in SIZES:
        A, w = want(T, mode, spacing)
        err = ref.same(capi.mesh_distance_host(A, surface_b(), D_FAMILY, spacing, mode), w)
        assert err is None, (T, mode, spacing, err)
        st = w[3]
        assert st["numWithin"] > 0 and st["numWithin"] + st["numBeyond"] == st["numSamples"] == len(w[0]) and (T < 257 or st["numBeyond"] > 0)
        assert (np.asarray(A[0]) < 0).any() and (np.asarray(A[0]) > 0).any()
    assert want(1025, 1, 0.2)[1][3]["numSamples"] > 4 * 1025


def boundary_case():
    """a flat sheet at z = 0 and samples at z = 0.25 above its inside"""
    B = ref.sheet(8)
    rng = np.random.default_rng(3)
    pos = np.concatenate([rng.uniform(-0.45, 0.45, (200, 2)), np.full((200, 1), 0.25)], 1).astype(np.float32)
    return (pos, np.zeros((0, 3), np.uint32)), B


def test_inclusive_boundary(capi):
    A, B = boundary_case()
    d, f, w, st = capi.mesh_distance_host(A, B, 0.25)
    assert ref.same((d, f, w, st), ref.distance(A, B, 0.25)) is None
    assert (d == 0.25).all() and st["numWithin"] == 200 and st["maxWithin"] == 0.25 and st["histogram"][1023] == st["sumW"] == 200 << st["scaleW"]
    below = float(np.nextafter(np.float32(0.25), np.float32(0.0)))
    d, f, w, st = capi.mesh_distance_host(A, B, below)
    assert ref.same((d, f, w, st), ref.distance(A, B, below)) is None
    assert np.isinf(d).all() and (f == ref.NONE).all() and st["numBeyond"] == 200 and st["sumW"] == 0 and st["sumWBeyond"] == 200 << st["scaleW"]


def tie_case():
    """faces 3 and 7 share the edge (0,0,0)-(1,0,0); the others lie 5 m away.  The sample above the edge's middle is 0.5 from both, in exact arithmetic"""
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0]] + [[5 + k, 5, 5] for k in range(3)]
    far = [4, 5, 6]
    faces = [far, far, far, [0, 1, 2], far, far, far, [1, 0, 3]]
    return (np.array([[0.5, 0, 0.5], [0.25, 0, -0.125]], np.float32), np.zeros((0, 3), np.uint32)), (np.array(pos, np.float32), np.array(faces, np.uint32))


def test_ties_take_the_lowest_face(capi):
    A, B = tie_case()
    got = capi.mesh_distance_host(A, B, 1.0)
    assert ref.same(got, ref.distance(A, B, 1.0)) is None
    assert list(got[1]) == [3, 3] and list(got[0]) == [0.5, 0.125]


def test_self_distance_is_zero(capi):
    from bundlefusion_amd import synth
    for mesh in (synth.room_mesh(), ref.sheet(5)):
        d, f, w, st = capi.mesh_distance_host(mesh, mesh, 0.1)
        assert ref.same((d, f, w, st), ref.distance(mesh, mesh, 0.1)) is None
        used = np.zeros(len(mesh[0]), bool); used[mesh[1].ravel()] = True
        assert used.all() and (d == 0.0).all() and st["maxWithin"] == 0.0 and st["sumWD"] == 0 and st["histogram"][0] == st["sumW"]


def degenerate_case():
    """a sheet with three degenerate faces put in front of, between and behind its own: two equal ids, collinear corners, a NaN corner"""
    pos, faces = ref.sheet(4)
    nv = len(pos)
    pos = np.concatenate([pos, np.array([[0, 0, 0.5], [0.25, 0, 0.5], [0.5, 0, 0.5], [np.nan, 0, 0]], np.float32)])
    bad = np.array([[0, 0, 5], [nv, nv + 1, nv + 2], [1, 2, nv + 3]], np.uint32)
    faces = np.concatenate([bad[:1], faces[:10], bad[1:2], faces[10:], bad[2:]])
    return pos, faces


def test_degenerate_faces_are_skipped_and_counted(capi):
    mesh = degenerate_case()
    rng = np.random.default_rng(5)
    A = (rng.uniform(-0.6, 0.6, (300, 3)).astype(np.float32), np.zeros((0, 3), np.uint32))
    got = capi.mesh_distance_host(A, mesh, 0.4)
    assert ref.same(got, ref.distance(A, mesh, 0.4)) is None
    assert got[3]["numDegenerateB"] == 3 and not np.isin(got[1], [0, 11, len(mesh[1]) - 1]).any()
    # the same faces in A give no samples (surface mode reads no other vertex: the NaN is not refused)
    for spacing in (0.0, 0.1):
        got = capi.mesh_distance_host(mesh, ref.sheet(3, z=0.1), 0.4, spacing, 1)
        w = ref.distance(mesh, ref.sheet(3, z=0.1), 0.4, spacing, 1)
        assert ref.same(got, w) is None and got[3]["numDegenerateA"] == 3 and got[3]["numSamples"] == (32 if spacing == 0.0 else len(w[0]))


def test_empty_inputs(capi):
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    B = ref.soup(10, 2)
    for mode in (0, 1):
        d, f, w, st = capi.mesh_distance_host(empty, B, 0.5, 0.1, mode)
        assert len(d) == len(f) == len(w) == 0 and st["numSamples"] == 0 and st["sumW"] == 0 and ref.same((d, f, w, st), ref.distance(empty, B, 0.5, 0.1, mode)) is None
        for none in (empty, (B[0], np.array([[0, 0, 1]], np.uint32))):          # no face, or degenerate faces only
            got = capi.mesh_distance_host(B, none, 0.5, 0.1, mode)
            assert ref.same(got, ref.distance(B, none, 0.5, 0.1, mode)) is None
            assert got[3]["numSamples"] > 0 and got[3]["numBeyond"] == got[3]["numSamples"] and np.isinf(got[0]).all() and (got[1] == ref.NONE).all()


def large_face_case():
    """one 6 m oblique triangle; samples within 5 cm of it, just beyond, and far from it inside its bounding box"""
    B = (np.array([[-3, -1, -2], [3, 0.5, 1], [-1, 2.5, 2]], np.float32), np.array([[0, 1, 2]], np.uint32))
    a, b, c = B[0].astype(np.float64)
    n = np.cross(b - a, c - a); n /= np.linalg.norm(n)
    rng = np.random.default_rng(7)
    uv = rng.uniform(0, 1, (600, 2)); uv = np.where(uv.sum(1, keepdims=True) > 1, 1 - uv, uv)
    on = a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a)
    off = np.concatenate([rng.uniform(-0.049, 0.049, 400), rng.uniform(0.051, 0.2, 100), rng.uniform(0.5, 2.0, 100)])
    return (np.asarray(on + off[:, None] * n, np.float32), np.zeros((0, 3), np.uint32)), B


def test_one_large_oblique_face(capi):
    A, B = large_face_case()
    got = capi.mesh_distance_host(A, B, 0.05)
    assert ref.same(got, ref.distance(A, B, 0.05)) is None
    assert 380 <= got[3]["numWithin"] <= 420


def distant_vertex_case():
    """the family's surface with a vertex no face uses 900 m away, and behind it a small triangle there"""
    pos, faces = surface_b()
    nv = len(pos)
    far = np.array([[900, 900, -900], [900, 0, 0], [900.01, 0, 0], [900, 0.01, 0]], np.float32)
    return (np.concatenate([pos, far]), np.concatenate([faces, np.array([[nv + 1, nv + 2, nv + 3]], np.uint32)]))


def test_a_distant_vertex_changes_nothing(capi):
    """... and costs nothing: the process's peak resident size grows by less than 64 MiB over the call (the pairs of 301 faces are kilobytes; a dense grid over
    the 1800 m bounding box at the host's cell of some 0.1 m would be 10^12 cells)"""
    import resource
    A, w = want(257, 0, 0.0)
    B = distant_vertex_case()
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    got = capi.mesh_distance_host(A, B, D_FAMILY)
    grown = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before          # KiB
    assert ref.same(got, w) is None
    assert grown < 64 << 10, grown


def sliver_cases():
    """long slivers, whose normal a cross product of nearly parallel edges gives badly: (A, B, D) with a 4.6 m sliver as the only face of B, its third corner
    1e-6, 1e-4, 5e-4 (below the 2^-10 at which the plane test is trusted), 2e-3 and 2e-2 of the long edge away from it; samples along and around it"""
    rng = np.random.default_rng(21)
    a = np.array([-2.0, -1.0, 0.3]); b = np.array([2.0, 1.3, -0.4])
    e = b - a
    perp = np.cross(e, [0.3, -0.2, 1.0]); perp /= np.linalg.norm(perp)
    cases = []
    for rel in (1e-6, 1e-4, 5e-4, 2e-3, 2e-2):
        c = a + 0.37 * e + rel * np.linalg.norm(e) * perp
        B = (np.array([a, b, c], np.float32), np.array([[0, 1, 2]], np.uint32))
        t = rng.uniform(-0.02, 1.02, (400, 1))
        pts = a + t * e + rng.normal(0, 0.03, (400, 3))
        cases.append(((pts.astype(np.float32), np.zeros((0, 3), np.uint32)), B, 0.05))
    return cases


def test_long_slivers(capi):
    for A, B, D in sliver_cases():
        got = capi.mesh_distance_host(A, B, D)
        assert ref.same(got, ref.distance(A, B, D)) is None
        assert got[3]["numDegenerateB"] == 0 and 50 < got[3]["numWithin"] < 400


def overflow_case(leg=11.3):
    """four faces of A whose one sample weighs just below 64 m^2, 63.9 m below a surface, D = 64: every term is near the top of its range, and with L = 2 the
    sums come within a factor of two of 2^62, the bound the scales were chosen for"""
    pos, faces = [], []
    for k in range(4):
        x = -30.0 + 15.0 * k
        pos += [[x, 0, 0], [x + leg, 0, 0], [x, leg, 0]]; faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    B = (np.array([[-500, -400, 63.9], [600, -400, 63.9], [0, 700, 63.9]], np.float32), np.array([[0, 1, 2]], np.uint32))
    return (np.array(pos, np.float32), np.array(faces, np.uint32)), B


def test_sums_and_histogram_at_the_overflow_boundary(capi):
    A, B = overflow_case()
    got = capi.mesh_distance_host(A, B, 64.0, 0.0, 1)
    w = ref.distance(A, B, 64.0, 0.0, 1)
    assert ref.same(got, w) is None
    st = got[3]
    assert (st["scaleW"], st["scaleWD"], st["scaleWD2"]) == (62 - 2 - 6, 62 - 2 - 6 - 6, 62 - 2 - 6 - 12) and st["numWithin"] == 4
    assert 2 ** 61 < st["sumW"] < 2 ** 62 and 2 ** 61 < st["sumWD"] < 2 ** 62 and 2 ** 61 < st["sumWD2"] < 2 ** 62
    assert st["histogram"].sum() == st["sumW"] and st["histogram"][int(63.9 * 16)] == st["sumW"]
    # one step over: a sample of 64 m^2 or more is refused
    with pytest.raises(Exception, match="64 square metres"):
        capi.mesh_distance_host(overflow_case(11.32)[0], B, 64.0, 0.0, 1)
    # the other end: the smallest D, one vertex: the scales grow, the terms do not
    one = (np.array([[0, 0, 2.0 ** -21]], np.float32), np.zeros((0, 3), np.uint32))
    got = capi.mesh_distance_host(one, ref.sheet(1), 2.0 ** -20)
    assert ref.same(got, ref.distance(one, ref.sheet(1), 2.0 ** -20)) is None
    assert got[3]["scaleWD2"] == 102 and got[3]["sumWD2"] == 2 ** 60 and got[3]["sumWD"] == 2 ** 61 and got[3]["sumW"] == 2 ** 62


def refusal_cases():
    """(name, A, B, maxDistance, sampleSpacing, sampleMode): every input the definition refuses but the one of 300 000 001 faces"""
    A, B = ref.soup(65, 4), surface_b()
    cases = [("maxDistance %r" % d, A, B, d, 0.0, 0) for d in (0.0, -1.0, float("nan"), float("inf"), 64.5)]
    cases += [("sampleSpacing %r" % s, A, B, 0.3, s, 1) for s in (-0.1, float("nan"), float("inf"))]
    cases.append(("sampleMode 2", A, B, 0.3, 0.0, 2))
    bad = A[1].copy(); bad[30, 1] = len(A[0]); cases.append(("a face id of nv in A", (A[0], bad), B, 0.3, 0.0, 0))
    bad = B[1].copy(); bad[299, 2] = len(B[0]); cases.append(("a face id of nv in B", A, (B[0], bad), 0.3, 0.0, 1))
    bad = A[0].copy(); bad[17, 1] = np.nan; cases.append(("a NaN vertex of A in vertex mode", (bad, A[1]), B, 0.3, 0.0, 0))
    bad = A[0].copy(); bad[3, 2] = 1024.0; cases.append(("a vertex of A at 1024 in vertex mode", (bad, A[1]), B, 0.3, 0.0, 0))
    cases.append(("a corner of A at 1024 in surface mode", (bad, A[1]), B, 0.3, 0.0, 1))
    bad = B[0].copy(); bad[B[1][7, 0], 0] = -1024.0; cases.append(("a corner of B at -1024", A, (bad, B[1]), 0.3, 0.0, 0))
    bad = A[0].copy(); bad[A[1][5, 0], 1] = 2000.0; fd = A[1].copy(); fd[5, 1] = fd[5, 0]          # two equal ids: degenerate, and still refused
    cases.append(("a corner at 2000 of a degenerate face of A in surface mode", (bad, fd), B, 0.3, 0.0, 1))
    bad = B[0].copy(); bad[B[1][9, 2], 2] = 1e30; cases.append(("a corner of B at 1e30, whose face's N2 overflows", A, (bad, B[1]), 0.3, 0.0, 0))
    cases.append(("a face of A with n above 1024", A, B, 0.3, 1e-5, 1))
    cases.append(("a sample of 64 m^2", overflow_case(11.32)[0], B, 0.3, 0.0, 1))
    big = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.tile(np.array([[0, 1, 2]], np.uint32), (300, 1)))
    cases.append(("more than 2^28 samples", big, B, 0.3, float(np.sqrt(2.0) / 1023.5), 1))
    return cases


def raw_host_call(capi, A, B, D, nfa=None, nfb=None):
    """bf_mesh_distance_host with face counts of the caller's choosing: (status, the output array, stats.numSamples), both planted with sevens"""
    pa, fa = capi._host_mesh(A); pb, fb = capi._host_mesh(B)
    p = capi.MeshDistanceParams(D, 0.0, 0); st = capi.MeshDistanceStats()
    st.numSamples = 7777
    out = np.full(16, 7.0)
    rc = capi.lib.bf_mesh_distance_host(pa.ctypes.data_as(C.c_void_p), fa.ctypes.data_as(C.c_void_p), C.c_uint32(len(pa)), C.c_uint32(len(fa) if nfa is None else nfa),
                                        pb.ctypes.data_as(C.c_void_p), fb.ctypes.data_as(C.c_void_p), C.c_uint32(len(pb)), C.c_uint32(len(fb) if nfb is None else nfb), C.byref(p),
                                        out.ctypes.data_as(C.c_void_p), None, None, C.c_uint32(16), C.byref(st))
    return rc, out, st.numSamples


def test_distance_host_refuses_more_than_300_000_000_faces(capi):
    """the count is refused before any array is read, so small arrays do: 300 000 001 faces in A, then in B; 300 000 000 is not refused for its count (not run:
    its arrays would be read)"""
    A, B = ref.soup(65, 4), surface_b()
    for nfa, nfb in ((300000001, None), (None, 300000001), (0xFFFFFFFF, None)):
        rc, out, n = raw_host_call(capi, A, B, 0.3, nfa, nfb)
        assert rc == -1 and (out == 7.0).all() and n == 7777 and b"too many faces" in capi.lib.bf_last_error()
    n = C.c_uint64(7)
    pa, fa = capi._host_mesh(A); p = capi.MeshDistanceParams(0.3, 0.0, 1)
    assert capi.lib.bf_mesh_distance_sample_count_host(pa.ctypes.data_as(C.c_void_p), fa.ctypes.data_as(C.c_void_p), C.c_uint32(len(pa)), C.c_uint32(300000001), C.byref(p), C.byref(n)) == -1
    assert n.value == 7
    assert raw_host_call(capi, A, B, 0.3)[0] == 0


def test_distance_host_refusals_write_nothing(capi):
    for name, A, B, D, spacing, mode in refusal_cases():
        pa, fa = capi._host_mesh(A); pb, fb = capi._host_mesh(B)
        p = capi.MeshDistanceParams(D, spacing, mode); st = capi.MeshDistanceStats()
        st.numSamples = 7777
        out = np.full(16, 7.0)
        rc = capi.lib.bf_mesh_distance_host(pa.ctypes.data_as(C.c_void_p), fa.ctypes.data_as(C.c_void_p), C.c_uint32(len(pa)), C.c_uint32(len(fa)), pb.ctypes.data_as(C.c_void_p),
                                            fb.ctypes.data_as(C.c_void_p), C.c_uint32(len(pb)), C.c_uint32(len(fb)), C.byref(p), out.ctypes.data_as(C.c_void_p), None, None, C.c_uint32(16),
                                            C.byref(st))
        assert rc == -1 and (out == 7.0).all() and st.numSamples == 7777, name
    # just inside: 1023.99994, D = 64, n = 1024 exactly
    A, B = ref.soup(65, 4), surface_b()
    ok = A[0].copy(); ok[3, 2] = np.nextafter(np.float32(1024.0), np.float32(0.0))
    for mode, spacing in ((0, 0.0), (1, 50.0)):          # (a face that reaches 1 km has to be cut, or its one sample would weigh more than 64 m^2)
        assert ref.same(capi.mesh_distance_host((ok, A[1]), B, 64.0, spacing, mode), ref.distance((ok, A[1]), B, 64.0, spacing, mode)) is None
    one = (np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.5, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    got = capi.mesh_distance_host(one, ref.sheet(2), 0.5, 1.0 / 1024.0, 1)
    assert got[3]["numSamples"] == 1024 * 1024 and got[3]["numWithin"] > 0


def test_room_mesh_is_the_surface_the_renderer_draws(capi):
    """every valid depth pixel of six frames at 160 x 120, back-projected in binary64 under the frame's pose, lies within 1e-6 m of synth.room_mesh().  The bar is
    derived: the binary32 rounding of a depth below 4 m is at most half an ulp, 2.4e-7 m; the pose's and the corners' binary32 roundings are of that size; a
    pixel's ray is at most 1.3 times longer than its depth."""
    from bundlefusion_amd import synth
    mesh = synth.room_mesh()
    assert mesh[0].shape == (72, 3) and mesh[0].dtype == np.float32 and mesh[1].shape == (108, 3) and mesh[1].dtype == np.uint32
    assert not ref.corners(*mesh)[4].any()
    worst = 0.0
    for k in (0, 20, 40, 450, 900, 1300):
        depth, _, T, K = synth.scene_room(k, 160, 120)
        ys, xs = np.nonzero(np.isfinite(depth))
        assert len(xs) > 10000
        z = depth[ys, xs].astype(np.float64)
        cam = np.stack([(xs - K["mx"]) / K["fx"] * z, (ys - K["my"]) / K["fy"] * z, z], 1)
        p = cam @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
        d = np.sqrt(ref.nearest(p, mesh)[0])
        print("frame %d: %d pixels, max distance to room_mesh() %.3g m" % (k, len(p), d.max()))
        worst = max(worst, float(d.max()))
    assert worst <= 1e-6


def test_error_ply_bytes(capi, tmp_path):
    mesh = ref.sheet(6)
    rng = np.random.default_rng(11)
    d = rng.uniform(0, 0.12, len(mesh[0]))
    d[::7] = np.inf; d[3] = 0.0; d[4] = float(np.float32(0.1)); d[5] = np.nan; d[6] = 0.05
    capi.write_ply_indexed_error(tmp_path / "err.ply", mesh[0], mesh[1], d, 0.1)
    assert (tmp_path / "err.ply").read_bytes() == ref.error_ply_bytes(mesh[0], mesh[1], d, 0.1)
    head, body = (tmp_path / "err.ply").read_bytes().split(b"end_header\n")
    rec = np.frombuffer(body[:16 * len(mesh[0])], np.dtype([("p", "<f4", 3), ("c", "u1", 4)]))
    assert tuple(rec["c"][0]) == (255, 0, 255, 255) and tuple(rec["c"][3]) == (0, 0, 255, 255) and tuple(rec["c"][4]) == (255, 0, 0, 255) and tuple(rec["c"][5]) == (255, 0, 255, 255)
