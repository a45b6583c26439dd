"""CPU tests of the mesh cleaning's host side: bf_mesh_clean_host (the definition on one core) against the numpy restatement tests/mesh_clean_ref.py - positions,
colours and normals compared as uint32, faces, labels and stats exactly: tolerance 0 -, the restatement's labelling against a sequential union-find, and
bf_write_ply_indexed_normals against the byte builder.  The families, orders and sizes are those of tests/test_mesh_clean_gpu.py."""
import numpy as np
import pytest

from tests import mesh_clean_ref as ref
from tests import mesh_weld_ref

SIZES = [0, 1, 2, 63, 64, 65, 257, 1025, 4097]
PARAMS = [(0, False), (ref.M, False), (0, True), (ref.M, True)]          # (min_faces, largest); normals always on


@pytest.fixture(scope="module")
def capi(built):
    from bundlefusion_amd import capi
    return capi


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    """(positions, colours, normals, faces, stats, labels) of two cleans: every array the same shape and the same bits, the stats equal"""
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, dict):
            if {n: g[n] for n in ref.STAT_KEYS} != w:
                return "stats %r != %r" % (g, w)
        elif w is None or g is None:
            if g is not w:
                return "array %d: one is None" % k
        elif g.shape != w.shape or not np.array_equal(_bits(g), _bits(w)):
            return "array %d differs (shapes %r %r)" % (k, g.shape, w.shape)
    return None


@pytest.mark.parametrize("order", ref.ORDERS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_clean_host_vs_restatement(capi, family, order):
    for T in SIZES:
        mesh = ref.build(family, T, seed=T, order=order)
        for min_faces, largest in PARAMS:
            want = ref.clean(*mesh, min_faces, largest, True)
            got = capi.mesh_clean_host(*mesh, min_faces, largest, True)
            err = same(got, want)
            assert err is None, (family, order, T, min_faces, largest, err)


@pytest.mark.parametrize("order", ref.ORDERS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_restatement_labels_vs_sequential_union_find(family, order):
    for T in [t for t in SIZES if t <= 1025]:
        pos, _, faces = ref.build(family, T, seed=T, order=order)
        a = ref.labels(len(pos), faces); b = ref.labels_union_find(len(pos), faces)
        assert np.array_equal(a, b), (family, order, T)
        assert np.array_equal(a[a], a) and (a <= np.arange(len(pos))).all()


def test_planted_families_hold_what_they_plant():
    m = ref.M
    for order in ref.ORDERS:
        st = ref.clean(*ref.islands(65, 1, order))[4]
        assert st["numComponents"] == 65 and st["largestComponentFaces"] == 1 and st["numVerticesOut"] == 195 and st["numIsolatedVertices"] == 0
        pos, col, faces = ref.strip(257, 2, order)
        st = ref.clean(pos, col, faces)[4]
        assert st["numComponents"] == 1 and st["numFacesOut"] == 257 and len(pos) == 259
        pos, col, faces = ref.fan(257, 3, order)
        assert np.bincount(faces.reshape(-1)).argmax() == len(pos) - 1 and np.bincount(faces.reshape(-1)).max() == 257          # the hub carries the highest id
        # patches: the threshold separates M - 1 from M; the tie between the two large ones goes to the lower label
        mesh = ref.patches(257, 4, order)
        out = ref.clean(*mesh, 0, False); st = out[4]
        assert st["numComponents"] == 6 and st["numComponentsKept"] == 6 and st["numFacesOut"] == 4 * m + 2 * 257
        st = ref.clean(*mesh, m, False)[4]
        assert st["numComponentsKept"] == 5 and st["numFacesOut"] == 3 * m + 1 + 2 * 257
        st = ref.clean(*mesh, m + 2, False)[4]
        assert st["numComponentsKept"] == 2
        big = ref.clean(*mesh, m, True)
        lab = out[5]; size = np.bincount(lab[mesh[2][:, 0]], minlength=len(lab))
        tied = np.nonzero(size == 257)[0]
        assert len(tied) == 2 and big[4]["numComponentsKept"] == 1 and big[4]["numFacesOut"] == 257
        assert np.array_equal(_bits(big[0]), _bits(mesh[0][lab == tied.min()]))
        # bridge: one component either way, and the bridging face sits on the three highest ids
        for through in ("face", "vertex"):
            pos, col, faces = ref.bridge(257, 5, order, through)
            st = ref.clean(pos, col, faces)[4]
            assert st["numComponents"] == 1 and st["numFacesOut"] == 2 * 257 + (through == "face")
        pos, col, faces = ref.bridge(257, 5, order)
        assert (np.sort(faces, axis=1) == [len(pos) - 3, len(pos) - 2, len(pos) - 1]).all(axis=1).sum() == 1
        # isolated: ids 0 and nv - 1 among the five
        pos, col, faces = ref.isolated(64, 6, order)
        out = ref.clean(pos, col, faces)
        used = np.zeros(len(pos), bool); used[faces.reshape(-1)] = True
        assert out[4]["numIsolatedVertices"] == 5 and not used[0] and not used[-1] and len(out[0]) == len(pos) - 5
        # repeated: faces with two and with three equal ids are there, and count
        pos, col, faces = ref.repeated(64, 7, order)
        two = ((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])); three = (faces[:, 0] == faces[:, 1]) & (faces[:, 1] == faces[:, 2])
        st = ref.clean(pos, col, faces)[4]
        assert two.sum() >= 5 and three.sum() >= 2 and st["numFacesOut"] == len(faces) and st["numIsolatedVertices"] == 1
        st = ref.clean(*ref.mixed(257, 8, order), m, False)[4]
        assert st["numIsolatedVertices"] == 3 and 0 < st["numComponentsKept"] < st["numComponents"]


def test_identity_and_empty_on_the_host(capi):
    mesh = ref.patches(65, 9, "shuffled")
    got = capi.mesh_clean_host(*mesh, 0, False, False)
    assert got[2] is None and all(np.array_equal(_bits(g), _bits(w)) for g, w in zip((got[0], got[1], got[3]), mesh))
    lab = got[5]
    assert np.array_equal(lab[lab], lab) and (lab <= np.arange(len(lab))).all()
    e3 = np.zeros((0, 3), np.float32)
    got = capi.mesh_clean_host(e3, e3, np.zeros((0, 3), np.uint32), 0, False, True)
    assert got[0].shape == (0, 3) and got[3].shape == (0, 3) and got[4] == dict.fromkeys(ref.STAT_KEYS, 0)


def test_normals_edge_cases_on_the_host(capi):
    """a face without area gives (0, 0, 0); a vertex whose face normals cancel gives (0, 0, 0); a sum that overflows to inf gives (0, 0, 0); -0 components survive"""
    pos = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0],                      # collinear
                    [0, 0, 5], [1, 0, 5], [0, 1, 5], [0, 0, 5.5],          # two faces with opposite windings share vertices 3, 4, 5
                    [0, 0, 9], [3e19, 0, 9], [0, 3e19, 9],                 # cross product 9e38 > FLT_MAX
                    [0, 0, 12], [0, 1, 12], [1, 0, 12]], np.float32)       # normal (0, 0, -1): x and y are -0 or +0 by the definition's operations
    faces = np.array([[0, 1, 2], [3, 4, 5], [3, 5, 4], [7, 8, 9], [10, 11, 12], [6, 6, 6]], np.uint32)
    col = np.zeros_like(pos)
    want = ref.clean(pos, col, faces, 0, False, True)
    got = capi.mesh_clean_host(pos, col, faces, 0, False, True)
    assert same(got, want) is None
    n = got[2]
    assert not n[0:3].any() and not n[3:6].any() and not n[7:10].any() and n[10:13, 2].tolist() == [-1.0, -1.0, -1.0] and not n[6].any()


def test_clean_host_refuses_a_face_id_beyond_the_vertices(capi):
    pos, col, faces = ref.strip(65, 1, "ascending")
    bad = faces.copy(); bad[40, 1] = len(pos)
    C = capi.C
    p = capi.MeshCleanParams(0, 0, 1); st = capi.MeshCleanStats()
    outs = [np.full((len(pos), 3), 7.0, np.float32) for _ in range(3)] + [np.full((len(faces), 3), 7, np.uint32), np.full(len(pos), 7, np.uint32)]
    rc = capi.lib.bf_mesh_clean_host(pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), bad.ctypes.data_as(C.c_void_p), len(pos), len(bad), C.byref(p),
                                     *[o.ctypes.data_as(C.c_void_p) for o in outs], len(pos), len(bad), C.byref(st))
    assert rc == -1 and b"numVertices" in capi.lib.bf_last_error()
    assert all((o == 7).all() for o in outs)
    with pytest.raises(Exception):
        capi.mesh_clean_host(pos, col, bad)
    # a capacity too small: BF_ERR_CAPACITY, the stats say what is needed, nothing else is written
    rc = capi.lib.bf_mesh_clean_host(pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), faces.ctypes.data_as(C.c_void_p), len(pos), len(faces), C.byref(p),
                                     *[o.ctypes.data_as(C.c_void_p) for o in outs[:4]], None, len(pos) - 1, len(faces), C.byref(st))
    assert rc == -4 and st.numVerticesOut == len(pos) and st.numFacesOut == 65 and all((o == 7).all() for o in outs)


def test_write_ply_indexed_normals_vs_the_byte_builder(capi, tmp_path):
    rng = np.random.default_rng(3)
    for nv, nf in ((0, 0), (3, 1), (400, 700), (65537, 65537)):          # the writer buffers 65536 records per write
        pos = rng.uniform(-5, 5, (nv, 3)).astype(np.float32); nrm = rng.uniform(-1, 1, (nv, 3)).astype(np.float32); col = rng.uniform(-0.1, 1.1, (nv, 3)).astype(np.float32)
        faces = rng.integers(0, max(nv, 1), (nf, 3)).astype(np.uint32)
        capi.write_ply_indexed_normals(tmp_path / "n.ply", pos, nrm, col, faces)
        raw = (tmp_path / "n.ply").read_bytes()
        assert raw == ref.ply_bytes_normals(pos, nrm, col, faces)
        assert len(raw.split(b"end_header\n", 1)[1]) == 28 * nv + 13 * nf
        # without normals: the file of bf_write_ply_indexed
        capi.write_ply_indexed_normals(tmp_path / "p.ply", pos, None, col, faces)
        capi.write_ply_indexed(tmp_path / "q.ply", pos, col, faces)
        assert (tmp_path / "p.ply").read_bytes() == (tmp_path / "q.ply").read_bytes() == mesh_weld_ref.ply_bytes(pos, col, faces) == ref.ply_bytes_normals(pos, None, col, faces)
    body = raw.split(b"end_header\n", 1)[1]
    assert np.array_equal(np.frombuffer(body[12:24], "<f4"), nrm[0]) and body[27] == 255
    with pytest.raises(Exception):
        capi.write_ply_indexed_normals(tmp_path / "no_such_dir" / "n.ply", pos, nrm, col, faces)
