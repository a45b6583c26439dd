"""CPU tests of the mesh weld's host side: bf_write_ply_indexed (the one PLY writer of bf_marching_cubes_save_mesh and bf_marching_cubes_save_mesh_gpu) against the
byte builder of tests/mesh_weld_ref.py, tolerance 0, and the two forms of the restatement against each other."""
import numpy as np
import pytest

from tests import mesh_weld_ref as ref


@pytest.fixture(scope="module")
def capi(built):
    from bundlefusion_amd import capi
    return capi


def _written(capi, tmp_path, pos, col, faces):
    path = tmp_path / "m.ply"
    capi.write_ply_indexed(path, pos, col, faces)
    return path.read_bytes()


def _colour_edge_values():
    """colours c where c * 255.0f + 0.5f is exactly an integer k (c = (k - 0.5) / 255 rounded, when the binary32 product and sum land on k), and the binary32
    neighbours of each either side"""
    k = np.arange(0, 258, dtype=np.float64)
    c = ((k - 0.5) / 255.0).astype(np.float32)
    hit = c[(c * np.float32(255.0) + np.float32(0.5)) == k.astype(np.float32)]
    assert len(hit) > 50
    return np.concatenate([hit, np.nextafter(hit, np.float32(np.inf)), np.nextafter(hit, np.float32(-np.inf))]).astype(np.float32)


def test_write_ply_indexed_empty_and_one_face(capi, tmp_path):
    e3 = np.zeros((0, 3), np.float32)
    raw = _written(capi, tmp_path, e3, e3, np.zeros((0, 3), np.uint32))
    assert raw == ref.ply_bytes(e3, e3, np.zeros((0, 3), np.uint32)) and raw.endswith(b"end_header\n") and b"element vertex 0\n" in raw and b"element face 0\n" in raw
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, -2.5, 1e-3]], np.float32); col = np.array([[-0.1, 0.0, 1.0], [1.5, 0.5, 0.25], [0.999, 0.001, 0.3333]], np.float32)
    faces = np.array([[2, 0, 1]], np.uint32)
    raw = _written(capi, tmp_path, pos, col, faces)
    assert raw == ref.ply_bytes(pos, col, faces)
    body = raw.split(b"end_header\n", 1)[1]
    assert len(body) == 3 * 16 + 13
    assert body[12:16] == bytes([0, 0, 255, 255]) and body[28:32] == bytes([255, 128, 64, 255])          # -0.1 -> 0, 1.5 -> 255, 0.5 -> 128, alpha 255
    assert body[48] == 3 and np.frombuffer(body[49:61], "<i4").tolist() == [2, 0, 1]


def test_write_ply_indexed_colour_rounding_and_a_few_hundred_faces(capi, tmp_path):
    rng = np.random.default_rng(5)
    edge = _colour_edge_values()
    n = 3 * ((len(edge) + 8 + 2) // 3)
    col = np.zeros(n, np.float32)
    col[:len(edge)] = edge
    col[len(edge):len(edge) + 8] = [-0.1, 0.0, 1.0, 1.5, -0.0, 0.5, 254.5 / 255.0, 255.5 / 255.0]
    col = col.reshape(-1, 3)
    pos = rng.uniform(-50, 50, col.shape).astype(np.float32)
    faces = rng.integers(0, len(pos), (400, 3)).astype(np.uint32)
    raw = _written(capi, tmp_path, pos, col, faces)
    assert raw == ref.ply_bytes(pos, col, faces)
    assert len(raw.split(b"end_header\n", 1)[1]) == len(pos) * 16 + 400 * 13


def test_write_ply_indexed_more_records_than_one_write(capi, tmp_path):
    """the writer buffers 65536 records per write: one vertex and one face more than that"""
    rng = np.random.default_rng(6)
    n = 65537
    pos = rng.uniform(-1, 1, (n, 3)).astype(np.float32); col = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    faces = rng.integers(0, n, (n, 3)).astype(np.uint32)
    assert _written(capi, tmp_path, pos, col, faces) == ref.ply_bytes(pos, col, faces)


def test_write_ply_indexed_reports_a_path_it_cannot_open(capi, tmp_path):
    e3 = np.zeros((0, 3), np.float32)
    with pytest.raises(Exception):
        capi.write_ply_indexed(tmp_path / "no_such_dir" / "m.ply", e3, e3, np.zeros((0, 3), np.uint32))


@pytest.mark.parametrize("transform", [None, ref.TRANSFORM])
def test_restatements_agree_on_a_planted_soup(transform):
    """400 triangles: corners from a pool of cells with sub-cell jitter, copies, rotations and reflections of other triangles, triangles of their own"""
    tris = ref.soup_mixed(400, seed=3)
    a = ref.weld(tris, transform); b = ref.weld_sequential(tris, transform)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
    nv, nf = len(a[0]), len(a[2])
    assert 100 < nv < 1200 and 100 < nf < 400          # vertices merged, faces dropped: every rule took part
    ids = ref.weld(tris)[2].astype(np.int64)
    assert (ids[:, 0] != ids[:, 1]).all() and len(np.unique(np.sort(ids, axis=1), axis=0)) == nf


@pytest.mark.parametrize("name,T,nv,nf", [("soup_one_cell", 65, 1, 0), ("soup_copies", 65, 3, 1), ("soup_distinct", 65, 195, 65), ("soup_pool", 400, 60, None)])
def test_planted_families_hold_what_they_plant(name, T, nv, nf):
    tris = getattr(ref, name)(T)
    a = ref.weld(tris); b = ref.weld_sequential(tris)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    assert len(a[0]) == nv and (nf is None or len(a[2]) == nf)
    if name == "soup_copies":
        assert a[2].tolist() == [[0, 1, 2]]


def test_boundary_family_sits_on_the_cell_edges():
    v = ref.boundary_values().astype(np.float64)
    frac = v * 1e5 - np.floor(v * 1e5)
    assert np.abs(frac - 0.5).max() < 0.1          # within two binary32 steps of k + 0.5
    keys = np.floor(v * ref.INV + 0.5)
    exact = v[:200]                                 # the j / 64 themselves
    assert len(np.unique(keys)) > 200 and np.array_equal(exact * 64.0, np.round(exact * 64.0))
    tris = ref.soup_boundaries(65)
    a = ref.weld(tris); b = ref.weld_sequential(tris)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
