"""CPU tests of the mesh simplification's host side: bf_mesh_simplify_host (the definition on one core) against the numpy restatement tests/mesh_simplify_ref.py -
positions, colours and normals compared as uint32, faces, map and stats exactly: tolerance 0 -, the vectorised restatement against its sequential form, what the
planted families plant, the refusals, and the C / C++ surface.  The families, orders and sizes are those of tests/test_mesh_simplify_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_simplify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "bundlefusion_amd", "lib")
SIZES = [0, 1, 2, 63, 64, 65, 257, 1025, 4097]


@pytest.fixture(scope="module")
def capi(built):
    from bundlefusion_amd import capi
    return capi


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    """(positions, colours, normals, faces, stats, map) of two simplifications: every array the same shape and the same bits, the stats equal"""
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


_WANT = {}


def want(family, T, order, normals):
    """the restatement's result, computed once and shared (read-only) by the tests of this process"""
    key = (family, T, order, normals)
    if key not in _WANT:
        mesh = ref.build(family, T, seed=T, order=order)
        _WANT[key] = (mesh, ref.simplify(*mesh[:4], normals))
    return _WANT[key]


@pytest.mark.parametrize("order", ref.ORDERS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_simplify_host_vs_restatement(capi, family, order):
    for T in SIZES:
        for normals in (False, True):
            mesh, w = want(family, T, order, normals)
            err = same(capi.mesh_simplify_host(*mesh[:4], normals), w)
            assert err is None, (family, order, T, normals, err)


@pytest.mark.parametrize("order", ref.ORDERS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_restatement_vectorised_vs_sequential(family, order):
    for T in [t for t in SIZES if t <= 1025]:
        mesh, w = want(family, T, order, True)
        err = same(ref.simplify_sequential(*mesh[:4], True), w)
        assert err is None, (family, order, T, err)
        st = w[4]
        assert st["numFacesIn"] == st["numFacesOut"] + st["numFacesCollapsed"] + st["numFacesDuplicate"] and st["numVerticesOut"] <= st["numClusters"] <= st["numVerticesIn"]


def test_planted_families_hold_what_they_plant():
    """the stats of every family follow from the cells its builder chose (expected_stats works on those integers, not on positions), and each family shows what it
    is there for - a family that degenerates cannot pass silently"""
    for order in ref.ORDERS:
        for family in ref.PLANTED:
            for T in (65, 257):
                pos, col, faces, cell, labels = ref.build(family, T, seed=T, order=order)
                out = ref.simplify(pos, col, faces, cell, True)
                assert out[4] == ref.expected_stats(labels, faces), (family, order, T)
                assert np.array_equal(ref.cell_indices(pos, cell).astype(np.int64), labels), (family, order, T)
        T = 257
        st = ref.simplify(*ref.grid(T, 1, order)[:4])[4]
        assert st["largestCluster"] == 9 and st["numFacesCollapsed"] > st["numFacesOut"] > 0 and st["numFacesDuplicate"] > 0
        pos, col, faces, cell, labels = ref.straddle(T, 2, order)
        assert (np.signbit(pos) & (pos == 0)).any() and (~np.signbit(pos) & (pos == 0)).any() and set(np.unique(labels)) == {-1, 0}
        assert ref.simplify(pos, col, faces, cell)[4]["numClusters"] == 8
        pos, col, faces, cell, labels = ref.boundary(T, 3, order)
        k = np.rint(pos.astype(np.float64) / cell)
        on = pos.astype(np.float64) == k * cell
        assert on.any() and (~on).any() and (labels[on] == k[on]).all() and (labels[~on] == k[~on] - 1).all() and labels.min() < 0 < labels.max()
        st = ref.simplify(*ref.hub(T, 4, order)[:4])[4]
        assert st["largestCluster"] == T and st["numClusters"] == 9 and st["numFacesOut"] == 8 and st["numFacesDuplicate"] == T - 8
        pos, col, faces, cell, labels = ref.sheets(T, 5, order)
        out = ref.simplify(pos, col, faces, cell)
        assert out[4]["numFacesOut"] == T and out[4]["numFacesDuplicate"] == T and out[4]["largestCluster"] == 2
        # the face with the lower index stays, with its winding: the output faces are the first occurrences, mapped
        tri = np.sort(out[5][faces].astype(np.int64), axis=1)
        _, firsts = np.unique(tri, axis=0, return_index=True)
        assert np.array_equal(out[3], out[5][faces[np.sort(firsts)]])
        if order == "shuffled":
            c = labels[faces[np.sort(firsts)].astype(np.int64)]          # the kept faces in cell coordinates: the sheets differ in the sign of the area
            area = (c[:, 1, 0] - c[:, 0, 0]) * (c[:, 2, 1] - c[:, 0, 1]) - (c[:, 1, 1] - c[:, 0, 1]) * (c[:, 2, 0] - c[:, 0, 0])
            assert (area > 0).any() and (area < 0).any()          # faces of both sheets stay
        pos, col, faces, cell, labels = ref.singles(T, 6, order)
        out = ref.simplify(pos, col, faces, cell)
        assert np.array_equal(_bits(out[0]), _bits(pos)) and np.array_equal(_bits(out[1]), _bits(col)) and np.array_equal(out[3], faces)
        assert np.array_equal(out[5], np.arange(len(pos))) and not np.array_equal(ref.quant(pos).astype(np.float64) / 1048576.0, pos.astype(np.float64))
        pos, col, faces, cell, labels = ref.speck(T, 7, order)
        out = ref.simplify(pos, col, faces, cell); st = out[4]
        gone = np.nonzero(out[5] == ref.NONE)[0]
        assert st["numFacesCollapsed"] == 4 and st["numFacesOut"] == T and st["numClusters"] == st["numVerticesOut"] + 1 and len(gone) == 4 and st["largestCluster"] == 4
        there = np.nonzero(out[5] != ref.NONE)[0]
        assert np.array_equal(np.sort(out[5][there]), np.arange(len(pos) - 4)) and (out[5][there] != there).any()          # later ids shift
        pos, col, faces, cell, labels = ref.isolated(T, 8, order)
        out = ref.simplify(pos, col, faces, cell); st = out[4]
        unused = np.ones(len(pos), bool); unused[faces.reshape(-1)] = False
        assert unused.sum() > 60 and st["largestCluster"] == 2 and st["numVerticesOut"] == st["numClusters"] == len(pos) - unused.sum() and (out[5][unused] != ref.NONE).all()
        assert (np.bincount(out[5], minlength=len(out[0])) == 2).sum() == unused.sum()
        assert (_bits(out[0][out[5][unused]]) != _bits(pos[unused])).any(axis=1).all()          # the unused vertex is in the mean, and is not the mean
    for name in ("patches", "mixed"):
        mesh = ref.build(name + "@fine", 257, 9, "shuffled"); st = ref.simplify(*mesh[:4])[4]
        assert st["numClusters"] > 0.9 * st["numVerticesIn"]
        mesh = ref.build(name + "@coarse", 257, 9, "shuffled"); st = ref.simplify(*mesh[:4])[4]
        assert 0 < st["numFacesOut"] < st["numFacesIn"] and st["largestCluster"] > 2
        mesh = ref.build(name + "@swallow", 257, 9, "shuffled"); st = ref.simplify(*mesh[:4])[4]
        assert st["numClusters"] == 1 and st["numVerticesOut"] == 0 and st["numFacesOut"] == 0 and st["numFacesCollapsed"] == st["numFacesIn"]


def _raw_call(capi, pos, col, faces, cell, vcap=None, fcap=None, normals=1):
    """bf_mesh_simplify_host on outputs pre-filled with 7: (status, outputs, stats)"""
    pos = np.ascontiguousarray(pos, np.float32); col = np.ascontiguousarray(col, np.float32); faces = np.ascontiguousarray(faces, np.uint32)
    p = capi.MeshSimplifyParams(cell, normals); st = capi.MeshSimplifyStats()
    outs = [np.full((len(pos), 3), 7.0, np.float32) for _ in range(3)] + [np.full((len(faces), 3), 7, np.uint32), np.full(len(pos), 7, np.uint32)]
    rc = capi.lib.bf_mesh_simplify_host(pos.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), faces.ctypes.data_as(C.c_void_p), len(pos), len(faces), C.byref(p),
                                        *[o.ctypes.data_as(C.c_void_p) for o in outs], len(pos) if vcap is None else vcap, len(faces) if fcap is None else fcap, C.byref(st))
    return rc, outs, st


def refusal_cases():
    """(name, positions, colours, faces, cell size): every input the definition refuses"""
    pos, col, faces, cell, _ = ref.grid(65, 1, "shuffled")
    cases = [("cellSize %r" % c, pos, col, faces, c) for c in (0.0, -1.0, float("nan"), float("inf"))]
    bad = pos.copy(); bad[17, 1] = np.nan; cases.append(("a NaN position", bad, col, faces, cell))
    bad = pos.copy(); bad[3, 2] = 1024.0; cases.append(("a position of 1024", bad, col, faces, cell))
    bad = col.copy(); bad[40, 0] = 1024.0; cases.append(("a colour of 1024", pos, bad, faces, cell))
    bad = pos.copy(); bad[9, 0] = 500.0; cases.append(("a cell index beyond 2^20", bad, col, faces, 1e-4))
    bad = faces.copy(); bad[30, 1] = len(pos); cases.append(("a face id of nv", pos, col, bad, cell))
    return cases


def test_simplify_host_refusals_leave_the_outputs_alone(capi):
    for name, pos, col, faces, cell in refusal_cases():
        rc, outs, _ = _raw_call(capi, pos, col, faces, cell)
        assert rc == -1 and all((o == 7).all() for o in outs), name
        with pytest.raises(ValueError):
            ref.simplify(pos, col, faces, cell)
    # just inside: 1023.99994 and a cell index of 2^20 - 1 are taken
    pos, col, faces, cell, _ = ref.grid(65, 1, "shuffled")
    ok = pos.copy(); ok[3, 2] = np.nextafter(np.float32(1024.0), np.float32(0.0))
    assert same(capi.mesh_simplify_host(ok, col, faces, cell, True), ref.simplify(ok, col, faces, cell, True)) is None
    edge = pos.copy(); edge[9, 0] = np.float32(1048575.5 * 2.0 ** -11); edge[10, 0] = -np.float32(1048574.5 * 2.0 ** -11)          # cells 2^20 - 1 and -(2^20 - 1)
    assert same(capi.mesh_simplify_host(edge, col, faces, 2.0 ** -11, True), ref.simplify(edge, col, faces, 2.0 ** -11, True)) is None
    edge[10, 0] = -np.float32(1048575.5 * 2.0 ** -11)          # floor gives -2^20
    assert _raw_call(capi, edge, col, faces, 2.0 ** -11)[0] == -1


def test_simplify_host_capacity(capi):
    pos, col, faces, cell, _ = ref.grid(257, 2, "shuffled")
    w = ref.simplify(pos, col, faces, cell, True)
    nv, nf = len(w[0]), len(w[3])
    for vcap, fcap in ((nv - 1, nf), (nv, nf - 1)):
        rc, outs, st = _raw_call(capi, pos, col, faces, cell, vcap, fcap)
        assert rc == -4 and {k: getattr(st, k) for k in ref.STAT_KEYS} == w[4] and all((o == 7).all() for o in outs)
    rc, outs, st = _raw_call(capi, pos, col, faces, cell, nv, nf)
    assert rc == 0 and np.array_equal(_bits(outs[0][:nv]), _bits(w[0])) and np.array_equal(outs[4], w[5]) and (outs[0][nv:] == 7).all()


def big_sum_mesh(seed=0):
    """One cell of 1024 m holds 8 400 000 vertices with x in [1023.5, 1024) and 4097 with x in [0, 1), and the cell below zero their mirror images: the sum of q(x)
    passes 2^53, and the small members give it low bits that binary64 cannot hold - the int64 -> binary64 conversion of the definition rounds.  Three faces to
    vertices in other cells keep both clusters in the output."""
    for s in range(seed, seed + 20):
        rng = np.random.default_rng(s)
        big = rng.uniform(1023.5, 1024.0, 8400000).astype(np.float32); big = np.minimum(big, np.nextafter(np.float32(1024.0), np.float32(0.0)))
        x = np.concatenate([big, rng.uniform(0.0, 1.0, 4097).astype(np.float32)])
        S = int(ref.quant(x).sum())
        if S > 2 ** 53 and int(np.float64(S)) != S:
            break
    else:
        raise AssertionError("no seed gives a sum that binary64 cannot hold")
    half = np.stack([x, rng.uniform(0.0, 1000.0, len(x)).astype(np.float32), rng.uniform(0.0, 1000.0, len(x)).astype(np.float32)], 1)
    others = np.array([[1.0, -1.0, 1.0], [1.0, 1.0, -1.0], [-1.0, -1.0, 1.0], [-1.0, 1.0, -1.0]], np.float32)          # four more cells of 1024 m
    pos = np.concatenate([half, half * np.array([-1.0, 1.0, 1.0], np.float32), others]).astype(np.float32)
    n = len(half)
    col = rng.uniform(0.0, 1.0, (len(pos), 3)).astype(np.float32)
    faces = np.array([[0, 2 * n, 2 * n + 1], [n, 2 * n + 2, 2 * n + 3], [0, n, 2 * n]], np.uint32)
    return pos, col, faces, 1024.0, S


@pytest.fixture(scope="module")
def big_sum():
    mesh = big_sum_mesh()
    return mesh, ref.simplify(*mesh[:4], True)


def test_sum_beyond_2_53_host_vs_restatement(capi, big_sum):
    (pos, col, faces, cell, S), w = big_sum
    big = pos[:8400000, 0]
    qb = ref.quant(big)
    assert int(qb.sum()) > 2 ** 53 and (qb % 64 == 0).all()          # the large members alone pass 2^53, in multiples of 64
    assert S > 2 ** 53 and int(np.float64(S)) != S                             # the sum of the cluster is not a binary64 number
    assert w[4]["largestCluster"] == 8404097 and w[4]["numVerticesOut"] == 6 and w[4]["numFacesOut"] == 3
    assert same(capi.mesh_simplify_host(pos, col, faces, cell, True), w) is None


def test_library_exports_every_symbol_of_the_simplification(built):
    """the rule of tests/test_host_cpu.py::test_library_exports_every_declared_symbol, for the two headers the simplification adds to"""
    lib = C.CDLL(os.path.join(LIBDIR, "libbf_hip.so"))
    for header, expect in (("bf_hip.h", ["bf_marching_cubes_simplify", "bf_marching_cubes_simplify_map", "bf_marching_cubes_download_simplified",
                                         "bf_marching_cubes_save_mesh_simplified", "bf_mesh_simplify_host"]), ("bf_pipeline.h", ["bf_pipeline_save_mesh_simplified"])):
        txt = open(os.path.join(ROOT, "include", header)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        names = sorted(set(re.findall(r"BF_API\s+[\w\s\*]+?\b(bf_\w+)\s*\(", txt)))
        assert all(n in names for n in expect), header
        missing = [n for n in names if not hasattr(lib, n)]
        assert not missing, missing


_WRAPPER_CPP = r'''
#include "bundlefusion/bundlefusion.hpp"
using namespace bundlefusion;
int main(int argc, char** argv) {
    // the host route needs no device: one cell swallows a triangle, two cells keep nothing of it either, three keep it
    const float pos[9] = {0.1f, 0.1f, 0.1f, 1.1f, 0.1f, 0.1f, 0.1f, 1.1f, 0.1f}, col[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
    const uint32_t faces[3] = {0, 1, 2};
    bf_mesh_simplify_params sp = {1.0f, 1};
    bf_mesh_simplify_stats st;
    float op[9], oc[9], on[9]; uint32_t of[3], map[3];
    if (bf_mesh_simplify_host(pos, col, faces, 3, 1, &sp, op, oc, on, of, map, 3, 1, &st) != BF_OK) return 2;
    if (st.numClusters != 3 || st.numFacesOut != 1 || on[2] != 1.0f || op[3] != 1.1f) return 3;
    std::printf("host ok\n");
    if (argc > 1) {          // never taken by the test: the wrappers only have to build and link
        CUDAMarchingCubesHashSDF mc(MarchingCubesParams{});
        bf_mesh_clean_params cp = {100, 0, 1};
        bf_clean_mesh m = mc.simplify(sp, &st);
        mc.saveMeshSimplified(std::string(argv[1]), cp, sp, nullptr, nullptr, &st);
        return (int)m.numVertices;
    }
    return 0;
}
'''


def test_cpp_simplify_wrappers_compile_and_link(built, tmp_path):
    """CUDAMarchingCubesHashSDF::simplify / saveMeshSimplified of bundlefusion.hpp build with plain g++ (no HIP headers) and resolve against libbf_hip.so, as
    tests/test_render_cpp.py checks the render wrappers"""
    src = tmp_path / "wrap.cpp"; src.write_text(_WRAPPER_CPP)
    exe = tmp_path / "wrap"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", LIBDIR, "-lbf_hip", "-Wl,-rpath," + LIBDIR, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "host ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
