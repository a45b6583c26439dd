"""CPU tests (-m "not gpu") of the point cloud's definition (DESIGN.md 1 "Point cloud"): the two numpy restatements of tests/point_cloud_ref.py agree on every
planted case of tests/point_cloud_cases.py, the library's host route bf_point_cloud_build_host equals them as bits, bf_write_ply_points writes the bytes assembled
here, and the cases are not vacuous - every family drops a pixel by the rule it is named for and keeps one."""
import numpy as np
import pytest

from tests import point_cloud_cases as cases
from tests import point_cloud_ref as R

CASES = cases.all_cases()
_expected = {}


def expected(case):
    """the vectorised restatement, computed once per case and shared"""
    if case["name"] not in _expected:
        out = R.build(case["frames"], case["Kinv"], case["cell"], case["max_depth"])
        for a in out[:3]:
            a.setflags(write=False)
        _expected[case["name"]] = out
    return _expected[case["name"]]


def same_cloud(got, want):
    return (got[0].shape == want[0].shape and np.array_equal(R.bits(got[0]), R.bits(want[0])) and np.array_equal(R.bits(got[1]), R.bits(want[1]))
            and np.array_equal(got[2], want[2]))


@pytest.fixture(scope="module")
def capi(built):
    from bundlefusion_amd import capi
    return capi


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_two_restatements_agree(case):
    want = expected(case)
    got = R.build_loop(case["frames"], case["Kinv"], case["cell"], case["max_depth"])
    assert got[3] == want[3]
    assert same_cloud(got, want)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_route_equals_the_restatement_as_bits(capi, case):
    want = expected(case)
    ds, cs, Ts = zip(*case["frames"])
    pos, nrm, col, n = capi.point_cloud_build_host(ds, cs, np.stack(Ts), case["Kinv"], case["cell"], case["max_depth"])
    assert n == len(want[0])
    assert same_cloud((pos, nrm, col), want)
    # a capacity below the count: the first points, and still the full count
    if n >= 2:
        p2, n2, c2, m = capi.point_cloud_build_host(ds, cs, np.stack(Ts), case["Kinv"], case["cell"], case["max_depth"], capacity=n // 2)
        assert m == n and same_cloud((p2, n2, c2), tuple(a[:n // 2] for a in want[:3]))


def _reasons(case):
    return [R.frame_candidates(D, C, case["Kinv"], T, case["cell"], case["max_depth"])[0] for D, C, T in case["frames"]]


def test_every_family_drops_by_its_rule_and_keeps_something():
    families = {}
    for c in CASES:
        f = families.setdefault(c["family"], dict(rules=set(), dropped=set(), kept=0, points=0))
        f["rules"] |= set(c["rules"])
        for r in _reasons(c):
            f["dropped"] |= set(np.unique(r).tolist()) - {R.KEPT}
            f["kept"] += int((r == R.KEPT).sum())
        f["points"] += len(expected(c)[0])
    assert set(families) == {"depth", "maxDepth", "border", "normal", "colour", "pose", "one cell", "pool", "distinct", "boundaries", "no thinning"}
    for name, f in families.items():
        assert f["rules"] <= f["dropped"], (name, [R.RULES[r] for r in f["rules"] - f["dropped"]])
        assert f["kept"] > 0 and f["points"] > 0, name
    named = set().union(*(f["rules"] for f in families.values()))
    assert named == set(range(1, 10))          # every rule of the definition is some family's


def test_planted_pixels_fall_as_planted():
    n = 0
    for c in CASES:
        reasons = _reasons(c)
        for f, y, x, why in c.get("expect", ()):
            assert reasons[f][y, x] == why, (c["name"], f, y, x, R.RULES[reasons[f][y, x]], R.RULES[why])
            n += 1
    assert n >= 15
    by = {c["name"]: c for c in CASES}
    # depth specials: the bad pixel has no position, and wherever it sits next to the centre, the centre falls by the neighbour rule
    c = by["depth_specials"]
    reasons = _reasons(c)
    assert len(reasons) == 25
    k = 0
    for v in range(5):
        for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
            r = reasons[k]; k += 1
            if (dx, dy) == (0, 0):
                assert r[3, 3] == R.NO_POSITION and r[3, 2] == r[3, 4] == r[2, 3] == r[4, 3] == R.NEIGHBOUR
            else:
                assert r[3, 3] == R.NEIGHBOUR
                bad = r[3 + dy, 3 + dx]
                assert bad == R.NO_POSITION
    # poses: frame 0 and the rotated frame give points, -inf and NaN poses nothing, +inf translation falls by `world`, +2^31 cells by `cell range`, -2^31 cells stay
    why = [set(np.unique(r[1:-1, 1:-1]).tolist()) for r in _reasons(by["poses"])]
    assert why == [{R.KEPT}, {R.POSE}, {R.POSE}, {R.WORLD}, {R.CELL_RANGE}, {R.KEPT}, {R.CELL_RANGE}, {R.KEPT}]


def test_thinning_families_say_what_they_claim():
    by = {c["name"]: c for c in CASES}
    # one cell: three frames of candidates, one point - frame 0's first candidate, although every candidate differs in position, normal and colour
    c = by["one_cell"]
    pos, nrm, col, ncand = expected(c)
    assert len(pos) == 1 and ncand == 3 * 4 * 6
    reason, P, N, rgba = R.frame_candidates(*c["frames"][0][:2], c["Kinv"], c["frames"][0][2], c["cell"], c["max_depth"])
    assert np.array_equal(R.bits(pos[0]), R.bits(P[1, 1])) and np.array_equal(col[0], rgba[1, 1])
    allP = np.concatenate([R.frame_candidates(D, C, c["Kinv"], T, c["cell"], c["max_depth"])[1][1:-1, 1:-1].reshape(-1, 3) for D, C, T in c["frames"]])
    allN = np.concatenate([R.frame_candidates(D, C, c["Kinv"], T, c["cell"], c["max_depth"])[2][1:-1, 1:-1].reshape(-1, 3) for D, C, T in c["frames"]])
    assert len(np.unique(allP, axis=0)) == len(allP) and len(np.unique(allN, axis=0)) > len(allN) // 2
    # without thinning the same frames give every candidate
    for name in ("no_thinning_0", "no_thinning_-1"):
        assert len(expected(by[name])[0]) == ncand == expected(by[name])[3]
    # pool: some 60 cells, each wanted many times, from every frame
    c = by["pool"]
    pos, _, _, ncand = expected(c)
    assert 40 <= len(pos) <= 90 and ncand > 10 * len(pos)
    per_frame = [R.frame_candidates(D, C, c["Kinv"], T, c["cell"], c["max_depth"]) for D, C, T in c["frames"]]
    cells = [set(map(tuple, R.cells_of(P[r == R.KEPT], c["cell"]).tolist())) for r, P, _, _ in per_frame]
    assert len(cells[0] & cells[1] & cells[2]) > 20
    # distinct: nothing is thinned away
    pos, _, _, ncand = expected(by["distinct"])
    assert len(pos) == ncand == 2 * 4 * 6
    # boundaries: points sit exactly on cell boundaries on both sides of 0, and truncation in place of floor merges other cells
    c = by["boundaries"]
    pos, _, _, ncand = expected(c)
    allP = np.concatenate([R.frame_candidates(D, C, c["Kinv"], T, c["cell"], c["max_depth"])[1][1:-1, 1:-1].reshape(-1, 3) for D, C, T in c["frames"]])
    scaled = allP.astype(np.float64) * R.cell_inverse(c["cell"])
    on = scaled[:, 0] == np.floor(scaled[:, 0])
    assert (on & (scaled[:, 0] < 0)).any() and (on & (scaled[:, 0] > 0)).any() and (scaled[:, 0] == 0).any() and (~on & (scaled[:, 0] < 0)).any()
    floor_cells = len(np.unique(np.floor(scaled), axis=0)); trunc_cells = len(np.unique(np.trunc(scaled), axis=0))
    assert floor_cells == len(pos) and trunc_cells < floor_cells < ncand


def test_ply_bytes(capi, tmp_path):
    c = {x["name"]: x for x in CASES}["pool"]
    pos, nrm, col, _ = expected(c)
    path = tmp_path / "cloud.ply"
    capi.write_ply_points(path, pos, nrm, col)
    data = path.read_bytes()
    assert data == R.ply_bytes(pos, nrm, col)
    assert data.index(b"end_header\n") + 11 + 28 * len(pos) == len(data) and b"element face" not in data
    assert (col[:, 3] == 255).all()
    empty = tmp_path / "empty.ply"
    capi.write_ply_points(empty, pos[:0], nrm[:0], col[:0])
    assert empty.read_bytes() == R.ply_bytes(pos[:0], nrm[:0], col[:0])


def test_cpp_header_saves_the_same_file(built, tmp_path):
    """SiftVisualization::saveToPointCloud of include/bundlefusion/bundlefusion.hpp over host images (plain g++, no device): every second frame of the pool case"""
    import os
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c = {x["name"]: x for x in CASES}["pool"]
    h, w = c["frames"][0][0].shape
    np.concatenate([np.ascontiguousarray(D, np.float32).ravel() for D, _, _ in c["frames"]]).tofile(str(tmp_path / "depth.bin"))
    np.concatenate([np.ascontiguousarray(Cc, np.uint8).ravel() for _, Cc, _ in c["frames"]]).tofile(str(tmp_path / "colour.bin"))
    np.concatenate([np.asarray(T, np.float32).ravel() for _, _, T in c["frames"]] + [np.asarray(c["Kinv"], np.float32).ravel()]).tofile(str(tmp_path / "mats.bin"))
    src = tmp_path / "cloud.cpp"
    src.write_text(r'''
#include "bundlefusion/bundlefusion.hpp"
using namespace bundlefusion;
template <typename T> std::vector<T> slurp(const std::string& p) { std::ifstream f(p, std::ios::binary); std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> r(b.size() / sizeof(T)); memcpy(r.data(), b.data(), r.size() * sizeof(T)); return r; }
int main(int argc, char** argv) {
    const std::string dir = argv[1]; const unsigned w = atoi(argv[2]), h = atoi(argv[3]), n = atoi(argv[4]);
    auto d = slurp<float>(dir + "/depth.bin"); auto c = slurp<unsigned char>(dir + "/colour.bin"); auto m = slurp<float>(dir + "/mats.bin");
    std::vector<const float*> ds; std::vector<const unsigned char*> cs; std::vector<mat4f> T(n); mat4f K;
    for (unsigned i = 0; i < n; ++i) { ds.push_back(d.data() + (size_t)i * w * h); cs.push_back(c.data() + (size_t)i * w * h * 4); memcpy(T[i].m, m.data() + 16 * i, 64); }
    memcpy(K.m, m.data() + 16 * n, 64);
    printf("%u\n", SiftVisualization::saveToPointCloud(dir + "/cpp.ply", ds, cs, T, K, w, h, /*skip=*/2, (unsigned int)-1, 3.5f, 0.0078125f));
    return 0;
}
''')
    lib_dir = os.path.join(root, "bundlefusion_amd", "lib")
    exe = tmp_path / "cloud"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"), str(src), "-L", lib_dir, "-lbf_hip", "-Wl,-rpath," + lib_dir, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path), str(w), str(h), str(len(c["frames"]))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want = R.build(c["frames"][::2], c["Kinv"], c["cell"], c["max_depth"])
    assert int(r.stdout) == len(want[0]) > 0
    assert (tmp_path / "cpp.ply").read_bytes() == R.ply_bytes(*want[:3])


def test_header_declares_what_the_library_exports(built):
    import ctypes as C
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "bf_pointcloud.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"BF_API\s+[\w\s\*]+?\b(bf_\w+)\s*\(", txt)))
    assert len(names) == 11, names
    lib = C.CDLL(os.path.join(root, "bundlefusion_amd", "lib", "libbf_hip.so"))
    assert not [n for n in names if not hasattr(lib, n)]
