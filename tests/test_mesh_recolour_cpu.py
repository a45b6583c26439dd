"""CPU tests of the mesh recolouring's definition: the two numpy restatements (tests/mesh_recolour_ref.py) and the library's one-core route
(bf_mesh_recolour_host) agree as bits - colours, view counts, stats and the rule code of every pair - on every planted case (tests/mesh_recolour_cases.py) and on
the random sphere; the planted cases test what they are named for; the meaning of a colour is stated by hand.  No GPU is needed."""
import functools

import numpy as np
import pytest

from bundlefusion_amd import capi
from tests import mesh_recolour_cases as cases
from tests import mesh_recolour_ref as R

F = np.float32
MODES = (0, 1)


def rparams(p, mode=None):
    return capi.MeshRecolourParams(float(p["depthMin"]), float(p["depthMax"]), float(p["depthTolerance"]), float(p["depthToleranceLin"]), float(p["minCos"]),
                                   int(p["mode"] if mode is None else mode))


def with_mode(case, mode):
    return dict(case, params=dict(case["params"], mode=mode))


def want(case, loop=False):
    f = R.recolour_loop if loop else R.recolour
    return f(case["pos"], case["nrm"], case["col"], case["frames"], case["w"], case["h"], case["K"], case["params"])


def host(case):
    return capi.mesh_recolour_host(case["pos"], case["nrm"], case["col"], case["frames"], case["w"], case["h"], case["K"], rparams(case["params"]), codes=True)


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(cases.all_cases())


@functools.lru_cache(maxsize=None)
def random_want(mode):
    """the random case and its restatement, computed once per mode and shared (never written to)"""
    case = with_mode(cases.random_case(), mode)
    return case, want(case)


CASE_NAMES = [c["name"] for c in cases.all_cases()]


def case_named(name):
    return next(c for c in all_cases() if c["name"] == name)


def test_library_exports_every_new_symbol():
    for name in ("bf_mesh_recolour_frame_from_pose", "bf_marching_cubes_recolour", "bf_marching_cubes_recolour_views", "bf_marching_cubes_download_recoloured",
                 "bf_marching_cubes_save_mesh_recoloured", "bf_mesh_recolour_host", "bf_pipeline_save_mesh_recoloured", "bf_pipeline_get_mesh_recolour_defaults"):
        assert hasattr(capi.lib, name), name


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatements_and_host_route_agree_on_planted_cases(name, mode):
    case = with_mode(case_named(name), mode)
    a, b, c = want(case), want(case, loop=True), host(case)
    assert R.same(b, a) is None, R.same(b, a)
    assert R.same(c, a) is None, R.same(c, a)
    st = a[2]
    assert st["numRecoloured"] + st["numUnseen"] == st["numVertices"] == len(case["pos"]) and st["numFramesUsed"] + st["numFramesSkipped"] == len(case["frames"])
    for code in case["codes"]:
        assert (a[3] == code).any(), (name, "rule code %d does not occur" % code)
    e = case["expect"] or {}
    if "views" in e:
        assert a[1].tolist() == e["views"]
    if "frame_views" in e:
        assert (a[3][0] == R.VIEW).astype(int).tolist() == e["frame_views"]
    if "first_codes" in e:
        assert a[3][:, 0].tolist() == e["first_codes"]
    if "skipped" in e:
        assert [int(f[4]) for f in case["frames"]] == e["skipped"] and (a[3][:, np.array(e["skipped"], bool)] == R.SKIPPED).all()
    # positions with no view keep their colour bit for bit
    unseen = a[1] == 0
    assert np.array_equal(R.bits(a[0][unseen]), R.bits(case["col"][unseen]))


def test_the_order_of_the_frames_is_under_test():
    """permuting the frames of the weights case changes the bits of the blend, on the restatement alone"""
    case = with_mode(case_named("order_weights"), 0)
    a = want(case)
    assert (a[1] == len(case["frames"])).all()
    changed = False
    for perm in ([1, 0, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1]):
        b = want(dict(case, frames=[case["frames"][k] for k in perm]))
        assert np.array_equal(b[1], a[1])
        changed = changed or not np.array_equal(R.bits(b[0]), R.bits(a[0]))
        assert np.allclose(b[0], a[0], rtol=1e-5, atol=0)
    assert changed


@pytest.mark.parametrize("name", ["order_tie", "order_nearer_wins"])
def test_best_view_takes_the_greatest_weight_and_ties_keep_the_earlier_frame(name):
    case = with_mode(case_named(name), 1)
    a = want(case)
    best = case["expect"]["best"]
    alone = want(dict(case, frames=[case["frames"][best]]))
    assert (a[1] == len(case["frames"])).all() and np.array_equal(R.bits(a[0]), R.bits(alone[0]))
    if name == "order_tie":
        other = want(dict(case, frames=[case["frames"][1]]))
        assert not np.array_equal(R.bits(a[0]), R.bits(other[0]))


@pytest.mark.parametrize("mode", MODES)
def test_meaning_a_vertex_on_a_pixel_centre_gets_that_pixel(mode):
    """the vertex projects exactly onto pixel (5, 1) of the only frame, whose bytes are (200, 100, 50): the expected colour is written out here, not taken from
    the restatement"""
    case = with_mode(cases.meaning_case(), mode)
    expected = np.array([F(200) / F(255), F(100) / F(255), F(50) / F(255)], F)
    for got in (want(case), want(case, loop=True), host(case)):
        assert got[1].tolist() == [1] and np.array_equal(R.bits(got[0][0]), R.bits(expected))


def test_frame_from_pose_is_the_cofactor_inverse_and_the_translation():
    M = cases.pose(tx=1.0, ty=2.0, tz=-1.0, rot=cases.ROT_Z90)
    W, o, skipped = capi.mesh_recolour_frame_from_pose(M)
    assert not skipped and o.tolist() == [1.0, 2.0, -1.0]
    assert np.array_equal(W, np.linalg.inv(M.astype(np.float64)).astype(F))          # exact for a signed permutation and small integers


@pytest.mark.parametrize("mode", MODES)
def test_random_sphere(mode):
    """about 5 000 vertices and 7 frames of 64 x 48: every rule code occurs and at least a quarter of the pairs are views (a condition on the input, met by the
    restatement alone); the loop restatement and the host route agree with the vectorised one as bits"""
    case, a = random_want(mode)
    codes = a[3]
    for code in range(7):
        assert (codes == code).any(), "rule code %d does not occur" % code
    assert (codes == R.VIEW).mean() >= 0.25, (codes == R.VIEW).mean()
    assert a[2]["maxViews"] >= 3 and 0 < a[2]["numUnseen"] < a[2]["numVertices"]
    assert R.same(host(case), a) is None
    assert R.same(want(case, loop=True), a) is None


def refusals():
    """(name, keyword changes) of every refusal of the definition"""
    p = R.params()
    return [("null_normals", dict(nrm=None)), ("width_1", dict(w=1)), ("height_1", dict(h=1)),
            ("nan_parameter", dict(params=dict(p, depthTolerance=float("nan")))), ("inf_parameter", dict(params=dict(p, depthMax=float("inf")))),
            ("depth_min_zero", dict(params=dict(p, depthMin=0.0))), ("depth_max_below_min", dict(params=dict(p, depthMin=2.0, depthMax=1.0))),
            ("negative_tolerance", dict(params=dict(p, depthTolerance=-0.5))), ("negative_linear_tolerance", dict(params=dict(p, depthToleranceLin=-0.5))),
            ("min_cos_zero", dict(params=dict(p, minCos=0.0))), ("min_cos_above_one", dict(params=dict(p, minCos=1.5))), ("mode_2", dict(params=dict(p, mode=2))),
            ("mode_negative", dict(params=dict(p, mode=-1)))]


@pytest.mark.parametrize("name,change", refusals(), ids=[r[0] for r in refusals()])
def test_host_route_refuses(name, change):
    case = dict(cases.meaning_case(), **change)
    frames = case["frames"] if case["w"] == 8 and case["h"] == 6 else []          # (the images no longer fit the size: the size is refused before they are read)
    with pytest.raises(capi.BFError):
        capi.mesh_recolour_host(case["pos"], case["nrm"], case["col"], frames, case["w"], case["h"], case["K"], rparams(case["params"]))


def test_ply_of_the_host_route_is_the_restatements(tmp_path):
    """the one-core route's file - bf_mesh_recolour_host's colours through bf_write_ply_indexed_normals - against the restatement's bytes"""
    case, a = random_want(0)
    n = len(case["pos"])
    faces = np.stack([np.arange(0, n - 2), np.arange(1, n - 1), np.arange(2, n)], 1).astype(np.uint32)[::3]
    pos = np.nan_to_num(case["pos"])
    got = host(case)
    capi.write_ply_indexed_normals(tmp_path / "host.ply", pos, case["nrm"], got[0], faces)
    assert (tmp_path / "host.ply").read_bytes() == R.ply_bytes(pos, case["nrm"], a[0], faces)
