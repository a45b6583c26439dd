"""CPU tests of the mesh texture's definition: the numpy restatement (tests/mesh_texture_ref.py) and the library's one-core route (bf_mesh_texture_host) agree - atlas
bytes, face frames, texture coordinates as bits, stats - on every planted case (tests/mesh_texture_cases.py) and on the sphere; the planted cases test what they are
named for; the layout's properties are proved by enumeration for every patch size; bf_write_ply_textured is held to a python writer.  No GPU is needed."""
import functools

import numpy as np
import pytest

from bundlefusion_amd import capi
from tests import mesh_recolour_ref as R
from tests import mesh_texture_cases as cases
from tests import mesh_texture_ref as T

F = np.float32


def tparams(p):
    return capi.MeshTextureParams(float(p["depthMin"]), float(p["depthMax"]), float(p["depthTolerance"]), float(p["depthToleranceLin"]), float(p["minCos"]), int(p["patchSize"]),
                                  int(p["atlasWidth"]))


def want(case):
    return T.texture(case["pos"], case["col"], case["faces"], case["frames"], case["w"], case["h"], case["K"], case["params"])


def host(case):
    return capi.mesh_texture_host(case["pos"], case["col"], case["faces"], case["frames"], case["w"], case["h"], case["K"], tparams(case["params"]))


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(cases.all_cases())


@functools.lru_cache(maxsize=None)
def sphere_want():
    """the sphere and its restatement, computed once and shared (never written to)"""
    case = cases.sphere_case()
    return case, want(case)


def case_named(name):
    return next(c for c in all_cases() if c["name"] == name)


CASE_NAMES = [c["name"] for c in all_cases()]


def test_library_exports_every_new_symbol():
    for name in ("bf_marching_cubes_texture", "bf_marching_cubes_download_texture", "bf_marching_cubes_save_mesh_textured", "bf_mesh_texture_host", "bf_mesh_texture_atlas_height",
                 "bf_write_ply_textured", "bf_pipeline_save_mesh_textured", "bf_pipeline_get_mesh_texture_defaults"):
        assert hasattr(capi.lib, name), name


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_and_host_route_agree_on_planted_cases(name):
    case = case_named(name)
    a = want(case)
    err = T.same(host(case), a)
    assert err is None, err
    st, e = a["stats"], case["expect"]
    assert st["numFacesTextured"] + st["numFacesUntextured"] == st["numFaces"] == len(case["faces"])
    assert st["numTexelsFromFrames"] + st["numTexelsFromVertices"] + st["numTexelsUnused"] == st["atlasWidth"] * st["atlasHeight"]
    assert st["numFramesUsed"] + st["numFramesSkipped"] == len(case["frames"])
    if "face_frame" in e:
        assert a["faceFrame"].tolist() == e["face_frame"]
    if "rule" in e:
        # faces 0 1 2: exactly the named corner fails, with the named rule, and the face is not textured; face 3, the control, is
        for f, corner in enumerate(e["failing"]):
            codes = a["codes"][f, :, 0].tolist()
            assert codes[corner] == e["rule"] and all(c == R.VIEW for k, c in enumerate(codes) if k != corner), (name, f, codes)
        assert a["faceFrame"].tolist() == [-1, -1, -1, 0]
    if "equal" in e:
        w = np.fmin(np.fmin(a["weights"][0, 0], a["weights"][0, 1]), a["weights"][0, 2])
        assert T.bits(w[e["equal"][0]]) == T.bits(w[e["equal"][1]])
    if "ulp" in e:
        w = np.fmin(np.fmin(a["weights"][0, 0], a["weights"][0, 1]), a["weights"][0, 2])
        greater, less = e["ulp"]
        assert int(T.bits(w)[greater]) - int(T.bits(w)[less]) == 1
    if "least_in_frame0" in e:
        w = a["weights"]
        assert np.argmin(w[:, :, 0], axis=1).tolist() == e["least_in_frame0"]
        assert (w[:, :, 1].min(1) > w[:, :, 0].min(1)).all() and (w[:, :, 0].max(1) > w[:, :, 1].max(1)).all()          # the greatest corner alone would keep frame 0
    if "skipped" in e:
        assert [int(f[4]) for f in case["frames"]] == e["skipped"] and (a["codes"][:, :, np.array(e["skipped"], bool)] == R.SKIPPED).all()
    if "why" in e:
        present = set(np.unique(a["why"]).tolist()) - {T.WHY_UNUSED}
        assert present == set(e["why"]), (name, present)
    if "why_index" in e:
        S, A = case["params"]["patchSize"], case["params"]["atlasWidth"]
        for f in e["why_index"]:
            x, y = (f >> 1) * S + (S - 1 if f & 1 else 0), (S - 1 if f & 1 else 0)
            assert a["why"][y, x] == T.WHY_INDEX and a["atlas"][y, x].tolist() == [0, 0, 0, 255]
    if "bytes_seen" in e:
        seen = set(np.unique(a["atlas"][a["why"] == T.WHY_NO_FRAME][:, :3]).tolist())
        assert set(e["bytes_seen"]) <= seen


def test_meaning_corner_texels_carry_their_vertices_pixels():
    """both faces of the cell are seen by the one frame and every corner projects onto a pixel centre: the corner texels, found through the texture coordinates the
    library returns, carry those pixels' bytes.  Stated from the frame, not from the restatement."""
    case = case_named("fill_corners_on_pixels")
    atlas, ff, uv, st = host(case)
    C = case["frames"][0][1]
    H, A = atlas.shape[:2]
    for f, pixels in enumerate(case["expect"]["corner_pixels"]):
        for corner, (px, py) in enumerate(pixels):
            x = int(uv[f, 2 * corner] * A); y = int((1.0 - uv[f, 2 * corner + 1]) * H)
            assert atlas[y, x].tolist() == C[py, px, :3].tolist() + [255], (f, corner)
    assert ff.tolist() == [0, 0] and st["numTexelsUnused"] == (A - 8) * H


def library_layout(S):
    """the layout the library ships for patches of S, read off bf_mesh_texture_host itself: four faces (two cells) in an atlas of two cells and one margin
    column, no frame, face f with the constant vertex colour LAYOUT_COLOURS[f] - a texel's bytes then name the face that owns it (the weights of a texel sum to 1
    within a few floats, so a channel is 0 or at least 254), and the texture coordinates name the corner texels.  Returns (owner [S, 2 S + 1] int: the face, -1
    unused; corner texels [4, 3, 2] int as (x, y))"""
    pos = np.zeros((12, 3), F)
    col = np.repeat(np.array(LAYOUT_COLOURS, F), 3, axis=0)
    faces = np.arange(12, dtype=np.uint32).reshape(4, 3)
    A = 2 * S + 1
    atlas, ff, uv, st = capi.mesh_texture_host(pos, col, faces, [], 8, 6, np.eye(4, dtype=F), tparams(T.params(patchSize=S, atlasWidth=A)))
    assert atlas.shape == (S, A, 4) and (ff == -1).all() and st["numTexelsFromFrames"] == 0
    owner = np.full((S, A), -2, np.int64)
    owner[(atlas == 0).all(2)] = -1
    for f, c in enumerate(LAYOUT_COLOURS):
        mine = (atlas[:, :, 3] == 255) & ((atlas[:, :, :3] >= 254) == (np.array(c) == 1)).all(2) & ((atlas[:, :, :3] == 0) == (np.array(c) == 0)).all(2)
        owner[mine] = f
    assert (owner >= -1).all() and st["numTexelsUnused"] == (owner == -1).sum() and st["numTexelsFromVertices"] == (owner >= 0).sum()
    x = uv[:, 0::2].astype(np.float64) * A - 0.5; y = (1.0 - uv[:, 1::2].astype(np.float64)) * S - 0.5
    cx, cy = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
    assert np.abs(x - cx).max() < 1e-3 and np.abs(y - cy).max() < 1e-3          # a texture coordinate is a texel centre
    return owner, np.stack([cx, cy], 2)


LAYOUT_COLOURS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)]


@pytest.mark.parametrize("S", range(4, 65))
def test_layout_ownership_is_a_partition_and_the_bilinear_footprint_stays_with_the_owner(S):
    """On the layout read off the library (library_layout), for every patch size: every texel of a cell has exactly one owner, the diagonal i + j == S - 1 going to
    half 0, the margin column is unused, and ownership and corner texels are the restatement's.  A bilinear lookup at a point (x, y) of a face's triangle (corner
    texel centres a, b, c, from the library's texture coordinates) reads with a weight above zero the texels i with |x - i| < 1 and j with |y - j| < 1, and all of
    them lie inside the cell and belong to that face - by enumeration of the triangle's points on a grid of quarter texels along its two edges from a, which has
    every integer point and points in every unit square.  Half 0 never reaches the diagonal (it reads i + j <= S - 2), half 1 reads i + j >= S: both have a
    gutter."""
    owner, corner = library_layout(S)
    m = S - 3
    assert (owner[:, 2 * S] == -1).all()
    for cell in (0, 1):
        own = owner[:, cell * S:(cell + 1) * S] - 2 * cell
        assert set(np.unique(own).tolist()) == {0, 1} and np.array_equal(own, T.owner(S))
        assert own.sum() == S * (S - 1) // 2 and ((own[::-1, ::-1] == 1) <= (own == 0)).all()          # half 1 turned by 180 degrees is half 0 without the diagonal
        j, i = np.mgrid[0:S, 0:S]
        assert (own[i + j == S - 1] == 0).all()
        local = corner[2 * cell:2 * cell + 2] - np.array([cell * S, 0])
        assert np.array_equal(local, T.corners(S))
        assert local[0].tolist() == [[0, 0], [m, 0], [0, m]] and local[1].tolist() == [[S - 1, S - 1], [S - 1 - m, S - 1], [S - 1, S - 1 - m]]
        steps = np.arange(0, 4 * m + 1) / 4.0          # (quarters: exact)
        s, r = np.meshgrid(steps, steps)
        inside = s + r <= m
        s, r = s[inside], r[inside]
        for half in (0, 1):
            a, b, c = local[half].astype(np.float64)
            assert np.abs(b - a).sum() == m and np.abs(c - a).sum() == m          # the two edges from a are m texels long, along the axes
            px = a[0] + s * ((b[0] - a[0]) / m) + r * ((c[0] - a[0]) / m); py = a[1] + s * ((b[1] - a[1]) / m) + r * ((c[1] - a[1]) / m)
            assert px.min() == min(a[0], b[0]) and px.max() == max(a[0], b[0]) and py.min() == min(a[1], c[1]) and py.max() == max(a[1], c[1])
            reach = []
            for ti in (np.floor(px).astype(int), np.ceil(px).astype(int)):
                for tj in (np.floor(py).astype(int), np.ceil(py).astype(int)):
                    assert (ti >= 0).all() and (ti < S).all() and (tj >= 0).all() and (tj < S).all() and (own[tj, ti] == half).all()
                    reach.append(ti + tj)
            assert (np.max(reach) == S - 2) if half == 0 else (np.min(reach) == S)


@pytest.mark.parametrize("nf,S,A", [(1, 8, 64), (2, 4, 4), (3, 5, 64), (17, 8, 64), (16, 8, 70), (257, 64, 16384), (1001, 7, 100)])
def test_texture_coordinates_as_bits(nf, S, A):
    pos = np.zeros((1, 3), F); faces = np.zeros((nf, 3), np.uint32)
    p = T.params(patchSize=S, atlasWidth=A)
    atlas, ff, uv, st = capi.mesh_texture_host(pos, pos, faces, [], 8, 6, np.eye(4, dtype=F), tparams(p))
    m, cpr, H = T.layout(nf, S, A)
    assert (st["atlasWidth"], st["atlasHeight"]) == (A, H) == atlas.shape[1::-1] and capi.mesh_texture_atlas_height(nf, tparams(p)) == H
    assert np.array_equal(T.bits(uv), T.bits(T.face_uv(nf, S, A)))
    # by hand: corner a of face 0 is texel (0, 0), corner a of face 1 texel (S - 1, S - 1)
    assert uv[0, 0] == F(0.5) / F(A) and uv[0, 1] == F(1) - F(0.5) / F(H)
    if nf > 1:
        assert uv[1, 0] == (F(S - 1) + F(0.5)) / F(A) and uv[1, 1] == F(1) - (F(S - 1) + F(0.5)) / F(H)
    assert (uv > 0).all() and (uv < 1).all()


def test_sphere():
    """about 2000 faces and 3 frames of 64 x 48: a condition on the input, met by the restatement alone - faces are textured and untextured, every rule code occurs
    among the corners, texels come from frames and from every kind of fallback but z - and the host route agrees with the restatement"""
    case, a = sphere_want()
    st = a["stats"]
    assert 1500 < st["numFaces"] < 2500 and 4 * st["numFacesTextured"] > st["numFaces"] and st["numFacesUntextured"] > 0
    for code in (R.VIEW, R.NORMAL, R.RANGE, R.IMAGE, R.FACING, R.OCCLUDED, R.COLOUR):
        assert (a["codes"] == code).any(), "rule code %d does not occur" % code
    for why in (T.WHY_FRAME, T.WHY_NO_FRAME, T.WHY_IMAGE, T.WHY_BLACK, T.WHY_INDEX):
        assert (a["why"] == why).any(), "no texel of kind %d" % why
    assert len(set(a["faceFrame"].tolist())) == cases.SPHERE_FRAMES + 1
    err = T.same(host(case), a)
    assert err is None, err


def test_zero_frames_give_the_interpolated_vertex_colours():
    case, _ = sphere_want()
    none = want(dict(case, frames=[]))
    skipped = want(dict(case, frames=[f[:4] + (True,) for f in case["frames"]]))
    assert (none["faceFrame"] == -1).all() and none["stats"]["numTexelsFromFrames"] == 0 and np.array_equal(none["atlas"], skipped["atlas"])
    assert T.same(host(dict(case, frames=[])), none) is None


def refusals():
    """(name, keyword changes) of every refusal of the definition"""
    p = T.params()
    return [("width_1", dict(w=1)), ("height_1", dict(h=1)), ("nan_parameter", dict(params=dict(p, depthTolerance=float("nan")))),
            ("inf_parameter", dict(params=dict(p, depthMax=float("inf")))), ("depth_min_zero", dict(params=dict(p, depthMin=0.0))),
            ("depth_max_below_min", dict(params=dict(p, depthMin=2.0, depthMax=1.0))), ("negative_tolerance", dict(params=dict(p, depthTolerance=-0.5))),
            ("negative_linear_tolerance", dict(params=dict(p, depthToleranceLin=-0.5))), ("min_cos_zero", dict(params=dict(p, minCos=0.0))),
            ("min_cos_above_one", dict(params=dict(p, minCos=1.5))), ("patch_3", dict(params=dict(p, patchSize=3))), ("patch_65", dict(params=dict(p, patchSize=65))),
            ("atlas_narrower_than_a_patch", dict(params=dict(p, atlasWidth=7))), ("atlas_16385", dict(params=dict(p, atlasWidth=16385)))]


@pytest.mark.parametrize("name,change", refusals(), ids=[r[0] for r in refusals()])
def test_host_route_refuses(name, change):
    case = dict(case_named("weight_tie"), **change)
    frames = case["frames"] if case["w"] == 8 and case["h"] == 6 else []          # (the images no longer fit the size: the size is refused before they are read)
    with pytest.raises(capi.BFError, match="status -1"):
        capi.mesh_texture_host(case["pos"], case["col"], case["faces"], frames, case["w"], case["h"], case["K"], tparams(case["params"]))


def null_refusals(frames, K):
    """(name, frames, numFrames, intrinsics) of the refusals that are about the call's pointers, not its values: `frames` is a recolour_frames() table of at least
    two frames that are not skipped, K the intrinsics as mat16"""
    holed = type(frames)(*frames)
    holed[1].d_colorRGBX = None
    depthless = type(frames)(*frames)
    depthless[0].d_depth = None
    return [("null_frames", None, len(frames), K), ("null_colour_image", holed, len(frames), K), ("null_depth_image", depthless, len(frames), K),
            ("null_intrinsics", frames, len(frames), None)]


def test_host_route_refuses_null_frames_null_images_and_null_intrinsics():
    """the rest of the recolouring's list: frames NULL with numFrames > 0, a frame that is not skipped with a null image, NULL intrinsics; a skipped frame's null
    images are no error"""
    case = case_named("weight_tie")
    pos, col, faces = case["pos"], case["col"], case["faces"]
    keep = [(np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1])) for f in case["frames"]]
    table = capi.recolour_frames([(d.ctypes.data, c.ctypes.data, f[2], f[3], f[4]) for (d, c), f in zip(keep, case["frames"])])
    p = tparams(case["params"])

    def call(frames, n, K):
        return capi.lib.bf_mesh_texture_host(pos.ctypes.data_as(capi.C.c_void_p), col.ctypes.data_as(capi.C.c_void_p), faces.ctypes.data_as(capi.C.c_void_p), len(pos), len(faces), frames, n,
                                             case["w"], case["h"], K, capi.C.byref(p), None, None, None, None)

    K = capi.mat16(case["K"])
    assert call(table, len(table), K) == 0
    for name, frames, n, intr in null_refusals(table, K):
        assert call(frames, n, intr) == -1, name
    skipped = type(table)(*table)
    skipped[1].d_depth = None; skipped[1].d_colorRGBX = None; skipped[1].skipped = 1
    assert call(skipped, len(skipped), K) == 0 and call(None, 0, K) == 0


def test_an_atlas_higher_than_32768_is_a_capacity_error():
    """S = 64 in an atlas one cell wide: 1024 faces are 512 cells, H = 32768, legal; 1025 faces need 513"""
    p = tparams(T.params(patchSize=64, atlasWidth=64))
    assert capi.mesh_texture_atlas_height(1024, p) == 32768
    with pytest.raises(capi.BFError, match="status -4"):
        capi.mesh_texture_atlas_height(1025, p)
    st = capi.MeshTextureStats()
    rc = capi.lib.bf_mesh_texture_host(None, None, np.zeros((1025, 3), np.uint32).ctypes.data_as(capi.C.c_void_p), 0, 1025, None, 0, 8, 6, capi.mat16(np.eye(4, dtype=F)), capi.C.byref(p), None,
                                       None, None, capi.C.byref(st))
    assert rc == -4


def test_ply_of_a_textured_mesh_is_the_python_writers(tmp_path):
    case, a = sphere_want()
    pos = np.nan_to_num(case["pos"])
    nrm = np.random.default_rng(3).normal(size=pos.shape).astype(F)
    for name, normals in (("plain.ply", None), ("normals.ply", nrm)):
        capi.write_ply_textured(tmp_path / name, "atlas of it.png", pos, normals, case["col"], case["faces"], a["faceUV"])
        assert (tmp_path / name).read_bytes() == T.ply_bytes("atlas of it.png", pos, normals, case["col"], case["faces"], a["faceUV"])
    head = (tmp_path / "plain.ply").read_bytes().split(b"end_header\n")[0].decode().split("\n")
    assert head[2:4] == ["comment bundlefusion_amd marching cubes", "comment TextureFile atlas of it.png"]
    assert head[-3:-1] == ["property list uchar int vertex_indices", "property list uchar float texcoord"]
    capi.write_ply_textured(tmp_path / "empty.ply", "none.png", np.zeros((0, 3), F), None, np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), np.zeros((0, 6), F))
    assert (tmp_path / "empty.ply").read_bytes() == T.ply_bytes("none.png", np.zeros((0, 3), F), None, np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), np.zeros((0, 6), F))
    with pytest.raises(capi.BFError):
        capi.write_ply_textured(tmp_path / "bad.ply", "a\nb.png", pos, None, case["col"], case["faces"], a["faceUV"])
