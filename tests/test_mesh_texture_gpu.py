"""GPU tests (-m gpu) of the device mesh texture (csrc/meshtexture.hip) and of the entry points built on it, against the numpy restatement
tests/mesh_texture_ref.py and the one-core route bf_mesh_texture_host.  Bar: atlas bytes, face frames, texture coordinates as uint32 and stats exactly, PLY and PNG
files byte for byte - tolerance 0.

Sizes: k_texture_select takes one face per thread in 64-lane waves and 256-thread workgroups without a loop: 63 / 64 / 65 faces are either side of a wave, 255 / 256 /
257 either side of a workgroup.  k_texture_fill walks the texels in steps of 4096 * 256: the atlas of 4100 x 256 texels (131199 faces in patches of 4) is the
smallest with more than one step (1024 texels more; a texel count is a multiple of 16).  Patch sizes 4 (the least), 5 (odd, and the atlas width no multiple of it), 8
(the default; one cell is one wave of the fill, whose threads walk the texels cell by cell) and 64 (the greatest; one cell is 16 workgroups)."""
import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix, sensor_desc
from tests import mesh_clean_ref
from tests import mesh_recolour_ref as R
from tests import mesh_simplify_ref
from tests import mesh_texture_cases as cases
from tests import mesh_texture_ref as T
from tests import mesh_weld_ref
from tests import test_mesh_weld_gpu as weld_gpu
from tests.test_mesh_texture_cpu import all_cases, host, null_refusals, refusals, sphere_want, tparams, want

pytestmark = pytest.mark.gpu

FILL_STEP = 4096 * 256


@pytest.fixture(scope="module")
def mc(gpu):
    return gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)


class Dev:
    """a case's mesh and frames in device memory (kept alive by this object)"""

    def __init__(self, capi, case):
        import torch
        self.mesh = (torch.from_numpy(np.ascontiguousarray(case["pos"], np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(case["col"], np.float32)).cuda(),
                     torch.from_numpy(np.ascontiguousarray(case["faces"], np.uint32).view(np.int32)).cuda())
        self.images = [(torch.from_numpy(f[0]).cuda(), torch.from_numpy(f[1]).cuda()) for f in case["frames"]]
        self.frames = capi.recolour_frames([(d.data_ptr(), c.data_ptr(), f[2], f[3], f[4]) for (d, c), f in zip(self.images, case["frames"])])


def device(capi, mc, case, dev=None):
    dev = dev or Dev(capi, case)
    return mc.texture(dev.mesh, dev.frames, case["w"], case["h"], case["K"], tparams(case["params"]))


def check(capi, mc, case, w=None):
    err = T.same(device(capi, mc, case), w or want(case))
    assert err is None, (case["name"], err)


@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_texture_planted_families(gpu, mc, family):
    """the face choice (one corner failing each rule in turn, ties, one float apart, the least corner, a skipped frame, degenerate faces), the fill (corners on
    pixels, the gutter out of the image, a black texel, z <= 0, the fallback's bytes), no frames, all skipped, no faces"""
    for case in all_cases():
        if case["family"] == family:
            w = want(case)
            check(gpu.capi, mc, case, w)
            assert T.same(host(case), w) is None


def test_texture_sphere(gpu, mc):
    case, w = sphere_want()
    check(gpu.capi, mc, case, w)
    assert T.same(host(case), w) is None


@pytest.mark.parametrize("nf,S,A", [(1, 8, 64), (2, 8, 64), (3, 8, 64), (15, 8, 64), (16, 8, 64), (17, 8, 64), (16, 8, 70), (11, 4, 16), (9, 5, 64), (777, 5, 203), (5, 64, 200), (63, 8, 256), (64, 8, 256),
                                    (65, 8, 256), (255, 8, 256), (256, 8, 256), (257, 8, 256)])
def test_texture_layout_shapes(gpu, mc, nf, S, A):
    """one, two, three faces; an odd count (the last half cell unused); a row of cells filled exactly (16 faces in 8 cells) and exceeded by one; an atlas width that
    is no multiple of the patch (an unused margin); patches of 4, 5, 8 and 64; face counts either side of a wave and of a workgroup.  The faces are the sphere's
    from its equator on, which the frames see."""
    case, _ = sphere_want()
    case = dict(cases.resized(case, len(case["faces"]) // 2 + nf, patchSize=S, atlasWidth=A))
    case["faces"] = case["faces"][-nf:]
    w = want(case)
    assert w["stats"]["numTexelsFromFrames"] > 0 and (w["stats"]["numTexelsUnused"] > 0) == (nf % 2 == 1 or A % S != 0 or (nf + 1) // 2 % (A // S) != 0)
    check(gpu.capi, mc, case, w)


def test_texture_one_atlas_past_a_step_of_the_texel_loop_then_a_small_one(gpu, mc):
    """131199 faces (the sphere's, repeated) in patches of 4 in an atlas 4100 wide: 4100 x 256 texels, 1024 past one step of the fill's loop, the last half cell and a
    margin of 4 columns unused; then a small atlas on the same object, which the buffers of the large one serve with nothing stale"""
    case, _ = sphere_want()
    large = cases.resized(case, 131199, frames=2, patchSize=4, atlasWidth=4100)
    w = want(large)
    assert FILL_STEP < w["stats"]["atlasWidth"] * w["stats"]["atlasHeight"] <= FILL_STEP + 1024 and len(case["faces"]) % 2 == 0
    check(gpu.capi, mc, large, w)
    live = gpu.capi.debug_live_resources()
    small = cases.resized(case, 257, patchSize=8, atlasWidth=70)
    check(gpu.capi, mc, small)
    assert gpu.capi.debug_live_resources()[:4] == live[:4]          # (the test's own tensors are torch's)


def test_texture_refusals_leave_the_last_result(gpu, mc):
    capi = gpu.capi
    case, w = sphere_want()
    good = cases.resized(case, 300)
    dev = Dev(capi, good)
    w = want(good)
    assert T.same(device(capi, mc, good, dev), w) is None
    st = w["stats"]
    for name, change in refusals():
        bad = dict(good, **change)
        with pytest.raises(capi.BFError, match="status -1"):
            mc.texture(dev.mesh, dev.frames, bad["w"], bad["h"], bad["K"], tparams(bad["params"]))
        got = mc.download_texture(st["atlasWidth"], st["atlasHeight"], st["numFaces"]) + (st,)
        assert T.same(got, w) is None, name
    # the call's pointers: frames NULL with numFrames > 0, a frame that is not skipped with a null image, NULL intrinsics
    pos, col, faces = dev.mesh
    mesh = capi.CleanMesh(pos.data_ptr(), col.data_ptr(), None, faces.data_ptr(), pos.numel() // 3, faces.numel() // 3)
    p = tparams(good["params"])
    for name, frames, n, intr in null_refusals(dev.frames, capi.mat16(good["K"])):
        assert capi.lib.bf_marching_cubes_texture(mc._h, capi.C.byref(mesh), frames, n, good["w"], good["h"], intr, capi.C.byref(p), None) == -1, name
        got = mc.download_texture(st["atlasWidth"], st["atlasHeight"], st["numFaces"]) + (st,)
        assert T.same(got, w) is None, name
    # an atlas higher than 32768 texels: 1025 faces in patches of 64, one cell per row
    with pytest.raises(capi.BFError, match="status -4"):
        mc.texture(Dev(capi, cases.resized(case, 1025)).mesh, dev.frames, good["w"], good["h"], good["K"], tparams(dict(good["params"], patchSize=64, atlasWidth=64)))
    got = mc.download_texture(st["atlasWidth"], st["atlasHeight"], st["numFaces"]) + (st,)
    assert T.same(got, w) is None


def test_texture_without_a_mesh_refuses_a_null_input(gpu):
    m = gpu.capi.MarchingCubesHashSDF(1, 1000, 0.02)
    case = all_cases()[0]
    dev = Dev(gpu.capi, case)
    with pytest.raises(gpu.capi.BFError, match="clean"):
        m.texture(None, dev.frames, case["w"], case["h"], case["K"], tparams(case["params"]))
    m.close()


# --------------------------------------------------------------------------- behind the weld, the clean and the simplify
CELL = 0.05


def _default_params(**more):
    gas = default_app_state()
    return T.params(depthMin=gas.s_sensorDepthMin, depthMax=gas.s_SDFMaxIntegrationDistance, depthTolerance=0.01, depthToleranceLin=0.01, minCos=0.3, **more)


def _files(capi, tmp_path, name, mesh, w):
    """the host route's two files for a mesh (positions, colours, normals or None, faces) and its texture `w`"""
    pos, col, nrm, faces = mesh
    capi.write_ply_textured(tmp_path / (name + ".ply"), name + ".png", pos, nrm, col, faces, w[2])
    capi.write_png_rgba8(tmp_path / (name + ".png"), w[0])
    return (tmp_path / (name + ".ply")).read_bytes(), (tmp_path / (name + ".png")).read_bytes()


def test_texture_behind_the_weld_the_clean_and_the_simplify_on_a_volume(gpu, tmp_path):
    """the three-frame 160 x 120 volume at 2 cm of tests/test_mesh_weld_gpu.py: extract, weld, clean, simplify on a 5 cm grid, texture from those three frames with
    the pipeline's default parameters (patches of 8 in an atlas 512 wide), moved and not.  The device against the restatement and the one-core route; a non-zero
    share of the faces is textured; the two files of bf_marching_cubes_save_mesh_textured, from the extraction, are the host route's byte for byte, with the
    recolouring before the simplification and without"""
    import torch
    capi = gpu.capi
    gs, p = weld_gpu._volume(gpu)
    W, H = 160, 120
    shots = [synth.scene_room(k, W, H) for k in (0, 20, 40)]
    Kd = shots[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    images = [(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda()) for d, c, _, _ in shots]
    m = capi.MarchingCubesHashSDF(600000, p.m_hashNumBuckets, 0.02)
    tris, found = m.extract(gs)
    assert found == len(tris) > 5000
    tp = _default_params(patchSize=8, atlasWidth=512)
    rp = dict(_default_params(), mode=0); del rp["patchSize"], rp["atlasWidth"]
    rparams = capi.MeshRecolourParams(rp["depthMin"], rp["depthMax"], rp["depthTolerance"], rp["depthToleranceLin"], rp["minCos"], 0)
    for transform in (None, mesh_weld_ref.TRANSFORM):
        poses = [Tk if transform is None else R.mul44(transform, Tk) for _, _, Tk, _ in shots]
        frames = [(d, c) + capi.mesh_recolour_frame_from_pose(M) for (d, c, _, _), M in zip(shots, poses)]
        dframes = capi.recolour_frames([(d.data_ptr(), c.data_ptr(), f[2], f[3], f[4]) for (d, c), f in zip(images, frames)])
        cleaned = mesh_clean_ref.clean(*mesh_weld_ref.weld(tris, transform), 41, False, True)
        simple = mesh_simplify_ref.simplify(cleaned[0], cleaned[1], cleaned[3], CELL, True)
        w = T.texture(simple[0], simple[1], simple[3], frames, W, H, K, tp)
        m.weld(None, transform)
        m.clean(None, 41, False, True)
        m.simplify(None, CELL, True)
        got = m.texture(None, dframes, W, H, K, tparams(tp))          # a NULL input: the simplify ran later than the clean
        st = got[3]
        print("textured %d of %d faces (%s): %d texels from frames, %d from vertices, %d unused, atlas %d x %d" % (
            st["numFacesTextured"], st["numFaces"], "moved" if transform is not None else "in place", st["numTexelsFromFrames"], st["numTexelsFromVertices"], st["numTexelsUnused"],
            st["atlasWidth"], st["atlasHeight"]))
        err = T.same(got, w)
        assert err is None, err
        assert st["numFaces"] == len(simple[3]) and 2 * st["numFacesTextured"] > st["numFaces"]
        assert T.same(capi.mesh_texture_host(simple[0], simple[1], simple[3], frames, W, H, K, tparams(tp)), w) is None
        # the files, from the extraction: weld + clean + simplify + texture in one call; no normals asked for, the file has none
        assert m.extract_gpu(gs) == (found, found)
        cst, rst, sst, tst = m.save_mesh_textured(tmp_path / "dev.ply", dframes, W, H, K, tparams(tp), transform, 41, False, False, None, CELL)
        plain = mesh_simplify_ref.simplify(cleaned[0], cleaned[1], cleaned[3], CELL, False)
        assert {k: cst[k] for k in mesh_clean_ref.STAT_KEYS} == cleaned[4] and rst is None and sst == plain[4] and tst == w["stats"]
        ply, png = _files(capi, tmp_path, "host", (plain[0], plain[1], None, plain[3]), capi.mesh_texture_host(plain[0], plain[1], plain[3], frames, W, H, K, tparams(tp)))
        assert (tmp_path / "dev.ply").read_bytes() == ply.replace(b"TextureFile host.png", b"TextureFile dev.png") and (tmp_path / "dev.png").read_bytes() == png
        # recoloured first, with normals, not simplified: the texture of the cleaned mesh with the recolouring's colours
        cst, rst, sst, tst = m.save_mesh_textured(tmp_path / "dev2.ply", dframes, W, H, K, tparams(tp), transform, 41, False, True, rparams, None)
        rc = R.recolour(cleaned[0], cleaned[2], cleaned[1], frames, W, H, K, rp)
        hw = capi.mesh_texture_host(cleaned[0], rc[0], cleaned[3], frames, W, H, K, tparams(tp))
        assert rst == rc[2] and sst is None and tst == hw[3] and tst["numFaces"] == len(cleaned[3])
        ply, png = _files(capi, tmp_path, "host2", (cleaned[0], rc[0], cleaned[2], cleaned[3]), hw)
        assert (tmp_path / "dev2.ply").read_bytes() == ply.replace(b"TextureFile host2.png", b"TextureFile dev2.png") and (tmp_path / "dev2.png").read_bytes() == png
        # one rule for the PNG's name: a dot that begins the base name is no extension
        m.save_mesh_textured(tmp_path / ".dot", dframes, W, H, K, tparams(tp), transform, 41, False, False, None, CELL)
        assert (tmp_path / ".dot").read_bytes() == (tmp_path / "dev.ply").read_bytes().replace(b"TextureFile dev.png", b"TextureFile .dot.png")
        assert (tmp_path / ".dot.png").read_bytes() == (tmp_path / "dev.png").read_bytes()
    m.close()


# --------------------------------------------------------------------------- the frame loop
MIN_FACES = 100
STRIDE = 10


def _pipeline(gpu):
    frames = weld_gpu._stream(25)
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = weld_gpu.PW, weld_gpu.PH
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.02, 50000, 20000
    gbs.s_maxNumImages = 8
    return gpu.capi.Pipeline(gas, gbs, sensor_desc(weld_gpu.PW, weld_gpu.PH, K)), gas, frames


def _run_pipeline(gpu, mesh_dir):
    """the 25-frame configuration of tests/test_mesh_recolour_gpu.py::_run_pipeline; mesh_dir: save the textured, simplified mesh after frame 12 and after the last"""
    import torch
    gp, gas, frames = _pipeline(gpu)
    results = []
    tp = None if mesh_dir is None else gp.mesh_texture_defaults()
    if tp is not None:
        tp.atlasWidth = 1024
    for k, (d, c, _, _) in enumerate(frames):
        assert gp.process_frame(torch.from_numpy(d).cuda(), torch.from_numpy(c).cuda())
        if mesh_dir is not None and k == 12:
            results.append(gp.save_mesh_textured(mesh_dir / "mid.ply", None, MIN_FACES, False, True, tp, STRIDE, False, CELL))
    if mesh_dir is not None:
        results.append(gp.save_mesh_textured(mesh_dir / "final.ply", None, MIN_FACES, False, True, tp, STRIDE, False, CELL))
    gp.synchronize()
    return gp, gas, results


def test_pipeline_save_mesh_textured_leaves_the_reconstruction_alone(gpu, tmp_path):
    """one run saves the textured mesh after frame 12 and after the last frame, the other never: the same trajectories, bf_scene_debug_hash, heap free count,
    allocated blocks and counters; the final files are stand-alone extract -> the restatements' weld, clean and simplify -> the one-core texture (frames and poses:
    the stored frames on the stride under the optimised trajectory) -> bytes"""
    capi = gpu.capi
    plain, _, _ = _run_pipeline(gpu, None)
    a = weld_gpu._volume_state(plain)
    plain.close()
    gp, gas, results = _run_pipeline(gpu, tmp_path)
    b = weld_gpu._volume_state(gp)
    assert np.array_equal(R.bits(a["traj"]), R.bits(b["traj"])) and np.array_equal(R.bits(a["opt"]), R.bits(b["opt"]))
    assert a["dbg"] == b["dbg"] and a["heap_free"] == b["heap_free"] and a["blocks"] == b["blocks"] and a["counters"] == b["counters"]
    d = gp.mesh_texture_defaults()
    rd = gp.mesh_recolour_defaults()
    assert (d.depthMin, d.depthMax, d.depthTolerance, d.depthToleranceLin, d.minCos) == (rd.depthMin, rd.depthMax, rd.depthTolerance, rd.depthToleranceLin, rd.minCos)
    assert (d.patchSize, d.atlasWidth) == (8, 8192)
    d.atlasWidth = 1024
    m = capi.MarchingCubesHashSDF.from_global_app_state(gas, max_triangles=3000000)
    tris, found = m.extract(gp.scene())
    assert found == len(tris) > 5000
    cleaned = mesh_clean_ref.clean(*mesh_weld_ref.weld(tris), MIN_FACES, False, True)
    simple = mesh_simplify_ref.simplify(cleaned[0], cleaned[1], cleaned[3], CELL, True)
    frames, K, W, H = gp.mesh_recolour_frames_host(STRIDE)
    assert len(frames) >= 2
    hw = capi.mesh_texture_host(simple[0], simple[1], simple[3], frames, W, H, K, d)
    cst, rst, sst, tst, nt = results[1]
    print("frame loop: textured %d of %d faces from %d frames, atlas %d x %d" % (tst["numFacesTextured"], tst["numFaces"], tst["numFramesUsed"], tst["atlasWidth"], tst["atlasHeight"]))
    assert nt == found and rst is None and sst == simple[4] and tst == hw[3] and tst["numFacesTextured"] > 0 and tst["numFramesUsed"] == len(frames)
    ply, png = _files(capi, tmp_path, "host", (simple[0], simple[1], simple[2], simple[3]), hw)
    assert (tmp_path / "final.ply").read_bytes() == ply.replace(b"TextureFile host.png", b"TextureFile final.png") and (tmp_path / "final.png").read_bytes() == png
    assert results[0][4] > 0 and (tmp_path / "mid.png").exists() and (tmp_path / "mid.ply").read_bytes() != (tmp_path / "final.ply").read_bytes()
    # recoloured first, moved, not simplified, a file name without an extension: the transform reaches the vertices and the poses alike
    cst, rst, sst, tst, nt = gp.save_mesh_textured(tmp_path / "moved", mesh_weld_ref.TRANSFORM, MIN_FACES, False, False, d, STRIDE, True, None)
    moved = mesh_clean_ref.clean(*mesh_weld_ref.weld(tris, mesh_weld_ref.TRANSFORM), MIN_FACES, False, True)
    mframes = gp.mesh_recolour_frames_host(STRIDE, mesh_weld_ref.TRANSFORM)[0]
    rp = R.params(rd.depthMin, rd.depthMax, rd.depthTolerance, rd.depthToleranceLin, rd.minCos, rd.mode)
    rc = R.recolour(moved[0], moved[2], moved[1], mframes, W, H, K, rp)
    hw = capi.mesh_texture_host(moved[0], rc[0], moved[3], mframes, W, H, K, d)
    assert rst == rc[2] and sst is None and tst == hw[3]
    ply, png = _files(capi, tmp_path, "host_moved", (moved[0], rc[0], None, moved[3]), hw)
    assert (tmp_path / "moved").read_bytes() == ply.replace(b"TextureFile host_moved.png", b"TextureFile moved.png") and (tmp_path / "moved.png").read_bytes() == png
    c = weld_gpu._volume_state(gp)
    assert c["dbg"] == b["dbg"] and c["heap_free"] == b["heap_free"] and c["blocks"] == b["blocks"]
    m.close()
    gp.close()


def test_pipeline_save_mesh_textured_refuses_a_sharded_volume(gpu, tmp_path):
    gp, _, _ = _pipeline(gpu)
    gp.set_volume_shard(0, 2)
    with pytest.raises(Exception, match="shard"):
        gp.save_mesh_textured(tmp_path / "shard.ply", None, MIN_FACES, False, True, None, STRIDE)
    assert not (tmp_path / "shard.ply").exists() and not (tmp_path / "shard.png").exists()
    gp.close()
