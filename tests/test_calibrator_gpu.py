"""GPU tests (-m gpu) of the depth registration (csrc/calibrator.hip): the operator against its numpy restatement (tests/calibrator_ref.py) bit for bit,
its independence of what the scratch plane saw before, the image manager's five ingest forms, and the frame loop with the flag on against a frame loop fed
depth that was registered beforehand."""
import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import default_app_state, default_bundling_state, sensor_desc
from tests import calibrator_cases as cc
from tests import calibrator_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]          # every test under a time limit of its own


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                # a copy: the shared inputs are read-only


def _register_on_device(gpu, depth, Kc, KdInv, E, calibrator=None):
    import torch
    h, w = depth.shape
    c = calibrator or gpu.capi.ImageCalibrator(w, h)
    d = _dev(np.asarray(depth, np.float32))
    c.process(d, Kc, KdInv, E, cc.THRESH_OFFSET, cc.THRESH_LIN)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def _assert_same_bits(got, want, what):
    g, w = got.view(np.uint32), want.view(np.uint32)
    diff = np.argwhere(g != w)
    assert len(diff) == 0, "%s: %d of %d pixels differ, first (y, x) %s: %r vs %r" % (what, len(diff), g.size, diff[0].tolist(), got[tuple(diff[0])], want[tuple(diff[0])])


# ---------------------------------------------------------------------------------------------- 5. operator against restatement
def _case(name):
    if name in ("room_160x120", "room_640x480", "noise_160x120"):
        w, h = (640, 480) if name == "room_640x480" else (160, 120)
        depth = cc.rig_frame(200, w, h)[0]                    # clutter 0.48 m in front of the camera: occlusion, dropped quads, quads leaving the image
        if name == "noise_160x120":
            depth = synth.add_depth_noise(depth)
        return (depth,) + cc.rig_matrices(w, h)
    if name == "focal_x2_160x120":                            # triangles span several pixels
        return (cc.rig_frame(0, 160, 120)[0],) + cc.rig_matrices(160, 120, focal_scale=2.0)        # k = 0: a silhouette inside the narrower view
    if name == "odd_size_131x67":                             # no multiple of the 64x4 tile in either direction
        return (np.ascontiguousarray(cc.rig_frame(200, 160, 120)[0][20:87, 11:142]),) + cc.rig_matrices(160, 120)
    assert name == "identity_160x120"
    K = synth.intrinsics(160, 120)
    return synth.scene_room(200, 160, 120)[0], cc.mat(K), cc.mat_inv(K), np.eye(4, dtype=np.float32)


@pytest.mark.parametrize("name", ["room_160x120", "room_640x480", "focal_x2_160x120", "noise_160x120", "identity_160x120", "odd_size_131x67"])
def test_operator_equals_restatement(gpu, name):
    depth, Kc, KdInv, E = _case(name)
    want = ref.register(depth, Kc, KdInv, E, cc.THRESH_OFFSET, cc.THRESH_LIN)
    got = _register_on_device(gpu, depth, Kc, KdInv, E)
    drawn = np.isfinite(want)
    assert 0.3 < drawn.mean() < 1.0 and np.all(want[~drawn] == -np.inf)          # so that equality says something
    _assert_same_bits(got, want, name)
    if name == "identity_160x120":
        q = ref.quad_survives(depth, cc.THRESH_OFFSET, cc.THRESH_LIN)
        assert np.array_equal(got[q].view(np.uint32), depth[q].view(np.uint32)) and np.all(got[~q] == -np.inf)
    if name == "focal_x2_160x120":                            # more drawn pixels than surviving quads in view: triangles cover several pixels each
        ok, U, V, _ = ref.project_vertices(depth, Kc, KdInv, E)
        inside = ok & (U >= 0) & (U <= 159 * 256) & (V >= 0) & (V <= 119 * 256)
        assert drawn.sum() > 2 * inside.sum()


# ---------------------------------------------------------------------------------------------- 6. order independence
def test_result_does_not_depend_on_the_frames_before(gpu):
    w, h = 160, 120
    Kc, KdInv, E = cc.rig_matrices(w, h)
    a, b = cc.rig_frame(200, w, h)[0], cc.rig_frame(100, w, h)[0]
    c = gpu.capi.ImageCalibrator(w, h)
    first = _register_on_device(gpu, a, Kc, KdInv, E, c)      # scratch plane armed by create
    other = _register_on_device(gpu, b, Kc, KdInv, E, c)
    again = _register_on_device(gpu, a, Kc, KdInv, E, c)      # armed by the frame before
    assert not np.array_equal(first.view(np.uint32), other.view(np.uint32))
    _assert_same_bits(again, first, "second run")
    _assert_same_bits(other, ref.register(b, Kc, KdInv, E, cc.THRESH_OFFSET, cc.THRESH_LIN), "frame after a frame")


# ---------------------------------------------------------------------------------------------- the image manager: five ingest forms
def _params(w, h):
    gas = default_app_state(); gbs = default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = w, h
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = 0.02, 20000, 8000
    gbs.s_widthSIFT, gbs.s_heightSIFT, gbs.s_maxNumImages = w, h, 8
    return gas, gbs


def _rig_sensors(w, h):
    """(the rig, a sensor whose one camera is the rig's colour camera)"""
    Kd, Kc = cc.mat(synth.intrinsics(w, h)), cc.mat(cc.colour_intrinsics(w, h))
    return sensor_desc(w, h, Kd, color_K=Kc, depth_extrinsics=cc.extrinsics()), sensor_desc(w, h, Kc)


def _manager_matrices(gpu, w, h):
    """the three matrices the image manager hands to the operator (CUDAImageManager.cpp:80): its own inverse of the depth intrinsics among them"""
    gas, gbs = _params(w, h)
    rig, _ = _rig_sensors(w, h)
    im = gpu.capi.ImageManager(gas, gbs, rig)
    KdInv = im.depth_intrinsics()[1]                          # integration size == depth size: the sensor's own
    im.close()
    return cc.mat(cc.colour_intrinsics(w, h)), KdInv, cc.extrinsics()


@pytest.mark.parametrize("filters", [(1, 1), (0, 0)])
def test_image_manager_registers_in_all_five_forms(gpu, filters):
    import torch
    from bundlefusion_amd import sensordata as sdm
    w, h = 160, 120
    depth, colour, _, _ = cc.rig_frame(200, w, h)
    u16 = sdm.depth_to_u16(depth, 1000.0)
    rgb = np.ascontiguousarray(colour[:, :, :3])
    rig, plain = _rig_sensors(w, h)
    Kc, KdInv, E = _manager_matrices(gpu, w, h)

    def manager(sensor, on):
        gas, gbs = _params(w, h)
        gbs.s_erodeSIFTdepth, gbs.s_depthFilter = filters
        im = gpu.capi.ImageManager(gas, gbs, sensor)
        assert im.set_camera_calibration(on) == on
        return im

    def state(im):
        return im.get_input_gpu() + im.get_integrate_frame_cpu(0)

    u16_dev, rgb_dev, depth_dev, colour_dev = _dev(u16.view(np.int16)), _dev(rgb), _dev(depth), _dev(colour)      # (int16: the bits of the u16 image); alive to the end
    as_float = torch.empty((h, w), dtype=torch.float32, device="cuda")
    gpu.capi.image_convert_depth_u16(as_float, u16_dev, 1000.0)
    torch.cuda.synchronize()
    want = {}
    for src, name in ((depth, "float"), (as_float.cpu().numpy(), "u16")):
        b = manager(plain, False)
        assert b.process(_register_on_device(gpu, src, Kc, KdInv, E), colour)
        want[name] = state(b)
        assert np.isfinite(want[name][0]).mean() > 0.3
        b.close()
    forms = {
        "process": ("float", lambda im: im.process(depth, colour)),
        "process_device": ("float", lambda im: im.process_device(depth_dev, colour_dev)),
        "process_raw": ("u16", lambda im: im.process_raw(u16, 1000.0, rgb.tobytes(), sdm.COLOR_RAW)),
        "process_raw_decoded": ("u16", lambda im: im.process_raw(u16, 1000.0, rgb)),
        "process_raw_device": ("u16", lambda im: im.process_raw(u16_dev, 1000.0, rgb_dev)),
    }
    for form, (kind, run) in forms.items():
        a = manager(rig, True)
        assert a.camera_calibration() and np.array_equal(a.sift_depth()[2], Kc)
        assert run(a)
        for got, exp, what in zip(state(a), want[kind], ("raw depth", "filtered depth", "colour", "stored depth", "stored colour")):
            assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), form + ": " + what
        a.close()
    # off: the depth camera's intrinsics are reported, and nothing is registered
    off = manager(rig, False)
    assert not off.camera_calibration() and np.array_equal(off.sift_depth()[2], cc.mat(synth.intrinsics(w, h)))
    assert off.process(depth, colour)
    if filters == (0, 0):
        assert np.array_equal(off.get_input_gpu()[0].view(np.uint32), depth.view(np.uint32))
    off.close()


# ---------------------------------------------------------------------------------------------- 7. end to end through the frame loop
W, H, NFRAMES = 320, 240, 21


@pytest.fixture(scope="module")
def rig_stream():
    """21 frames of the displaced-camera stream: [(depth from the depth camera, colour from the colour camera)]"""
    return [cc.rig_frame(k, W, H)[:2] for k in range(NFRAMES)]


def _run_loop(gpu, sensor, flag, feed, n=NFRAMES):
    gas, gbs = _params(W, H)
    gas.s_bUseCameraCalibration = int(flag)
    gp = gpu.capi.Pipeline(gas, gbs, sensor)
    for i in range(n):
        assert feed(gp, i), i
    for _ in range(4):
        gp.process_end_of_sequence()
    gp.synchronize()
    h, heap, cnt, vox = gp.scene().download()
    return dict(active=gp.camera_calibration(), integrated=gp.integrated_trajectory().copy(), optimised=gp.optimized_trajectory().copy(), counters=gp.counters(),
                hash=h, heap=heap, count=cnt, voxels=vox)


def _assert_same_run(got, want, name):
    for t in ("integrated", "optimised"):
        assert np.array_equal(np.isfinite(got[t][:, 0, 0]), np.isfinite(want[t][:, 0, 0])), name + ": validity of the %s poses" % t
        assert np.array_equal(got[t].view(np.uint32), want[t].view(np.uint32)), name + ": %s trajectory" % t
    assert got["counters"] == want["counters"], name
    assert got["count"] == want["count"] and np.array_equal(got["hash"]["pos"], want["hash"]["pos"]) and np.array_equal(got["hash"]["ptr"], want["hash"]["ptr"]), name + ": hash table"
    assert np.array_equal(got["heap"][:got["count"] + 1], want["heap"][:want["count"] + 1]), name + ": heap"
    assert np.array_equal(got["voxels"].view(np.uint8), want["voxels"].view(np.uint8)), name + ": voxel bytes"


@pytest.mark.parametrize("form", ["process_frame", "process_frame_raw"])
def test_frame_loop_registers_like_a_loop_fed_registered_depth(gpu, rig_stream, form):
    """A: flag on, the rig's sensor description, raw displaced depth.  B: flag off, one camera (the rig's colour camera), depth registered beforehand by the
    standalone operator with the matrices the image manager uses.  Poses, their validity, the operator counters, hash table, heap and every voxel byte agree."""
    import torch
    from bundlefusion_amd import sensordata as sdm
    rig, plain = _rig_sensors(W, H)
    Kc, KdInv, E = _manager_matrices(gpu, W, H)
    cal = gpu.capi.ImageCalibrator(W, H)
    colours = [_dev(c) for _, c in rig_stream]
    if form == "process_frame":
        raw = [_dev(d) for d, _ in rig_stream]
        a = _run_loop(gpu, rig, True, lambda gp, i: gp.process_frame(raw[i], colours[i]))
        assert all(np.array_equal(r.cpu().numpy().view(np.uint32), d.view(np.uint32)) for r, (d, _) in zip(raw, rig_stream)), "the caller's depth was written"
    else:
        u16 = [sdm.depth_to_u16(d, 1000.0) for d, _ in rig_stream]
        rgb = [np.ascontiguousarray(c[:, :, :3]) for _, c in rig_stream]
        raw = []
        for u in u16:
            f = torch.empty((H, W), dtype=torch.float32, device="cuda")
            gpu.capi.image_convert_depth_u16(f, _dev(u.view(np.int16)), 1000.0)
            torch.cuda.synchronize()
            raw.append(f)
        a = _run_loop(gpu, rig, True, lambda gp, i: gp.process_frame_raw(u16[i], 1000.0, rgb[i].tobytes(), sdm.COLOR_RAW))
    registered = [cal.process(d.clone(), Kc, KdInv, E, cc.THRESH_OFFSET, cc.THRESH_LIN) for d in raw]
    torch.cuda.synchronize()
    assert not torch.equal(registered[0], raw[0])
    b = _run_loop(gpu, plain, False, lambda gp, i: gp.process_frame(registered[i], colours[i]))
    assert a["active"] and not b["active"]
    # so that equality says something: every frame tracked, both chunks closed and solved, a volume built
    assert len(b["integrated"]) == NFRAMES and np.isfinite(b["integrated"][:, 0, 0]).all(), "frames lost: %s" % np.flatnonzero(~np.isfinite(b["integrated"][:, 0, 0])).tolist()
    assert b["counters"]["integrate"] > 10 and b["counters"]["local_solves"] >= 2 and b["count"] > 500, (b["counters"], b["count"])
    _assert_same_run(a, b, form)


# ---------------------------------------------------------------------------------------------- 8. identity stays off
def test_identity_extrinsics_keep_the_flag_off(gpu, rig_stream):
    K = cc.mat(synth.intrinsics(W, H))
    frames = [(_dev(d), _dev(c)) for d, c in rig_stream[:11]]
    runs = [_run_loop(gpu, sensor_desc(W, H, K), flag, lambda gp, i: gp.process_frame(frames[i][0], frames[i][1]), n=11) for flag in (False, True)]
    assert not runs[0]["active"] and not runs[1]["active"]
    assert np.isfinite(runs[0]["integrated"][:, 0, 0]).all() and runs[0]["count"] > 500
    _assert_same_run(runs[1], runs[0], "flag on, identity extrinsics")
    # the image manager itself: asked for, and still off
    gas, gbs = _params(W, H)
    im = gpu.capi.ImageManager(gas, gbs, sensor_desc(W, H, K))
    assert im.set_camera_calibration(True) is False and np.array_equal(im.sift_depth()[2], K)
    im.close()
