"""GPU tests (-m gpu) of the recording (csrc/sensorrecord.hip, bf_sens_recorder_record_device, bf_pipeline_set_record_state / _save_recording): the two
packing kernels against the host (numpy's float32 restatement of the depth rule, bf_jpeg_forward_host), the recorder fed from device buffers against
the host route's file, and the frame loop with a record state against the loop without one.

Tolerance: none.  The depth rule is one float32 multiplication, one addition and a truncation; the encoder's forward stage is binary32 arithmetic in a
defined order shared by host and device (csrc/bf_jpeg_fwd.h): every result is compared as BYTES, device outputs behind a sentinel pattern with a guard tail.
"""
import os
import sys

import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import default_app_state, default_bundling_state, default_record_state, intrinsics_matrix, sensor_desc
from tests import record_cases as rc
from tests.sensor_ingest_streams import image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_BYTES = 4096
LENGTHS = (1, 63, 64, 65, 640 * 480 + 1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Out:
    """A device output pre-filled with sentinel bytes and followed by a guard tail of sentinel bytes (tests/test_sensor_ingest_gpu.py)."""

    def __init__(self, nbytes, seed=0):
        import torch
        self.n = int(nbytes)
        self.init = np.random.default_rng(seed).integers(0, 256, self.n + GUARD_BYTES, dtype=np.uint8)
        self.buf = torch.from_numpy(self.init.copy()).cuda()
        self.t = self.buf[:self.n]

    def check(self, expected, what):
        import torch
        torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        assert np.array_equal(got[self.n:], self.init[self.n:]), what + ": guard tail written"
        exp = np.ascontiguousarray(expected).view(np.uint8).reshape(-1)
        assert exp.size == self.n, what
        bad = np.flatnonzero(got[:self.n] != exp)
        assert bad.size == 0, "%s: %d of %d bytes differ, first at byte %d" % (what, bad.size, self.n, bad[0])


@pytest.fixture(scope="module")
def sdm(gpu):
    from bundlefusion_amd import sensordata
    return sensordata


# ------------------------------------------------------------------------------------------------ 6: depth packing
SPECIAL = np.array([-np.inf, np.inf, np.nan, 0.0, -0.0, -1.0, -1e-30, -65.0, 1e-7, 65.5354, 65.5355, 65.536, 1e9], np.float32)


@pytest.mark.parametrize("shift", [1000.0, 5000.0, 999.5])
def test_depth_packing_every_u16_value_and_the_special_ones(gpu, sdm, shift):
    """every u16 / 1000 value plus the invalid and the boundary ones; expected: the rule in numpy float32 operations in the same order"""
    with np.errstate(divide="ignore"):
        d = np.concatenate([(np.arange(65536, dtype=np.uint16).astype(np.float32) / np.float32(1000.0)).astype(np.float32), SPECIAL])
    want = sdm.record_depth_rule(d, shift)
    if shift == 1000.0:
        assert np.array_equal(want[:65536], np.arange(65536, dtype=np.uint16)) and not want[65536:65544].any()
    o = _Out(d.size * 2, seed=1)
    gpu.capi.image_convert_depth_to_u16(o.t, _dev(d), shift)
    o.check(want, "depth shift %g" % shift)


@pytest.mark.parametrize("n", LENGTHS)
def test_depth_packing_lengths(gpu, sdm, n):
    rng = np.random.default_rng(n)
    d = (rng.random(n, dtype=np.float32) * np.float32(70.0) - np.float32(2.0)).astype(np.float32)
    d[rng.integers(0, n, min(n, 13))] = SPECIAL[:min(n, 13)]
    d[-1] = np.float32(65.5354)
    for shift in (1000.0, 999.5):
        want = sdm.record_depth_rule(d, shift)
        o = _Out(n * 2, seed=2)
        gpu.capi.image_convert_depth_to_u16(o.t, _dev(d), shift)
        o.check(want, "depth n=%d shift %g" % (n, shift))
    if n > 8:                                                   # buffers that are not 16-byte aligned take the pixel-by-pixel path
        src = _dev(np.concatenate([np.zeros(1, np.float32), d]))[1:]
        o = _Out(n * 2 + 2, seed=3)
        gpu.capi.image_convert_depth_to_u16(o.t[2:], src, 1000.0)
        o.check(np.concatenate([o.init[:2], sdm.record_depth_rule(d, 1000.0).view(np.uint8)]), "depth n=%d, unaligned" % n)


# ------------------------------------------------------------------------------------------------ 7: the forward stage
@pytest.mark.parametrize("size", [(1, 1), (7, 9), (8, 8), (9, 3), (24, 16), (65, 17), (257, 8), (640, 480)])
def test_jpeg_forward_device_gives_the_hosts_coefficients(gpu, sdm, size):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    blocks = ((w + 7) // 8) * ((h + 7) // 8)
    for k, kind in enumerate(("smooth", "noise", "edges")):
        rgbx = np.concatenate([image(w, h, kind, rng), rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], 2)
        dev = _dev(rgbx)
        for q in (1, 50, 90, 100):
            want = sdm.jpeg_forward_host(rgbx, q)
            assert want.shape == (blocks, 3, 64)
            o = _Out(blocks * 384, seed=10 * k + q)
            gpu.capi.jpeg_forward_device(dev, w, h, q, o.t)
            o.check(want, "%dx%d %s q%d" % (w, h, kind, q))


def test_jpeg_forward_device_checks_its_arguments(gpu):
    import torch
    from bundlefusion_amd.capi import BFError
    img = torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda")
    out = torch.zeros(192 + 8, dtype=torch.int16, device="cuda")
    with pytest.raises(BFError):
        gpu.capi.jpeg_forward_device(img, 0, 8, 90, out)
    with pytest.raises(BFError):
        gpu.capi.jpeg_forward_device(img, 65536, 8, 90, out)
    with pytest.raises(BFError):
        gpu.capi.jpeg_forward_device(img, 8, 8, 90, out[1:])              # not 16-byte aligned
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ 8: record_device
def _tiny_pipeline(gpu, w=320, h=240):
    """a pipeline that only lends the recorder its device (pinned slots)"""
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = w, h
    gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks, gas.s_SDFVoxelSize = 20000, 8000, 0.02
    gbs.s_widthSIFT, gbs.s_heightSIFT, gbs.s_maxNumImages = w, h, 2
    Kd = synth.intrinsics(w, h)
    return gpu.capi.Pipeline(gas, gbs, sensor_desc(w, h, intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])))


@pytest.fixture(scope="module")
def case(sdm, tmp_path_factory):
    d = tmp_path_factory.mktemp("record_host_route_gpu")
    fr, T = rc.frames(), rc.trajectory()
    return fr, T, rc.host_route(sdm, d / "host.sens", d / "host.tmp.sens", fr, T)


@pytest.mark.parametrize("threads,slots", [(1, 2), (4, 3)])
def test_record_device_writes_the_host_routes_file(gpu, sdm, case, tmp_path, threads, slots):
    import torch
    frames, T, want = case
    gp = _tiny_pipeline(gpu)
    dev = [(_dev(d), _dev(c)) for d, c in frames]
    stream = torch.cuda.Stream()
    rec = sdm.SensRecorder(gp, rc.header(sdm), tmp_path / "t.sens", threads, slots)
    with torch.cuda.stream(stream):
        for i, (d, c) in enumerate(dev):
            rec.record(d, c, stream.cuda_stream)
    name, n = rec.finish(tmp_path / "dev.sens", T)
    rec.close()
    got = open(name, "rb").read()
    assert n == rc.NUM_TRANSFORMS and len(got) == len(want) and got == want
    assert sorted(os.listdir(tmp_path)) == ["dev.sens"]
    gp.close()


# ------------------------------------------------------------------------------------------------ 9: the frame loop
W, H = 640, 480


def _params(w=W, h=H, voxel=0.02, buckets=50000, blocks=20000, max_images=8):
    gas = default_app_state(); gbs = default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = w, h
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = voxel, buckets, blocks
    gbs.s_maxNumImages = max_images
    if (w, h) != (W, H):
        gbs.s_widthSIFT, gbs.s_heightSIFT = w, h
    return gas, gbs


@pytest.fixture(scope="module")
def loop_frames():
    """the 33-frame stream of tests/test_pipeline_gpu.py::_loop_frames, on the host"""
    frames = synth.render_frames(range(33))
    Kd = frames[0][3]
    return intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"]), [(d, c) for d, c, _, _ in frames]


def _loop_run(gpu, sensor, params, feed, n, record_to=None, tmp=None):
    gas, gbs = params
    gp = gpu.capi.Pipeline(gas, gbs, sensor)
    if record_to is not None:
        st = default_record_state()
        st.s_recordData = 1
        st.s_recordDataFile = str(record_to).encode()
        gp.set_record_state(st, 4, str(tmp) + os.sep + "bf_")
    for i in range(n):
        assert feed(gp, i), i
    for _ in range(4):
        gp.process_end_of_sequence()
    gp.synchronize()
    saved = gp.save_recording() if record_to is not None else None
    again = gp.save_recording() if record_to is not None else None
    h, heap, cnt, vox = gp.scene().download()
    res = dict(integrated=gp.integrated_trajectory().copy(), optimised=gp.optimized_trajectory().copy(), counters=gp.counters(), hash=h, heap=heap, count=cnt,
               voxels=vox, saved=saved, again=again)
    gp.close()
    return res


def _assert_same_run(got, want, name):
    for t in ("integrated", "optimised"):
        assert np.array_equal(got[t].view(np.uint32), want[t].view(np.uint32)), name + ": %s trajectory" % t
    assert got["counters"] == want["counters"], name
    assert got["count"] == want["count"] and np.array_equal(got["hash"]["pos"], want["hash"]["pos"]) and np.array_equal(got["hash"]["ptr"], want["hash"]["ptr"]), name + ": hash table"
    assert np.array_equal(got["heap"][:got["count"] + 1], want["heap"][:want["count"] + 1]), name + ": heap"
    assert np.array_equal(got["voxels"].view(np.uint8), want["voxels"].view(np.uint8)), name + ": voxel bytes"


def _check_recording(sdm, run, path, fed, tmp, name):
    """the saved file holds the first numTransforms frames: depth = the rule applied to what was fed, colour = bf_encode_jpeg_rgb at quality 90 of what was fed,
    poses = the trajectory manager's optimised transforms; nothing is left in the temporary directory"""
    saved_name, n = run["saved"]
    assert saved_name == str(path) and run["again"] == ("", 0), name
    opt = run["optimised"]
    assert n == len(opt) > 0, name
    sd = sdm.SensorData(path, use_pillow=False)
    try:
        assert len(sd) == n and sd.info.depthShift == 1000.0 and sd.info.colorCompressionType == sdm.COLOR_JPEG and sd.info.depthCompressionType == sdm.DEPTH_ZLIB_USHORT, name
        assert np.array_equal(sd.trajectory().view(np.uint32), opt.view(np.uint32)), name + ": poses"
        for i in range(n):
            d, c = fed[i]
            assert np.array_equal(sd.depth_raw(i), sdm.record_depth_rule(d, 1000.0)), "%s: depth of frame %d" % (name, i)
            assert sd.color_compressed(i) == sdm.encode_jpeg_rgb(np.ascontiguousarray(c[:, :, :3]), 90), "%s: colour of frame %d" % (name, i)
    finally:
        sd.close()
    assert os.listdir(tmp) == [], name + ": temporary file left behind"


@pytest.mark.parametrize("form", ["host", "device"])
def test_frame_loop_records_and_changes_nothing_it_does_not_own(gpu, sdm, loop_frames, tmp_path, form):
    K, frames = loop_frames
    sensor = sensor_desc(W, H, K)
    fed = [(d.reshape(H, W), c.reshape(H, W, 4)) for d, c in frames]
    if form == "device":
        dev = [(_dev(d), _dev(c)) for d, c in frames]
        feed = lambda gp, i: gp.process_frame(dev[i][0], dev[i][1])
    else:
        feed = lambda gp, i: gp.process_frame(frames[i][0], frames[i][1])
    tmp = tmp_path / "tmp"; tmp.mkdir()
    plain = _loop_run(gpu, sensor, _params(), feed, len(frames))
    rec = _loop_run(gpu, sensor, _params(), feed, len(frames), tmp_path / "scan.sens", tmp)
    assert plain["counters"]["deintegrate"] > 20 and plain["counters"]["global_solves"] >= 3 and len(plain["optimised"]) > 20
    _assert_same_run(rec, plain, form)
    _check_recording(sdm, rec, tmp_path / "scan.sens", fed, tmp, form)
    if form == "device":
        assert all(np.array_equal(a.cpu().numpy().view(np.uint32), np.ascontiguousarray(d).view(np.uint32).reshape(a.shape)) for (a, _), (d, _) in zip(dev, frames)), "the caller's depth was written"


def test_record_state_is_refused_where_it_must_be(gpu, loop_frames, tmp_path):
    from bundlefusion_amd.capi import BFError
    K, frames = loop_frames
    gp = gpu.capi.Pipeline(*_params(), sensor_desc(W, H, K))
    st = default_record_state()
    st.s_recordData, st.s_recordCompression = 1, 0
    with pytest.raises(BFError, match="sensor"):                     # the legacy container
        gp.set_record_state(st, 2, str(tmp_path) + os.sep)
    with pytest.raises(BFError):                                     # nothing records: nothing to save
        gp.save_recording(tmp_path / "x.sens")
    assert gp.process_frame(frames[0][0], frames[0][1])
    st.s_recordCompression = 1
    with pytest.raises(BFError, match="first frame"):
        gp.set_record_state(st, 2, str(tmp_path) + os.sep)
    gp.close()
    assert os.listdir(tmp_path) == []


def test_recorded_depth_is_the_unregistered_one(gpu, sdm, tmp_path):
    """s_bUseCameraCalibration on, a rig whose depth camera is displaced: the loop registers the depth, the recording keeps the sensor's own"""
    from tests import calibrator_cases as cc
    w, h, n = 320, 240, 12
    Kd, Kc = cc.mat(synth.intrinsics(w, h)), cc.mat(cc.colour_intrinsics(w, h))
    rig = sensor_desc(w, h, Kd, color_K=Kc, depth_extrinsics=cc.extrinsics())
    stream = [cc.rig_frame(k, w, h)[:2] for k in range(n)]
    fed = [(np.asarray(d, np.float32).reshape(h, w), np.asarray(c, np.uint8).reshape(h, w, 4)) for d, c in stream]
    dev = [(_dev(d), _dev(c)) for d, c in fed]
    gas, gbs = _params(w, h, buckets=20000, blocks=8000)
    gas.s_bUseCameraCalibration = 1
    tmp = tmp_path / "tmp"; tmp.mkdir()
    for form, feed in (("device", lambda gp, i: gp.process_frame(dev[i][0], dev[i][1])), ("host", lambda gp, i: gp.process_frame(fed[i][0], fed[i][1]))):
        path = tmp_path / (form + ".sens")
        run = _loop_run(gpu, rig, (gas, gbs), feed, n, path, tmp)
        _check_recording(sdm, run, path, fed, tmp, "rig, " + form)


def test_played_file_records_its_own_raw_depth(gpu, sdm, tmp_path, monkeypatch):
    """a .sens of tools/make_sens.py (u16 depth at shift 1000) played through bf_sens_player with recording on: the recorded planes are the source file's"""
    import importlib.util
    n, w, h = 12, 320, 240
    src = tmp_path / "src.sens"
    spec = importlib.util.spec_from_file_location("make_sens", os.path.join(ROOT, "tools", "make_sens.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", ["make_sens.py", str(src), "--frames", str(n), "--width", str(w), "--height", str(h)])
    tool.main()
    sd = sdm.SensorData(src, use_pillow=False)
    gas, gbs = _params(w, h, buckets=20000, blocks=8000)
    gp = gpu.capi.Pipeline(gas, gbs, sd.sensor_desc())
    st = default_record_state()
    st.s_recordData = 1
    tmp = tmp_path / "tmp"; tmp.mkdir()
    gp.set_record_state(st, 2, str(tmp) + os.sep)
    with sdm.SensPlayer(gp, sd, 2) as player:
        count = 0
        while player.next():
            count += 1
    assert count == n
    for _ in range(4):
        gp.process_end_of_sequence()
    name, written = gp.save_recording(tmp_path / "replay.sens")
    opt = gp.optimized_trajectory().copy()
    gp.close()
    assert written == len(opt) > 0 and os.listdir(tmp) == []
    out = sdm.SensorData(name, use_pillow=False)
    assert len(out) == written and (out.info.depthWidth, out.info.depthHeight, out.info.colorWidth, out.info.colorHeight) == (w, h, w, h)
    for i in range(written):
        assert np.array_equal(out.depth_raw(i), sd.depth_raw(i)), "depth of frame %d" % i
        rgbx = sd.color_rgbx(i)
        assert out.color_compressed(i) == sdm.encode_jpeg_rgb(np.ascontiguousarray(rgbx[:, :, :3]), 90), "colour of frame %d" % i
    out.close(); sd.close()
