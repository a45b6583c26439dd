"""GPU tests (-m gpu) of the sensor-format ingest (csrc/sensoringest.hip, bf_image_manager_process_raw*, bf_pipeline_process_frame_raw*,
bf_sens_player): u16 depth and RGB8 / JPEG colour converted and reconstructed on the device against the host path that
bf_sensor_data_read_depth / bf_decode_color_rgb / bf_sensor_data_read_color_rgbx are.

Tolerance: none.  The depth conversion is one IEEE float32 division, the colour path is integer arithmetic shared with the host
(csrc/bf_jpeg_recon.h): every result is compared as BYTES, device outputs behind a sentinel pattern with a guard tail.
"""
import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import default_app_state, default_bundling_state, intrinsics_matrix, sensor_desc
from tests.sensor_ingest_streams import encoded_streams, fixture_streams, image as _image, vertical_only_stream

pytestmark = pytest.mark.gpu

GUARD_BYTES = 4096
LENGTHS = (1, 63, 64, 65, 640 * 480 + 1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Out:
    """A device output pre-filled with sentinel bytes and followed by a guard tail of sentinel bytes (tests/test_ingest_gpu.py)."""

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


# ------------------------------------------------------------------------------------------------ 1, 2: the conversions
@pytest.mark.parametrize("shift", [1000.0, 5000.0, 1.0, 999.5, 0.25])
def test_depth_conversion_every_u16_value(gpu, shift):
    """all 65 536 values: 0 -> -inf, otherwise float32(raw) / float32(shift), correctly rounded - numpy's float32 division"""
    raw = np.arange(65536, dtype=np.uint16)
    with np.errstate(divide="ignore"):
        want = (raw.astype(np.float32) / np.float32(shift)).astype(np.float32)
    want[0] = -np.inf
    o = _Out(raw.size * 4, seed=1)
    gpu.capi.image_convert_depth_u16(o.t, _dev(raw), shift)
    o.check(want, "depth shift %g" % shift)


@pytest.mark.parametrize("n", LENGTHS)
def test_depth_conversion_lengths(gpu, n):
    rng = np.random.default_rng(n)
    raw = rng.integers(0, 65536, n).astype(np.uint16)
    raw[rng.random(n) < 0.1] = 0
    raw[-1] = 65535
    for shift in (1000.0, 999.5):
        want = (raw.astype(np.float32) / np.float32(shift)).astype(np.float32)
        want[raw == 0] = -np.inf
        o = _Out(n * 4, seed=2)
        gpu.capi.image_convert_depth_u16(o.t, _dev(raw), shift)
        o.check(want, "depth n=%d shift %g" % (n, shift))


@pytest.mark.parametrize("n", LENGTHS)
def test_rgb8_to_rgbx(gpu, n):
    rgb = np.random.default_rng(n + 7).integers(0, 256, (n, 3), dtype=np.uint8)
    want = np.concatenate([rgb, np.full((n, 1), 255, np.uint8)], 1)
    o = _Out(n * 4, seed=3)
    gpu.capi.image_convert_rgb8_to_rgbx(o.t, _dev(rgb))
    o.check(want, "rgbx n=%d" % n)


# ------------------------------------------------------------------------------------------------ 3: JPEG reconstruction
def _reconstruct_on_device(gpu, sdm, blob, w, h, seed):
    """-> None if every byte is right; the device may decline NONE of these streams"""
    ref = sdm.decode_color_rgb(blob, sdm.COLOR_JPEG, w, h)
    want = np.concatenate([ref, np.full((h, w, 1), 255, np.uint8)], 2)
    info = sdm.jpeg_parse(blob, w, h)
    coef = sdm.jpeg_entropy_decode(blob, info)
    assert coef is not None, "the entropy decoder handed an ordinary stream back to the host"
    planes = _Out(info.planeBytes, seed=seed)
    o = _Out(w * h * 4, seed=seed + 1)
    took = gpu.capi.jpeg_reconstruct_device(info, _dev(coef), planes.t, o.t)
    assert took is True, "the device declined an 8-bit baseline stream in a required layout"
    o.check(want, "%dx%d" % (w, h))
    import torch
    assert np.array_equal(planes.buf.cpu().numpy()[planes.n:], planes.init[planes.n:]), "guard tail of the sample planes written"


def test_jpeg_reconstruction_on_every_fixture_stream(gpu):
    from bundlefusion_amd import sensordata as sdm
    streams = fixture_streams()
    assert len(streams) > 400
    for n, (blob, w, h, layout, q, restart, kind) in enumerate(streams):
        try:
            _reconstruct_on_device(gpu, sdm, blob, w, h, n)
        except AssertionError as e:
            raise AssertionError("stream %d (%dx%d layout %d q%d restart %d kind %d): %s" % (n, w, h, layout, q, restart, kind, e))


def test_jpeg_reconstruction_on_the_encoders_streams(gpu):
    from bundlefusion_amd import sensordata as sdm
    for n, (blob, w, h) in enumerate(encoded_streams(sdm)):          # among them 640x480 and 1296x968
        _reconstruct_on_device(gpu, sdm, blob, w, h, 1000 + n)


def test_jpeg_layout_the_device_declines_is_declined_not_wrong(gpu):
    """chroma sub-sampled vertically only (1x2): the host decoder reads it, the device returns its status and writes nothing"""
    from bundlefusion_amd import sensordata as sdm
    from bundlefusion_amd.capi import BFError
    blob, w, h = vertical_only_stream()
    info = sdm.jpeg_parse(blob, w, h)
    assert (info.comp[0].h, info.comp[0].v, info.comp[1].h, info.comp[1].v) == (1, 2, 1, 1)
    ref = sdm.decode_color_rgb(blob, sdm.COLOR_JPEG, w, h)
    coef = sdm.jpeg_entropy_decode(blob, info)
    assert np.array_equal(sdm.jpeg_reconstruct_host(info, coef), ref)
    planes, o = _Out(info.planeBytes, 5), _Out(w * h * 4, 6)
    assert gpu.capi.jpeg_reconstruct_device(info, _dev(coef), planes.t, o.t) is False
    o.check(o.init[:o.n], "declined stream: output untouched")
    planes.check(planes.init[:planes.n], "declined stream: planes untouched")
    # and the image manager decodes such a frame on the host inside the call
    im, _ = _manager(gpu, w, h, w, h, w, h, 1, 1)
    d = np.full((h, w), 1200, np.uint16)
    assert im.process_raw(d, 1000.0, blob, sdm.COLOR_JPEG)
    want = np.concatenate([ref, np.full((h, w, 1), 255, np.uint8)], 2)
    assert np.array_equal(im.get_input_gpu()[2], want)
    with pytest.raises(BFError):
        im.process_raw(_dev(d), 1000.0, _dev(coef), jpeg=info)        # device-resident coefficients: there is no host to fall back to
    im.close()


# ------------------------------------------------------------------------------------------------ 4: image manager
def _manager(gpu, dw, dh, cw, ch, wi, hi, erode, depth_filter):
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = wi, hi
    gbs.s_widthSIFT, gbs.s_heightSIFT = cw, ch
    gbs.s_erodeSIFTdepth, gbs.s_depthFilter = int(erode), int(depth_filter)
    s = sensor_desc(dw, dh, intrinsics_matrix(0.8 * dw, 0.8 * dw, dw / 2, dh / 2))
    s.colorWidth, s.colorHeight = cw, ch
    return gpu.capi.ImageManager(gas, gbs, s, 1), gbs


def _sensor_frame(dw, dh, cw, ch, seed):
    """u16 depth with level steps around the erosion threshold and invalid pixels; an RGB8 image"""
    rng = np.random.default_rng(seed)
    levels = np.array([1000, 1049, 1051, 1099, 1101, 2500], np.uint16)
    d = np.repeat(np.repeat(levels[rng.integers(0, len(levels), ((dh + 1) // 2, (dw + 2) // 3))], 2, axis=0), 3, axis=1)[:dh, :dw].copy()
    d[rng.random((dh, dw)) < 0.05] = 0
    rgb = _image(cw, ch, ("smooth", "noise", "edges")[seed % 3], rng)
    return d, rgb


MANAGER_SIZES = (((64, 48), (64, 48), (64, 48)), ((64, 48), (130, 97), (64, 48)), ((130, 97), (65, 40), (64, 48)), ((640, 480), (640, 480), (640, 480)))


@pytest.mark.parametrize("sizes", MANAGER_SIZES, ids=lambda s: "d%dx%d_c%dx%d_i%dx%d" % (s[0] + s[1] + s[2]))
@pytest.mark.parametrize("erode,depth_filter", ((1, 1), (1, 0), (0, 1), (0, 0)), ids=("erode_filter", "erode", "filter", "neither"))
def test_image_manager_raw_equals_host_path(gpu, sizes, erode, depth_filter):
    """The same frames as (a) host-decoded float depth + RGBX through bf_image_manager_process and (b) u16 + stored colour bytes (JPEG, raw RGB8, PNG) through
    bf_image_manager_process_raw, (c) decoded host buffers, (d) device buffers: sensor-resolution inputs and stored frames equal byte for byte, frame after
    frame (six frames: the staging slots and the input sets rotate)."""
    import io
    from bundlefusion_amd import sensordata as sdm
    (dw, dh), (cw, ch), (wi, hi) = sizes
    shift = 1000.0
    frames = []
    for i in range(6):
        d, rgb = _sensor_frame(dw, dh, cw, ch, 80 + i)
        kind = ("jpeg", "raw", "jpeg")[i % 3]
        blob = sdm.encode_jpeg_rgb(rgb, 92) if kind == "jpeg" else rgb.tobytes()
        comp = sdm.COLOR_JPEG if kind == "jpeg" else sdm.COLOR_RAW
        if i == 4:
            try:
                from PIL import Image
                buf = io.BytesIO(); Image.fromarray(rgb).save(buf, format="PNG")
                blob, comp = buf.getvalue(), sdm.COLOR_PNG
            except ImportError:
                pass
        frames.append((d, blob, comp))
    host, _ = _manager(gpu, dw, dh, cw, ch, wi, hi, erode, depth_filter)
    legs = {name: _manager(gpu, dw, dh, cw, ch, wi, hi, erode, depth_filter)[0] for name in ("stored", "decoded", "device")}
    for i, (d, blob, comp) in enumerate(frames):
        depth = (d.astype(np.float32) / np.float32(shift)).astype(np.float32)
        depth[d == 0] = -np.inf
        rgb = sdm.decode_color_rgb(blob, comp, cw, ch)
        rgbx = np.concatenate([rgb, np.full((ch, cw, 1), 255, np.uint8)], 2)
        assert host.process(depth, rgbx)
        info = coef = None
        if comp == sdm.COLOR_JPEG:
            info = sdm.jpeg_parse(blob, cw, ch); coef = sdm.jpeg_entropy_decode(blob, info)
        assert legs["stored"].process_raw(d, shift, blob, comp)
        assert legs["decoded"].process_raw(d, shift, coef if info is not None else rgb, jpeg=info)
        assert legs["device"].process_raw(_dev(d), shift, _dev(coef if info is not None else rgb), jpeg=info)
        want_in, want_fr = host.get_input_gpu(), host.get_integrate_frame_cpu(i)
        for name, im in legs.items():
            got_in, got_fr = im.get_input_gpu(), im.get_integrate_frame_cpu(i)
            for k, part in enumerate(("raw depth", "filtered depth", "colour")):
                assert np.array_equal(got_in[k].view(np.uint8), want_in[k].view(np.uint8)), "%s frame %d: sensor-resolution %s" % (name, i, part)
            assert np.array_equal(got_fr[0].view(np.uint8), want_fr[0].view(np.uint8)), "%s frame %d: stored depth" % (name, i)
            assert np.array_equal(got_fr[1], want_fr[1]), "%s frame %d: stored colour" % (name, i)
    for i in (0, 3):                                                   # earlier frames still hold their own images
        want_fr = host.get_integrate_frame_cpu(i)
        for name, im in legs.items():
            got_fr = im.get_integrate_frame_cpu(i)
            assert np.array_equal(got_fr[0].view(np.uint8), want_fr[0].view(np.uint8)) and np.array_equal(got_fr[1], want_fr[1]), (name, i)
    host.close()
    for im in legs.values():
        im.close()


def test_image_manager_raw_rejects_bad_frames(gpu):
    from bundlefusion_amd import sensordata as sdm
    from bundlefusion_amd.capi import BFError
    im, _ = _manager(gpu, 16, 12, 16, 12, 16, 12, 1, 1)
    d, rgb = _sensor_frame(16, 12, 16, 12, 3)
    with pytest.raises(BFError, match="wrong size"):
        im.process_raw(d, 1000.0, rgb.tobytes()[:-3], sdm.COLOR_RAW)
    with pytest.raises(BFError, match="expected"):
        im.process_raw(d, 1000.0, sdm.encode_jpeg_rgb(_image(24, 12, "smooth", None), 90), sdm.COLOR_JPEG)
    with pytest.raises(BFError, match="depthShift"):
        im.process_raw(d, 0.0, rgb.tobytes(), sdm.COLOR_RAW)
    assert im.num_frames() == 0
    assert im.process_raw(d, 1000.0, rgb.tobytes(), sdm.COLOR_RAW) and im.num_frames() == 1
    im.close()


# ------------------------------------------------------------------------------------------------ 5: the frame loop
W, H = 640, 480


def _loop_params(voxel, buckets, blocks):
    gas = default_app_state(); gbs = default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = W, H
    gas.s_SDFVoxelSize, gas.s_hashNumBuckets, gas.s_hashNumSDFBlocks = voxel, buckets, blocks
    gbs.s_maxNumImages = 8
    return gas, gbs


@pytest.fixture(scope="module")
def sensor_stream(tmp_path_factory):
    """43 synthetic frames in sensor format (u16 depth at shift 1000, JPEG q92 colour) and the .sens file that holds them"""
    from bundlefusion_amd import sensordata as sdm
    frames = synth.render_frames(range(43))
    Kd = frames[0][3]
    K = intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])
    raw = [(sdm.depth_to_u16(d, 1000.0), sdm.encode_jpeg_rgb(np.ascontiguousarray(c[:, :, :3]), 92)) for d, c, _, _ in frames]
    path = tmp_path_factory.mktemp("sens") / "stream.sens"
    K4 = np.eye(4, dtype=np.float32); K4[0, 0], K4[1, 1], K4[0, 2], K4[1, 2] = Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"]
    with sdm.SensorDataWriter(path, (W, H), (W, H), K4, depth_shift=1000.0, color_compression=sdm.COLOR_JPEG) as wr:
        for (d, blob), (_, _, T, _) in zip(raw, frames):
            wr.add_frame(T, d, blob)
    return raw, K, path


@pytest.mark.parametrize("config", ["exact_serial", "shipped"])
def test_frame_loop_raw_ingest_equals_host_decoded_frames(gpu, sensor_stream, config):
    """43 frames (four closed chunks, global solves, re-integrations) (i) host-decoded through process_frame, (ii) through process_frame_raw, (iii) from the
    .sens file through the player with 1 and with 4 threads: optimised and integrated trajectories, counters, hash table, heap and every voxel byte agree, compared
    the way test_pipeline_gpu.py::test_frame_loop_is_deterministic compares two runs.  Once under the suite's configuration (exact contract, serial solves), once
    under the shipped one (fast contract, solve lag 10)."""
    from bundlefusion_amd import sensordata as sdm
    raw, K, path = sensor_stream
    n = len(raw)

    def pipeline():
        gas, gbs = _loop_params(0.004, 1000000, 250000) if config == "shipped" else _loop_params(0.02, 50000, 20000)
        gp = gpu.capi.Pipeline(gas, gbs, sensor_desc(W, H, K))
        if config == "shipped":
            gp.scene().set_arith("fast")
            gp.set_solve_lag(10)
            assert gp.solve_lag() == 10
        return gp

    def finish(gp):
        for _ in range(4):
            gp.process_end_of_sequence()
        gp.synchronize()
        h, heap, cnt, vox = gp.scene().download()
        return gp.integrated_trajectory().copy(), gp.optimized_trajectory().copy(), gp.counters(), h, heap, cnt, vox

    def host_decoded():
        sd = sdm.SensorData(path, use_pillow=False)
        gp = pipeline()
        for i in range(n):
            assert gp.process_frame(sd.depth(i), sd.color_rgbx(i))
        sd.close()
        return finish(gp)

    def raw_frames():
        gp = pipeline()
        for d, blob in raw:
            assert gp.process_frame_raw(d, 1000.0, blob, sdm.COLOR_JPEG)
        return finish(gp)

    def player(threads):
        sd = sdm.SensorData(path, use_pillow=False)
        gp = pipeline()
        with sdm.SensPlayer(gp, sd, threads) as pl:
            for i in range(n):
                assert pl.next() is True, i
            assert pl.next() is False
        out = finish(gp)
        sd.close()
        return out

    ref = host_decoded()
    # so that equality says something: every frame tracked, chunks closed and solved, frames re-integrated
    assert len(ref[0]) == n and np.isfinite(ref[0][:, 0, 0]).all(), "frames lost: %s" % np.flatnonzero(~np.isfinite(ref[0][:, 0, 0])).tolist()
    assert ref[2]["deintegrate"] >= 1 and ref[2]["global_solves"] >= 4 and ref[2]["local_solves"] >= 4, ref[2]
    for name, run in (("process_frame_raw", raw_frames), ("player, 1 thread", lambda: player(1)), ("player, 4 threads", lambda: player(4))):
        got = run()
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), name + ": integrated trajectory"
        assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), name + ": optimised trajectory"
        assert got[2] == ref[2], name
        assert np.array_equal(got[3]["pos"], ref[3]["pos"]) and np.array_equal(got[3]["ptr"], ref[3]["ptr"]) and got[5] == ref[5], name + ": hash table"
        assert np.array_equal(got[4][:got[5] + 1], ref[4][:ref[5] + 1]), name + ": heap"
        diff = np.nonzero((got[6]["sdf"] != ref[6]["sdf"]) | (got[6]["weight"] != ref[6]["weight"]) | (got[6]["color"] != ref[6]["color"]).any(axis=1))[0]
        print("%s [%s] vs host-decoded frames: %d of %d voxels differ" % (name, config, len(diff), len(got[6])))
        assert len(diff) == 0, "%s: %d voxels differ (first: %s)" % (name, len(diff), diff[:8].tolist())
