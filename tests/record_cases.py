"""Shared inputs of tests/test_record_cpu.py and tests/test_record_gpu.py: the 37-frame case of the recorder's back end and the host route it is
held to - bf_sensor_data_writer_add_frame + bf_encode_jpeg_rgb at quality 90 + the depth rule on the calling thread, then
bf_sensor_data_save_recorded: what RGBDSensor::recordFrame / saveRecordedFramesToFile of include/bundlefusion/bundlefusion.hpp always did."""
import numpy as np

from tests.sensor_ingest_streams import image

NUM_FRAMES, NUM_TRANSFORMS = 37, 30
COLOUR_SIZE, DEPTH_SIZE = (40, 24), (24, 16)          # (width, height)


def frames(n=NUM_FRAMES, colour_size=COLOUR_SIZE, depth_size=DEPTH_SIZE, seed=11):
    """[(depth float32 (h, w) metres with invalid values of every kind, rgbx uint8 (h, w, 4) with a random X byte)]"""
    rng = np.random.default_rng(seed)
    (cw, ch), (dw, dh) = colour_size, depth_size
    out = []
    for i in range(n):
        rgb = image(cw, ch, ("smooth", "noise", "edges")[i % 3], rng)
        rgb = np.roll(rgb, i, axis=1)
        rgbx = np.concatenate([rgb, rng.integers(0, 256, (ch, cw, 1), dtype=np.uint8)], 2)
        d = (rng.random((dh, dw), dtype=np.float32) * np.float32(6.0) + np.float32(0.3)).astype(np.float32)
        flat = d.reshape(-1)
        flat[rng.integers(0, flat.size, 8)] = [-np.inf, np.inf, np.nan, 0.0, -0.0, -1.5, 65.5354, 70.0]
        out.append((d, np.ascontiguousarray(rgbx)))
    return out


def trajectory(n=NUM_TRANSFORMS, invalid=7):
    """n camera-to-world poses, pose `invalid` all -inf"""
    T = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for i in range(n):
        a = np.float32(0.01 * i)
        T[i, :3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
        T[i, :3, 3] = [0.02 * i, -0.01 * i, 0.005 * i]
    if 0 <= invalid < n:
        T[invalid] = -np.inf
    return T


def header(sdm, colour_size=COLOUR_SIZE, depth_size=DEPTH_SIZE, name="RGBDSensor"):
    """the SensorDataInfo of a recording: JPEG colour, zlib u16 depth, shift 1000"""
    info = sdm.SensorDataInfo()
    info.versionNumber = 4
    info.sensorName = name.encode()
    K = np.array([[30.0, 0, 11.5, 0], [0, 30.0, 7.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    E = np.eye(4, dtype=np.float32)
    for field, m in (("colorIntrinsic", K * np.float32(1.5)), ("colorExtrinsic", E), ("depthIntrinsic", K), ("depthExtrinsic", E)):
        setattr(info, field, (sdm.C.c_float * 16)(*np.asarray(m, np.float32).reshape(16)))
    info.colorCompressionType, info.depthCompressionType = sdm.COLOR_JPEG, sdm.DEPTH_ZLIB_USHORT
    info.colorWidth, info.colorHeight = colour_size
    info.depthWidth, info.depthHeight = depth_size
    info.depthShift = 1000.0
    return info


def host_route(sdm, path, tmp, frame_list, T, info=None):
    """today's recordFrame + saveRecordedFramesToFile on the calling thread -> the bytes of the final file"""
    info = info if info is not None else header(sdm)
    h = sdm.C.c_void_p()
    sdm.check(sdm.lib.bf_sensor_data_writer_create(str(tmp).encode(), sdm.C.byref(info), sdm.C.byref(h)))
    I = (sdm.C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
    for d, rgbx in frame_list:
        jpeg = sdm.encode_jpeg_rgb(np.ascontiguousarray(rgbx[:, :, :3]), 90)
        u16 = np.ascontiguousarray(sdm.record_depth_rule(d, 1000.0))
        sdm.check(sdm.lib.bf_sensor_data_writer_add_frame(h, I, 0, 0, jpeg, len(jpeg), u16.ctypes.data))
    sdm.check(sdm.lib.bf_sensor_data_writer_close(h))
    sd = sdm.SensorData(tmp, use_pillow=False)
    try:
        sd.save_recorded(path, T)
    finally:
        sd.close()
    return open(path, "rb").read()
