"""ctypes view of include/bf_sensordata.h: recorded RGB-D sequences (".sens", ml::SensorData version 4).

Host-only but for SensPlayer over a pipeline, which feeds the device ingest.  JPEG / PNG colour frames are decoded with Pillow through the C ABI's decoder callback when Pillow is
importable (the reference decodes them with stb_image inside mLib); raw colour and raw / zlib depth need nothing.
"""
import ctypes as C
import io

import numpy as np

from .capi import lib, check, RGBDSensorDesc, JpegInfo, BF_ERR_NOT_ON_DEVICE

COLOR_RAW, COLOR_PNG, COLOR_JPEG = 0, 1, 2
DEPTH_RAW_USHORT, DEPTH_ZLIB_USHORT, DEPTH_OCCI_USHORT = 0, 1, 2


class SensorDataInfo(C.Structure):
    _fields_ = [
        ("versionNumber", C.c_uint32),
        ("sensorName", C.c_char * 256),
        ("colorIntrinsic", C.c_float * 16), ("colorExtrinsic", C.c_float * 16),
        ("depthIntrinsic", C.c_float * 16), ("depthExtrinsic", C.c_float * 16),
        ("colorCompressionType", C.c_int32), ("depthCompressionType", C.c_int32),
        ("colorWidth", C.c_uint32), ("colorHeight", C.c_uint32), ("depthWidth", C.c_uint32), ("depthHeight", C.c_uint32),
        ("depthShift", C.c_float),
        ("numFrames", C.c_uint64), ("numIMUFrames", C.c_uint64),
    ]


_DECODER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8))

lib.bf_sensor_data_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
lib.bf_sensor_data_close.argtypes = [C.c_void_p]
lib.bf_sensor_data_get_info.argtypes = [C.c_void_p, C.POINTER(SensorDataInfo)]
lib.bf_sensor_data_get_sensor_desc.argtypes = [C.c_void_p, C.POINTER(RGBDSensorDesc)]
lib.bf_sensor_data_set_color_decoder.argtypes = [C.c_void_p, _DECODER, C.c_void_p]
lib.bf_sensor_data_get_frame_pose.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
lib.bf_sensor_data_get_frame_sizes.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
lib.bf_sensor_data_read_depth_raw.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
lib.bf_sensor_data_read_depth.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
lib.bf_sensor_data_read_color_compressed.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
lib.bf_sensor_data_read_color_rgbx.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
lib.bf_sensor_data_writer_create.argtypes = [C.c_char_p, C.POINTER(SensorDataInfo), C.POINTER(C.c_void_p)]
lib.bf_sensor_data_writer_add_frame.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
lib.bf_sensor_data_writer_close.argtypes = [C.c_void_p]
lib.bf_sensor_data_save_with_trajectory.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
lib.bf_evaluate_ate_rmse.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
lib.bf_sensor_data_evaluate_trajectory.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
lib.bf_decode_color_rgb.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p]
lib.bf_encode_jpeg_rgb.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
lib.bf_jpeg_forward_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64]
lib.bf_jpeg_entropy_encode.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
lib.bf_sensor_data_writer_add_frame_compressed.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
lib.bf_sensor_data_save_recorded.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
lib.bf_sens_recorder_create.argtypes = [C.c_void_p, C.POINTER(SensorDataInfo), C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
lib.bf_sens_recorder_record_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
lib.bf_sens_recorder_record_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.bf_sens_recorder_get_num_recorded.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
lib.bf_sens_recorder_finish.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
lib.bf_sens_recorder_destroy.argtypes = [C.c_void_p]
lib.bf_jpeg_parse.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(JpegInfo)]
lib.bf_jpeg_entropy_decode.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(JpegInfo), C.c_void_p, C.c_uint64]
lib.bf_jpeg_reconstruct_host.argtypes = [C.POINTER(JpegInfo), C.c_void_p, C.c_void_p]


class SensFrame(C.Structure):
    _fields_ = [("frame", C.c_uint64), ("depthU16", C.c_void_p), ("colour", C.c_void_p), ("colourBytes", C.c_uint64), ("jpegCoefficients", C.c_int32), ("jpeg", JpegInfo)]


lib.bf_sens_player_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
lib.bf_sens_player_next.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
lib.bf_sens_player_peek.argtypes = [C.c_void_p, C.POINTER(SensFrame), C.POINTER(C.c_int)]
lib.bf_sens_player_destroy.argtypes = [C.c_void_p]


def decode_color_rgb(blob, compression, width, height):
    """the built-in colour decoder (bf_decode_color_rgb): stored bytes -> RGB8 (h, w, 3)"""
    buf = np.frombuffer(blob, np.uint8)
    out = np.empty((height, width, 3), np.uint8)
    check(lib.bf_decode_color_rgb(buf.ctypes.data, buf.size, compression, width, height, out.ctypes.data))
    return out


def encode_jpeg_rgb(rgb, quality=90):
    """baseline 4:4:4 JPEG of an RGB8 image (bf_encode_jpeg_rgb), as bytes"""
    a = np.ascontiguousarray(rgb, np.uint8)
    h, w = a.shape[:2]
    n = C.c_uint64()
    check(lib.bf_encode_jpeg_rgb(a.ctypes.data, w, h, quality, None, 0, C.byref(n)))
    buf = np.empty(n.value, np.uint8)
    check(lib.bf_encode_jpeg_rgb(a.ctypes.data, w, h, quality, buf.ctypes.data, n.value, C.byref(n)))
    return buf.tobytes()


def jpeg_forward_host(pixels, quality=90):
    """the encoder's forward stage (bf_jpeg_forward_host): RGB8 (h, w, 3) or RGBX8 (h, w, 4) -> int16 (blocks, 3, 64), zigzag order"""
    a = np.ascontiguousarray(pixels, np.uint8)
    h, w, stride = a.shape
    coef = np.empty((((w + 7) // 8) * ((h + 7) // 8), 3, 64), np.int16)
    check(lib.bf_jpeg_forward_host(a.ctypes.data, stride, w, h, quality, coef.ctypes.data, coef.size))
    return coef


def jpeg_entropy_encode(coef, width, height, quality=90):
    """the encoder's entropy stage (bf_jpeg_entropy_encode): the coefficients of jpeg_forward_host -> the JPEG stream, as bytes"""
    c = np.ascontiguousarray(coef, np.int16)
    assert c.size == ((width + 7) // 8) * ((height + 7) // 8) * 192
    n = C.c_uint64()
    check(lib.bf_jpeg_entropy_encode(width, height, quality, c.ctypes.data, None, 0, C.byref(n)))
    buf = np.empty(n.value, np.uint8)
    check(lib.bf_jpeg_entropy_encode(width, height, quality, c.ctypes.data, buf.ctypes.data, n.value, C.byref(n)))
    return buf.tobytes()


def jpeg_parse(blob, width=0, height=0):
    """headers of a baseline JPEG stream -> JpegInfo (bf_jpeg_parse); width x height: the size the container states (0 x 0: any)"""
    buf = np.frombuffer(blob, np.uint8)
    info = JpegInfo()
    check(lib.bf_jpeg_parse(buf.ctypes.data, buf.size, width, height, C.byref(info)))
    return info


def jpeg_entropy_decode(blob, info):
    """the scan's quantised coefficients, int16 (numBlocks, 64) in the layout of bf_jpeg_info, or None where they do not fit int16 (BF_ERR_NOT_ON_DEVICE)"""
    buf = np.frombuffer(blob, np.uint8)
    coef = np.empty((info.numBlocks, 64), np.int16)
    rc = lib.bf_jpeg_entropy_decode(buf.ctypes.data, buf.size, C.byref(info), coef.ctypes.data, coef.size)
    if rc == BF_ERR_NOT_ON_DEVICE:
        return None
    check(rc)
    return coef


def jpeg_reconstruct_host(info, coef):
    """coefficients -> RGB8 (h, w, 3) on the host: the image the device reconstruction gives"""
    coef = np.ascontiguousarray(coef, np.int16)
    assert coef.size == info.numBlocks * 64
    out = np.empty((info.height, info.width, 3), np.uint8)
    check(lib.bf_jpeg_reconstruct_host(C.byref(info), coef.ctypes.data, out.ctypes.data))
    return out


def _pillow_decode(_user, data, size, _ctype, width, height, out):
    try:
        from PIL import Image
        img = Image.open(io.BytesIO(C.string_at(data, size))).convert("RGB")
        if img.size != (width, height):
            return 1
        C.memmove(out, img.tobytes(), width * height * 3)
        return 0
    except Exception:           # the C side turns a non-zero return into "the colour decoder failed"
        return 1


class SensorData:
    """A .sens file opened for reading (SensorData::loadFromFile + the accessors SensorDataReader uses)."""

    def __init__(self, filename, use_pillow=True):
        self._h = C.c_void_p()
        check(lib.bf_sensor_data_open(str(filename).encode(), C.byref(self._h)))
        self.info = SensorDataInfo()
        check(lib.bf_sensor_data_get_info(self._h, C.byref(self.info)))
        self._cb = None
        if use_pillow and self.info.colorCompressionType in (COLOR_PNG, COLOR_JPEG):
            try:
                import PIL  # noqa: F401
                self._cb = _DECODER(_pillow_decode)
                check(lib.bf_sensor_data_set_color_decoder(self._h, self._cb, None))
            except ImportError:
                pass

    def close(self):
        if self._h:
            lib.bf_sensor_data_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self.info.numFrames)

    @property
    def sensor_name(self):
        return self.info.sensorName.decode()

    def sensor_desc(self):
        d = RGBDSensorDesc()
        check(lib.bf_sensor_data_get_sensor_desc(self._h, C.byref(d)))
        return d

    def pose(self, i):
        T = (C.c_float * 16)()
        tc, td = C.c_uint64(), C.c_uint64()
        check(lib.bf_sensor_data_get_frame_pose(self._h, i, T, C.byref(tc), C.byref(td)))
        return np.array(T, np.float32).reshape(4, 4), tc.value, td.value

    def frame_sizes(self, i):
        a, b = C.c_uint64(), C.c_uint64()
        check(lib.bf_sensor_data_get_frame_sizes(self._h, i, C.byref(a), C.byref(b)))
        return a.value, b.value

    def depth_raw(self, i):
        out = np.empty((self.info.depthHeight, self.info.depthWidth), np.uint16)
        check(lib.bf_sensor_data_read_depth_raw(self._h, i, out.ctypes.data))
        return out

    def depth(self, i):
        """float32 metres, -inf where the stored value is 0 (SensorDataReader::processDepth)."""
        out = np.empty((self.info.depthHeight, self.info.depthWidth), np.float32)
        check(lib.bf_sensor_data_read_depth(self._h, i, out.ctypes.data))
        return out

    def color_compressed(self, i):
        n = C.c_uint64()
        check(lib.bf_sensor_data_read_color_compressed(self._h, i, None, 0, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        check(lib.bf_sensor_data_read_color_compressed(self._h, i, buf.ctypes.data, n.value, C.byref(n)))
        return buf.tobytes()

    def color_rgbx(self, i):
        out = np.empty((max(self.info.colorHeight, 1), max(self.info.colorWidth, 1), 4), np.uint8)
        check(lib.bf_sensor_data_read_color_rgbx(self._h, i, out.ctypes.data))
        return out

    def trajectory(self):
        """cameraToWorld of every frame (SensorDataReader::getTrajectory)."""
        return np.stack([self.pose(i)[0] for i in range(len(self))]) if len(self) else np.zeros((0, 4, 4), np.float32)

    def save_with_trajectory(self, filename, trajectory):
        """SensorDataReader::saveToFile(filename, trajectory): frames beyond the trajectory get an all -inf pose."""
        T = np.ascontiguousarray(trajectory, np.float32).reshape(-1, 16)
        check(lib.bf_sensor_data_save_with_trajectory(self._h, str(filename).encode(), T.ctypes.data if len(T) else None, len(T)))

    def save_recorded(self, filename, trajectory):
        """RGBDSensor::saveRecordedFramesToFile: the first len(trajectory) frames, each with its pose"""
        T = np.ascontiguousarray(trajectory, np.float32).reshape(-1, 16)
        check(lib.bf_sensor_data_save_recorded(self._h, str(filename).encode(), T.ctypes.data if len(T) else None, len(T)))

    def evaluate_trajectory(self, trajectory):
        """SensorDataReader::evaluateTrajectory: (ATE RMSE [m], number of poses used) against the stored poses re-based to identity."""
        T = np.ascontiguousarray(trajectory, np.float32).reshape(-1, 16)
        rmse, n = C.c_float(), C.c_uint32()
        check(lib.bf_sensor_data_evaluate_trajectory(self._h, T.ctypes.data, len(T), C.byref(rmse), C.byref(n)))
        return rmse.value, n.value


class SensPlayer:
    """Decode-ahead player (bf_sens_player): `threads` workers read, inflate and entropy-decode the frames of `sensor_data` ahead of the loop; next() hands
    the next frame, in order, to `pipeline`'s device ingest.  pipeline None: decode only - peek() shows the slot next() would hand over (no GPU needed).
    Open the file with SensorData(path, use_pillow=False): a decoder callback would be called from every worker thread, and its frames travel as RGB8."""

    def __init__(self, pipeline, sensor_data, threads=4):
        self._h = C.c_void_p()
        self._pipe, self._sd = pipeline, sensor_data                      # both must outlive the player
        check(lib.bf_sens_player_create(pipeline._h if pipeline is not None else None, sensor_data._h, int(threads), C.byref(self._h)))

    def close(self):
        if self._h:
            lib.bf_sens_player_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def next(self):
        """-> whether a frame was handed over (False at the end of the file); raises at the frame that failed to decode"""
        got = C.c_int()
        check(lib.bf_sens_player_next(self._h, C.byref(got)))
        return bool(got.value)

    def peek(self):
        """copies of the next frame's slot: (frame, depth u16 (h, w), colour, JpegInfo or None) - colour is RGB8 (h, w, 3), or int16 coefficients (numBlocks, 64)
        with a JpegInfo; None at the end of the file"""
        fr, got = SensFrame(), C.c_int()
        check(lib.bf_sens_player_peek(self._h, C.byref(fr), C.byref(got)))
        if not got.value:
            return None
        i = self._sd.info
        depth = np.frombuffer((C.c_uint8 * (i.depthWidth * i.depthHeight * 2)).from_address(fr.depthU16), np.uint16).reshape(i.depthHeight, i.depthWidth).copy()
        raw = np.frombuffer((C.c_uint8 * fr.colourBytes).from_address(fr.colour), np.uint8).copy()
        if fr.jpegCoefficients:
            info = JpegInfo.from_buffer_copy(fr.jpeg)
            return fr.frame, depth, raw.view(np.int16).reshape(info.numBlocks, 64), info
        return fr.frame, depth, raw.reshape(i.colorHeight, i.colorWidth, 3), None


class SensorDataWriter:
    """SensorData::saveToFile, frame by frame."""

    def __init__(self, filename, depth_size, color_size, depth_intrinsic, color_intrinsic=None, depth_shift=1000.0, sensor_name="synthetic",
                 depth_compression=DEPTH_ZLIB_USHORT, color_compression=COLOR_RAW, depth_extrinsic=None, color_extrinsic=None):
        info = SensorDataInfo()
        info.versionNumber = 4
        info.sensorName = sensor_name.encode()[:255]
        eye = np.eye(4, dtype=np.float32)
        for name, m in (("depthIntrinsic", depth_intrinsic), ("colorIntrinsic", depth_intrinsic if color_intrinsic is None else color_intrinsic),
                        ("depthExtrinsic", eye if depth_extrinsic is None else depth_extrinsic),
                        ("colorExtrinsic", eye if color_extrinsic is None else color_extrinsic)):
            setattr(info, name, (C.c_float * 16)(*np.asarray(m, np.float32).reshape(16)))
        info.depthWidth, info.depthHeight = depth_size
        info.colorWidth, info.colorHeight = color_size
        info.depthShift = depth_shift
        info.depthCompressionType = depth_compression
        info.colorCompressionType = color_compression
        self.info = info
        self._h = C.c_void_p()
        check(lib.bf_sensor_data_writer_create(str(filename).encode(), C.byref(info), C.byref(self._h)))

    def add_frame(self, camera_to_world, depth_u16, color_bytes=b"", ts_color=0, ts_depth=0):
        d = np.ascontiguousarray(depth_u16, np.uint16)
        assert d.size == self.info.depthWidth * self.info.depthHeight
        T = (C.c_float * 16)(*np.asarray(camera_to_world, np.float32).reshape(16))
        cb = bytes(color_bytes)
        check(lib.bf_sensor_data_writer_add_frame(self._h, T, ts_color, ts_depth, cb if cb else None, len(cb), d.ctypes.data))

    def close(self):
        if self._h:
            h, self._h = self._h, C.c_void_p()
            check(lib.bf_sensor_data_writer_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def record_depth_rule(depth_m, depth_shift=1000.0):
    """the recording's depth rule (RGBDSensor.cpp:305) in float32 numpy operations, in the library's order: v = d * shift; 0 < v < 65535.5 ? u16(v + 0.5) : 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(depth_m, np.float32) * np.float32(depth_shift)).astype(np.float32)
        ok = (v > np.float32(0)) & (v < np.float32(65535.5))
        r = (np.where(ok, v, np.float32(0)) + np.float32(0.5)).astype(np.float32)
    return np.where(ok, r.astype(np.uint16), np.uint16(0)).astype(np.uint16)


class SensRecorder:
    """bf_sens_recorder: the front half of a frame (coefficients + u16 depth) goes into a ring of slots, `threads` workers entropy-code and deflate, the blobs are
    appended to `tmp_filename` in frame order; finish() attaches the trajectory and writes the .sens.  pipeline None: host frames only, no GPU needed.
    info: a SensorDataInfo (JPEG colour; SensorDataWriter(...).info has the layout)."""

    def __init__(self, pipeline, info, tmp_filename, threads=0, slots=0):
        self._h = C.c_void_p()
        self._pipe = pipeline
        self.info = info
        check(lib.bf_sens_recorder_create(pipeline._h if pipeline is not None else None, C.byref(info), str(tmp_filename).encode(), int(threads), int(slots), C.byref(self._h)))

    def close(self):
        if self._h:
            lib.bf_sens_recorder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def record(self, depth, rgbx, stream=0):
        """depth float32 metres, rgbx uint8 (h, w, 4): host numpy arrays (packed on the calling thread) or torch device tensors (packed on `stream`)"""
        if isinstance(depth, np.ndarray):
            d = np.ascontiguousarray(depth, np.float32); c = np.ascontiguousarray(rgbx, np.uint8)
            assert d.size == self.info.depthWidth * self.info.depthHeight and c.size == self.info.colorWidth * self.info.colorHeight * 4
            check(lib.bf_sens_recorder_record_host(self._h, c.ctypes.data, d.ctypes.data))
        else:
            assert depth.numel() == self.info.depthWidth * self.info.depthHeight and rgbx.numel() == self.info.colorWidth * self.info.colorHeight * 4
            check(lib.bf_sens_recorder_record_device(self._h, depth.data_ptr(), rgbx.data_ptr(), stream))

    def num_recorded(self):
        n = C.c_uint64()
        check(lib.bf_sens_recorder_get_num_recorded(self._h, C.byref(n)))
        return n.value

    def finish(self, filename, trajectory, overwrite=False):
        """-> (name written, frames written)"""
        T = np.ascontiguousarray(trajectory, np.float32).reshape(-1, 16)
        name = C.create_string_buffer(4096); n = C.c_uint64()
        check(lib.bf_sens_recorder_finish(self._h, str(filename).encode(), T.ctypes.data if len(T) else None, len(T), int(bool(overwrite)), name, len(name), C.byref(n)))
        return name.value.decode(), n.value


def depth_to_u16(depth_m, depth_shift=1000.0):
    """metres (non-finite / non-positive = invalid) -> the stored u16 (0 = invalid), rounding to nearest like a sensor would."""
    d = np.asarray(depth_m, np.float32)
    ok = np.isfinite(d) & (d > 0)
    q = np.zeros(d.shape, np.uint16)
    q[ok] = np.clip(np.rint(d[ok] * depth_shift), 1, 65535).astype(np.uint16)
    return q


def ate_rmse(trajectory, reference):
    """PoseHelper::evaluateAteRmse: (RMSE of the camera positions after a rigid alignment, number of poses used)."""
    A = np.ascontiguousarray(trajectory, np.float32).reshape(-1, 16)
    B = np.ascontiguousarray(reference, np.float32).reshape(-1, 16)
    n = min(len(A), len(B))
    rmse, num = C.c_float(), C.c_uint32()
    check(lib.bf_evaluate_ate_rmse(A.ctypes.data if n else None, B.ctypes.data if n else None, n, C.byref(rmse), C.byref(num)))
    return rmse.value, num.value
