"""CPU tests (-m "not gpu") of the recording (include/bf_record.h): the JPEG encoder split into bf_jpeg_forward_host + bf_jpeg_entropy_encode with its
bytes unchanged, the recorder's threaded back end against the host route on the calling thread, the recording keys of the parameter file.

Tolerance: none - every comparison is of bytes (or of SHA-256 digests of bytes).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import record_cases as rc
from tests.sensor_ingest_streams import image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "bundlefusion_amd", "lib")
FIXTURE = os.path.join(ROOT, "tests", "golden", "jpeg_encoder_parent.npz")


@pytest.fixture(scope="module")
def sdm(built):
    from bundlefusion_amd import sensordata
    return sensordata


# ------------------------------------------------------------------------------------------------ 1, 2: the encoder
def test_encoder_still_gives_the_digests_taken_before_the_split(sdm):
    """tests/golden/jpeg_encoder_parent.npz was written by tools/make_jpeg_encoder_fixture.py on the commit before the encoder was split"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_jpeg_encoder_fixture", os.path.join(ROOT, "tools", "make_jpeg_encoder_fixture.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    z = np.load(FIXTURE)
    names, dig, sizes = tool.digests(sdm)
    assert len(names) == len(z["name"]) == 6 + 4 * 3 * 4
    assert names == [str(n) for n in z["name"]]
    bad = [n for n, a, b in zip(names, dig, z["sha256"]) if a != str(b)]
    assert not bad, bad
    assert sizes == [int(v) for v in z["size"]]


@pytest.mark.parametrize("size", [(1, 1), (7, 9), (8, 8), (9, 3), (24, 16), (65, 17), (257, 8), (640, 480)])
def test_two_stages_give_the_encoders_bytes(sdm, size):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    for kind in ("smooth", "noise", "edges"):
        rgb = image(w, h, kind, rng)
        rgbx = np.concatenate([rgb, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], 2)
        for q in ((1, 50, 90, 100) if w < 640 else (90,)):
            coef = sdm.jpeg_forward_host(rgb, q)
            assert sdm.jpeg_entropy_encode(coef, w, h, q) == sdm.encode_jpeg_rgb(rgb, q), (kind, q)
            assert sdm.jpeg_forward_host(rgbx, q).tobytes() == coef.tobytes(), "stride 4 with a random X byte: %s q%d" % (kind, q)


def test_stage_arguments_are_checked(sdm):
    from bundlefusion_amd.capi import BFError
    rgb = np.zeros((8, 8, 3), np.uint8)
    coef = np.zeros(192, np.int16)
    lib = sdm.lib
    assert lib.bf_jpeg_forward_host(rgb.ctypes.data, 3, 8, 8, 90, coef.ctypes.data, 191) != 0            # capacity
    assert lib.bf_jpeg_forward_host(rgb.ctypes.data, 2, 8, 8, 90, coef.ctypes.data, 192) != 0            # stride
    assert lib.bf_jpeg_forward_host(rgb.ctypes.data, 3, 65536, 1, 90, coef.ctypes.data, 1 << 40) != 0
    n = C.c_uint64()
    assert lib.bf_jpeg_entropy_encode(8, 8, 90, coef.ctypes.data, None, 0, C.byref(n)) == 0 and n.value > 0
    small = np.zeros(4, np.uint8)
    assert lib.bf_jpeg_entropy_encode(8, 8, 90, coef.ctypes.data, small.ctypes.data, 4, C.byref(n)) != 0
    with pytest.raises(BFError):
        sdm.check(lib.bf_jpeg_entropy_encode(0, 8, 90, coef.ctypes.data, None, 0, C.byref(n)))


# ------------------------------------------------------------------------------------------------ 3: the back end alone
@pytest.fixture(scope="module")
def case(sdm, tmp_path_factory):
    d = tmp_path_factory.mktemp("record_host_route")
    fr, T = rc.frames(), rc.trajectory()
    return fr, T, rc.host_route(sdm, d / "host.sens", d / "host.tmp.sens", fr, T)


def _record(sdm, d, frames, T, threads, slots, name="out.sens", overwrite=False):
    rec = sdm.SensRecorder(None, rc.header(sdm), d / ("tmp_%d_%d.sens" % (threads, slots)), threads, slots)
    try:
        for depth, rgbx in frames:
            rec.record(depth, rgbx)
        assert rec.num_recorded() == len(frames)
        return rec.finish(d / name, T, overwrite), rec
    finally:
        rec.close()


@pytest.mark.parametrize("threads,slots", [(1, 2), (4, 2), (12, 7)])
def test_back_end_writes_the_host_routes_file(sdm, case, tmp_path, threads, slots):
    frames, T, want = case
    (name, n), _ = _record(sdm, tmp_path, frames, T, threads, slots)
    assert n == rc.NUM_TRANSFORMS and name == str(tmp_path / "out.sens")
    got = open(name, "rb").read()
    assert len(got) == len(want) and got == want, "threads %d slots %d: the file differs from the host route's" % (threads, slots)
    assert not os.path.exists(tmp_path / ("tmp_%d_%d.sens" % (threads, slots))), "the temporary file is left behind"
    sd = sdm.SensorData(name, use_pillow=False)
    assert len(sd) == rc.NUM_TRANSFORMS and np.all(np.isneginf(sd.pose(7)[0])) and np.array_equal(sd.pose(3)[0], T[3])
    assert np.array_equal(sd.depth_raw(5), sdm.record_depth_rule(frames[5][0]))
    sd.close()


def test_more_transforms_than_frames_is_the_references_error(sdm, case, tmp_path):
    from bundlefusion_amd.capi import BFError
    frames, _, _ = case
    with pytest.raises(BFError, match="more transforms than frames"):
        _record(sdm, tmp_path, frames, rc.trajectory(38), 4, 3)
    assert not os.path.exists(tmp_path / "out.sens") and not os.path.exists(tmp_path / "tmp_4_3.sens")


def test_an_existing_name_gets_the_numeric_suffix(sdm, case, tmp_path):
    frames, T, want = case
    (tmp_path / "out.sens").write_bytes(b"taken")
    (tmp_path / "out1.sens").write_bytes(b"taken too")
    (name, n), _ = _record(sdm, tmp_path, frames[:12], T[:10], 2, 2)
    assert name == str(tmp_path / "out2.sens") and n == 10
    assert (tmp_path / "out.sens").read_bytes() == b"taken" and (tmp_path / "out1.sens").read_bytes() == b"taken too"
    (name, n), _ = _record(sdm, tmp_path, frames, T, 2, 2, overwrite=True)
    assert name == str(tmp_path / "out.sens") and open(name, "rb").read() == want


def test_destroy_without_finish_leaves_no_temporary_file(sdm, case, tmp_path):
    frames, _, _ = case
    rec = sdm.SensRecorder(None, rc.header(sdm), tmp_path / "t.sens", 3, 2)
    for depth, rgbx in frames[:9]:
        rec.record(depth, rgbx)
    rec.close()
    assert os.listdir(tmp_path) == []


def test_recorder_starts_over_after_finish_and_checks_its_arguments(sdm, case, tmp_path):
    from bundlefusion_amd.capi import BFError
    frames, T, want = case
    rec = sdm.SensRecorder(None, rc.header(sdm), tmp_path / "t.sens", 2, 3)
    assert rec.finish(tmp_path / "none.sens", T) == ("", 0) and not os.path.exists(tmp_path / "none.sens")        # nothing recorded: no file
    for depth, rgbx in frames:
        rec.record(depth, rgbx)
    assert rec.finish(tmp_path / "a.sens", T)[1] == rc.NUM_TRANSFORMS
    assert rec.finish(tmp_path / "b.sens", T) == ("", 0) and not os.path.exists(tmp_path / "b.sens")              # a second finish without new frames
    for depth, rgbx in frames:
        rec.record(depth, rgbx)
    assert rec.finish(tmp_path / "c.sens", T)[1] == rc.NUM_TRANSFORMS
    assert (tmp_path / "a.sens").read_bytes() == want and (tmp_path / "c.sens").read_bytes() == want
    with pytest.raises(BFError):                                                      # device frames need a recorder created over a pipeline
        sdm.check(sdm.lib.bf_sens_recorder_record_device(rec._h, 16, 16, None))
    rec.close()
    for threads, slots in ((13, 0), (1, 1)):
        with pytest.raises(BFError):
            sdm.SensRecorder(None, rc.header(sdm), tmp_path / "bad.sens", threads, slots)
    raw = rc.header(sdm); raw.colorCompressionType = sdm.COLOR_RAW
    with pytest.raises(BFError):
        sdm.SensRecorder(None, raw, tmp_path / "bad.sens")
    with pytest.raises(BFError):
        sdm.SensRecorder(None, rc.header(sdm), tmp_path / "no such directory" / "t.sens")


def test_raw_depth_recording(sdm, case, tmp_path):
    frames, T, _ = case
    info = rc.header(sdm); info.depthCompressionType = sdm.DEPTH_RAW_USHORT
    want = rc.host_route(sdm, tmp_path / "host.sens", tmp_path / "host.tmp.sens", frames[:9], T[:9], info)
    rec = sdm.SensRecorder(None, info, tmp_path / "t.sens", 3, 2)
    for depth, rgbx in frames[:9]:
        rec.record(depth, rgbx)
    name, n = rec.finish(tmp_path / "raw.sens", T[:9])
    rec.close()
    assert n == 9 and open(name, "rb").read() == want


# ------------------------------------------------------------------------------------------------ 4: parameters and exports
RECORD_KEYS = '''
s_sensorIdx = 8;
s_recordData = false;           // master flag of the recording
s_recordCompression = true;     // .sens instead of .sensor
s_recordDataWidth = 640;
s_recordDataHeight = 480;
s_recordDataFile = "dump/recording.sens";
'''


def test_record_state_reader(built, tmp_path):
    from bundlefusion_amd.capi import RecordState, default_record_state, GlobalAppState, lib
    f = tmp_path / "zParametersDefault.txt"
    f.write_text(RECORD_KEYS)
    g, missing = default_record_state(f, with_missing=True)
    assert missing == 0
    ref = default_record_state()
    assert bytes(g) == bytes(ref)
    assert (ref.s_recordData, ref.s_recordCompression, ref.s_recordDataWidth, ref.s_recordDataHeight, ref.s_recordDataFile) == (0, 1, 640, 480, b"dump/recording.sens")
    other = tmp_path / "other.txt"
    other.write_text('s_recordData = true;\ns_recordCompression = false;\ns_recordDataWidth = 320;\ns_recordDataHeight = 240;\ns_recordDataFile = "my scans/a b.sens"; // with blanks\n')
    g, missing = default_record_state(other, with_missing=True)
    assert missing == 0 and (g.s_recordData, g.s_recordCompression, g.s_recordDataWidth, g.s_recordDataHeight, g.s_recordDataFile) == (1, 0, 320, 240, b"my scans/a b.sens")
    bare = tmp_path / "bare.txt"
    bare.write_text("s_sensorIdx = 8;\n")
    g, missing = default_record_state(bare, with_missing=True)
    assert missing == len(RecordState._fields_) == 5 and bytes(g) == bytes(ref)
    # the app state keeps ignoring the keys
    a, b = GlobalAppState(), GlobalAppState()
    na, nb = C.c_uint32(), C.c_uint32()
    assert lib.bf_global_app_state_read(str(f).encode(), C.byref(a), C.byref(na)) == 0 and lib.bf_global_app_state_read(str(bare).encode(), C.byref(b), C.byref(nb)) == 0
    assert bytes(a) == bytes(b) and na.value == nb.value


def test_library_exports_every_symbol_of_bf_record_h(built):
    """the rule of tests/test_render_cpp.py applied to bf_record.h, and to the entries this feature adds to the other headers"""
    txt = open(os.path.join(ROOT, "include", "bf_record.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"BF_API\s+[\w\s\*]+?\b(bf_\w+)\s*\(", txt)))
    assert len(names) == 10 and "bf_pipeline_save_recording" in names and "bf_sens_recorder_record_device" in names
    names += ["bf_jpeg_forward_host", "bf_jpeg_entropy_encode", "bf_sensor_data_writer_add_frame_compressed", "bf_image_convert_depth_to_u16", "bf_jpeg_forward_device"]
    lib = C.CDLL(os.path.join(LIBDIR, "libbf_hip.so"))
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    declared = txt + "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("bf_sensordata.h", "bf_hip.h"))
    assert all(re.search(r"BF_API\s+int\s+%s\s*\(" % n, declared) for n in names)


# ------------------------------------------------------------------------------------------------ 5: the depth round trip
def test_depth_rule_returns_every_u16_of_a_played_file(sdm):
    """u16 / 1000 (what bf_sensor_data_read_depth hands to the loop, 0 -> -inf) goes back to the same u16 under the recording's rule: all 65 536 values.
    This is why a played file's recording may be held to the source's raw depth with equality."""
    raw = np.arange(65536, dtype=np.uint16)
    metres = (raw.astype(np.float32) / np.float32(1000.0)).astype(np.float32)
    metres[0] = -np.inf
    back = sdm.record_depth_rule(metres, 1000.0)
    assert back.dtype == np.uint16 and int(np.count_nonzero(back != raw)) == 0
    # and the rule's edges
    edge = np.array([-np.inf, np.inf, np.nan, 0.0, -0.0, -1.0, 1e-7, 65.5354, 65.5355, 65.536, 1e9, 0.0004, 0.0005], np.float32)
    want = np.array([0, 0, 0, 0, 0, 0, 0, 65535, 0, 0, 0, 0, 1], np.uint16)
    v = (edge * np.float32(1000.0)).astype(np.float32)
    assert v[8] >= np.float32(65535.5) and v[7] < np.float32(65535.5) and v[12] + np.float32(0.5) >= 1
    assert np.array_equal(sdm.record_depth_rule(edge, 1000.0), want)
