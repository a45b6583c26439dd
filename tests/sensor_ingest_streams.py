"""Shared inputs of tests/test_sensor_ingest_cpu.py and tests/test_sensor_ingest_gpu.py: the JPEG streams of tests/golden/sensor_ingest_jpeg.npz
(written by tools/make_jpeg_fixture.py), streams of the library's own encoder, and a stream in a layout the device declines."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sensor_ingest_jpeg.npz")
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def fixture_streams():
    """[(blob, width, height, layout, quality, restart, kind)] - layout 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0, 3 = grey"""
    z = np.load(FIXTURE)
    data, off = z["data"].tobytes(), z["offset"]
    return [(data[off[i]:off[i + 1]],) + tuple(int(v) for v in m) for i, m in enumerate(z["meta"])]


def image(w, h, kind, rng):          # tests/test_sensordata_cpu.py::_test_image
    if kind == "smooth":
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([127 + 100 * np.sin(x / 17.0 + y / 29.0), 127 + 90 * np.cos(x / 11.0), 100 + 80 * np.sin(y / 7.0)], -1)
        return np.clip(a, 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a = np.zeros((h, w, 3), np.uint8)
    a[:, w // 2:] = [255, 0, 0]; a[h // 3:, : w // 3] = [0, 0, 255]; a[::7] = [0, 255, 0]
    return a


def encoded_streams(sdm):
    """streams of the library's own encoder (4:4:4, image-optimised Huffman tables): [(blob, width, height)]"""
    rng = np.random.default_rng(5)
    out = []
    for (w, h), kind, q in (((640, 480), "smooth", 92), ((640, 480), "noise", 92), ((1296, 968), "edges", 92), ((1296, 968), "smooth", 50), ((9, 3), "noise", 100), ((24, 16), "edges", 1)):
        out.append((sdm.encode_jpeg_rgb(image(w, h, kind, rng), q), w, h))
    return out



def vertical_only_stream():
    """A baseline stream whose chroma is sub-sampled vertically only (luma 1x2): no common encoder writes one, so a 4:2:2 stream of the fixture (luma 2x1, MCU = two
    luma blocks + Cb + Cr) is re-labelled - sampling factor 1x2 and a size with the same number of MCUs.  The scan is valid for the new layout (the picture is not
    the original's, which does not matter).  -> (blob, width, height)"""
    blob, w, h = next((s[0], s[1], s[2]) for s in fixture_streams() if s[1:4] == (37, 29, 1) and s[5] == 0)
    mcus_x, mcus_y = -(-w // 16), -(-h // 8)
    sof = blob.index(b"\xff\xc0")
    b = bytearray(blob)
    assert b[sof + 9] == 3 and b[sof + 11] == 0x21
    nw, nh = 8 * mcus_x, 16 * mcus_y
    b[sof + 5:sof + 9] = bytes([nh >> 8, nh & 255, nw >> 8, nw & 255])
    b[sof + 11] = 0x12
    return bytes(b), nw, nh
