"""Writes tests/golden/sensor_ingest_jpeg.npz: the baseline JPEG streams of tests/test_sensor_ingest_cpu.py / _gpu.py.

Needs Pillow (libjpeg) - the tests that read the file do not.  Streams: sizes 1x1 ... 641x481, 4:4:4 / 4:2:2 / 4:2:0 / greyscale,
qualities 1 / 50 / 92 / 100, with and without restart markers, image kinds smooth / noise / edges.  Up to 37x29 the full product; the
larger sizes take a covering part of it so that the file stays well below 1 MB.

The file holds `data` (all streams back to back), `offset` (n + 1 positions) and `meta` (n rows: width, height, layout 0 = 4:4:4 /
1 = 4:2:2 / 2 = 4:2:0 / 3 = grey, quality, restart interval in MCUs, kind 0 = smooth / 1 = noise / 2 = edges).
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("smooth", "noise", "edges")
LAYOUTS = (0, 1, 2, 3)
QUALITIES = (1, 50, 92, 100)


def test_image(w, h, kind, rng):          # tests/test_sensordata_cpu.py::_test_image
    if kind == "smooth":
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([127 + 100 * np.sin(x / 17.0 + y / 29.0), 127 + 90 * np.cos(x / 11.0), 100 + 80 * np.sin(y / 7.0)], -1)
        return np.clip(a, 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a = np.zeros((h, w, 3), np.uint8)
    a[:, w // 2:] = [255, 0, 0]; a[h // 3:, : w // 3] = [0, 0, 255]; a[::7] = [0, 255, 0]
    return a


def encode(img, layout, quality, restart):
    im = Image.fromarray(img)
    kw = {"restart_marker_blocks": restart} if restart else {}
    buf = io.BytesIO()
    if layout == 3:
        im.convert("L").save(buf, format="JPEG", quality=quality, **kw)
    else:
        im.save(buf, format="JPEG", quality=quality, subsampling=layout, **kw)
    return buf.getvalue()


def cases():
    for (w, h) in ((1, 1), (8, 8), (17, 9), (37, 29)):
        for layout in LAYOUTS:
            for q in QUALITIES:
                for restart in (0, 3):
                    for kind in range(3):
                        yield w, h, layout, q, restart, kind
    n = 0
    for layout in LAYOUTS:
        for q in QUALITIES:
            for kind in range(3):
                n += 1
                yield 64, 48, layout, q, (0, 5)[n % 2], kind
    for layout in LAYOUTS:
        for k, (q, kind) in enumerate(((50, 0), (92, 2), (1, 1))):
            yield 320, 240, layout, q, (0, 7)[(k + layout) % 2], kind
    for layout in LAYOUTS:
        for k, (q, kind) in enumerate(((92, 0), (1, 1))):
            yield 641, 481, layout, q, (0, 11)[(k + layout) % 2], kind
    yield 641, 481, 2, 50, 11, 2


def main():
    rng = np.random.default_rng(20)
    blobs, meta = [], []
    for w, h, layout, q, restart, kind in cases():
        blobs.append(encode(test_image(w, h, KINDS[kind], rng), layout, q, restart))
        meta.append((w, h, layout, q, restart, kind))
    offset = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    out = os.path.join(ROOT, "tests", "golden", "sensor_ingest_jpeg.npz")
    np.savez_compressed(out, data=np.frombuffer(b"".join(blobs), np.uint8), offset=offset, meta=np.array(meta, np.int32))
    print("%d streams, %d bytes of JPEG, file %d bytes" % (len(blobs), offset[-1], os.path.getsize(out)), file=sys.stderr)


if __name__ == "__main__":
    main()
