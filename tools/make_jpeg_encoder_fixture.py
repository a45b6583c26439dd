#!/usr/bin/env python3
"""Write tests/golden/jpeg_encoder_parent.npz: SHA-256 digests of bf_encode_jpeg_rgb's streams, taken BEFORE the encoder was split into
bf_jpeg_forward_host + bf_jpeg_entropy_encode (run on the commit before the split; tests/test_record_cpu.py holds the split encoder to them).

  * the six images of tests/sensor_ingest_streams.py::encoded_streams (their own qualities);
  * sizes 1x1, 7x9, 8x8 and 65x17, kinds smooth / noise / edges, each at quality 1, 50, 90 and 100.
The file holds names, sizes and digests only.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_encoder_parent.npz")
SIZES = ((1, 1), (7, 9), (8, 8), (65, 17))
KINDS = ("smooth", "noise", "edges")
QUALITIES = (1, 50, 90, 100)


def small_cases():
    """[(name, rgb, quality)]: deterministic - one generator per case, seeded by the case"""
    from tests.sensor_ingest_streams import image
    out = []
    for w, h in SIZES:
        for k, kind in enumerate(KINDS):
            for q in QUALITIES:
                rng = np.random.default_rng(1000 * w + 10 * h + k)
                out.append(("%dx%d_%s_q%d" % (w, h, kind, q), image(w, h, kind, rng), q))
    return out


def digests(sdm):
    """-> (names, sha256 hex digests, stream sizes)"""
    from tests.sensor_ingest_streams import encoded_streams
    names, dig, sizes = [], [], []
    for i, (blob, w, h) in enumerate(encoded_streams(sdm)):
        names.append("encoded_streams_%d_%dx%d" % (i, w, h)); dig.append(hashlib.sha256(blob).hexdigest()); sizes.append(len(blob))
    for name, rgb, q in small_cases():
        blob = sdm.encode_jpeg_rgb(rgb, q)
        names.append(name); dig.append(hashlib.sha256(blob).hexdigest()); sizes.append(len(blob))
    return names, dig, sizes


def main():
    from bundlefusion_amd import sensordata as sdm
    names, dig, sizes = digests(sdm)
    np.savez_compressed(OUT, name=np.array(names), sha256=np.array(dig), size=np.array(sizes, np.int64))
    print("%s: %d digests, %d bytes" % (OUT, len(names), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
