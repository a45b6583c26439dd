"""CPU tests (-m "not gpu") of the host half of the sensor-format ingest: the JPEG decoder in its stages (bf_jpeg_parse, bf_jpeg_entropy_decode,
bf_jpeg_reconstruct_host) against the one-pass bf_decode_color_rgb, the layout of the coefficient buffer, and the decode-ahead player's workers
(bf_sens_player over a null pipeline).  Tolerance: none - images and slots are compared as bytes.

JPEG streams: tests/golden/sensor_ingest_jpeg.npz (written by tools/make_jpeg_fixture.py with Pillow; not needed here) plus streams made at
test time by bf_encode_jpeg_rgb, among them 640x480 and 1296x968.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests.sensor_ingest_streams import FIXTURE, ZIGZAG, encoded_streams, fixture_streams, image as _image


def test_fixture_covers_what_it_promises():
    s = fixture_streams()
    meta = np.array([m[1:] for m in s])
    assert {(1, 1), (8, 8), (17, 9), (37, 29), (64, 48), (320, 240), (641, 481)} == set(map(tuple, meta[:, :2]))
    for size in set(map(tuple, meta[:, :2])):
        assert set(meta[(meta[:, 0] == size[0]) & (meta[:, 1] == size[1]), 2]) == {0, 1, 2, 3}, size          # every layout at every size
    assert set(meta[:, 3]) == {1, 50, 92, 100} and set(meta[:, 5]) == {0, 1, 2} and {0} < set(meta[:, 4])
    combos = {(int(m[2]), int(m[3]), int(m[4] > 0), int(m[5])) for m in meta}
    assert combos == {(l, q, r, k) for l in range(4) for q in (1, 50, 92, 100) for r in (0, 1) for k in range(3)}
    assert os.path.getsize(FIXTURE) < 700 << 10


def test_stages_equal_the_one_pass_decoder(built):
    """parse + entropy decode + host reconstruction == bf_decode_color_rgb, on every fixture stream and on the encoder's streams"""
    from bundlefusion_amd import sensordata as sdm
    streams = [(s[0], s[1], s[2]) for s in fixture_streams()] + encoded_streams(sdm)
    assert len(streams) > 400
    for n, (blob, w, h) in enumerate(streams):
        ref = sdm.decode_color_rgb(blob, sdm.COLOR_JPEG, w, h)
        info = sdm.jpeg_parse(blob, w, h)
        coef = sdm.jpeg_entropy_decode(blob, info)
        assert coef is not None, n
        assert np.array_equal(sdm.jpeg_reconstruct_host(info, coef), ref), (n, w, h)
        assert np.array_equal(sdm.jpeg_reconstruct_host(sdm.jpeg_parse(blob), coef), ref)       # no expected size: the stream's own


def test_description_and_coefficient_layout(built):
    """The POD description and the documented buffer: numBlocks * 64 int16, components one after the other, raster order inside a component's
    block grid (padded to whole MCUs), natural order inside a block, quantised.  Checked on a stream whose coefficients are known: the
    library's encoder stores what it quantised, and a block of a constant image has only a DC term."""
    from bundlefusion_amd import sensordata as sdm
    layouts = {0: ((1, 1), (1, 1), (1, 1)), 1: ((2, 1), (1, 1), (1, 1)), 2: ((2, 2), (1, 1), (1, 1)), 3: ((1, 1),)}
    seen = set()
    for blob, w, h, layout, q, restart, kind in fixture_streams():
        info = sdm.jpeg_parse(blob, w, h)
        samp = layouts[layout]
        assert (info.width, info.height, info.numComponents, info.restartInterval) == (w, h, len(samp), restart)
        hmax, vmax = samp[0]
        assert (info.hmax, info.vmax) == (hmax, vmax) and info.mcusX == -(-w // (8 * hmax)) and info.mcusY == -(-h // (8 * vmax))
        blocks = 0
        for ci, (ch, cv) in enumerate(samp):
            c = info.comp[ci]
            assert (c.h, c.v, c.blocksX, c.blocksY, c.blockOffset, c.planeOffset) == (ch, cv, info.mcusX * ch, info.mcusY * cv, blocks, blocks * 64)
            assert info.qtPresent[c.tq]
            blocks += c.blocksX * c.blocksY
        assert info.numBlocks == blocks and info.planeBytes == blocks * 64
        coef = sdm.jpeg_entropy_decode(blob, info)
        assert coef.shape == (blocks, 64) and coef.dtype == np.int16
        if q == 100:
            assert all(v == 1 for ci in range(len(samp)) for v in info.qt[info.comp[ci].tq])        # libjpeg at quality 100: every step is 1
        seen.add((layout, restart > 0))
    assert len(seen) == 8
    # block order and natural order: an image that is constant inside every 8x8 block, with another level per block -> DC = 8 * (level - 128) / q[0] and
    # no AC; a horizontal ramp inside one block puts its energy into the first ROW of that block (natural index 1, zigzag index 1 too) and a vertical
    # ramp into the first COLUMN (natural index 8, zigzag index 2)
    bw, bh = 5, 3
    level = (np.arange(bw * bh).reshape(bh, bw) * 11 + 30).astype(np.uint8)
    img = np.repeat(np.repeat(level, 8, axis=0), 8, axis=1)
    rgb = np.stack([img] * 3, -1).copy()
    rgb[8:16, 16:24] += (np.arange(8) * 6).astype(np.uint8)[None, :, None]          # block (bx 2, by 1): horizontal ramp
    rgb[16:24, 0:8] += (np.arange(8) * 6).astype(np.uint8)[:, None, None]           # block (bx 0, by 2): vertical ramp
    rgb = rgb[:, :37]                                                               # 37 wide: the last block column is padding past the image
    blob = sdm.encode_jpeg_rgb(rgb, 100)
    info = sdm.jpeg_parse(blob, 37, 24)
    coef = sdm.jpeg_entropy_decode(blob, info)
    assert (info.comp[0].blocksX, info.comp[0].blocksY, info.numBlocks) == (5, 3, 45) and coef.shape == (45, 64)
    luma = coef[:15].reshape(3, 5, 64)
    assert all(v == 1 for v in info.qt[info.comp[0].tq])
    for by in range(bh):
        for bx in range(bw):
            if (bx, by) in ((2, 1), (0, 2)):
                continue
            assert abs(int(luma[by, bx, 0]) - 8 * (int(level[by, bx]) - 128)) <= 1, (bx, by)      # raster order of the block grid
            assert not luma[by, bx, 1:].any()
    assert abs(luma[1, 2, 1]) > 20 and luma[1, 2, 8] == 0 and abs(luma[2, 0, 8]) > 20 and luma[2, 0, 1] == 0      # natural order, not zigzag (ZIGZAG[2] == 8)
    assert ZIGZAG[2] == 8
    assert not coef[15:, 1:].any() and np.abs(coef[15:, 0]).max() <= 1              # grey image: chroma blocks (components 1 and 2) are empty


def test_entropy_stage_rejects_what_the_decoder_rejects(built):
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    from bundlefusion_amd import sensordata as sdm
    from bundlefusion_amd.capi import BFError
    rng = np.random.default_rng(3)
    img = _image(64, 48, "smooth", rng)
    buf = io.BytesIO(); Image.fromarray(img).save(buf, format="JPEG", progressive=True)
    prog = buf.getvalue()
    for fn in (lambda b: sdm.decode_color_rgb(b, sdm.COLOR_JPEG, 64, 48), lambda b: sdm.jpeg_parse(b, 64, 48)):
        with pytest.raises(BFError, match="progressive"):
            fn(prog)
    base = prog.replace(b"\xff\xc2", b"\xff\xc0", 1)
    for fn in (lambda b: sdm.decode_color_rgb(b, sdm.COLOR_JPEG, 32, 48), lambda b: sdm.jpeg_parse(b, 32, 48)):
        with pytest.raises(BFError, match="expected"):
            fn(base)
    buf = io.BytesIO(); Image.fromarray(img).save(buf, format="JPEG", quality=92)
    good = buf.getvalue()
    info = sdm.jpeg_parse(good, 64, 48)
    other = sdm.jpeg_parse(sdm.encode_jpeg_rgb(img, 92), 64, 48)
    with pytest.raises(BFError, match="does not belong"):                      # a description of another stream
        sdm.jpeg_entropy_decode(good, other)
    sos = good.index(b"\xff\xda")
    for cut in (sos - 7, sos + 5, 40, 3):                                       # inside a header segment: both refuse, with the same message
        msgs = []
        for fn in (lambda b: sdm.decode_color_rgb(b, sdm.COLOR_JPEG, 64, 48), lambda b: sdm.jpeg_parse(b, 64, 48)):
            with pytest.raises(BFError) as e:
                fn(good[:cut])
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], cut
    for cut in (sos + 40, len(good) // 2, len(good) - 3):                       # inside the scan: whatever the one-pass decoder does, the stages do
        part = good[:cut]
        try:
            ref = sdm.decode_color_rgb(part, sdm.COLOR_JPEG, 64, 48)
        except BFError as e:
            with pytest.raises(BFError) as e2:
                sdm.jpeg_entropy_decode(part, sdm.jpeg_parse(part, 64, 48))
            assert str(e2.value) == str(e)
        else:
            pinfo = sdm.jpeg_parse(part, 64, 48)
            assert np.array_equal(sdm.jpeg_reconstruct_host(pinfo, sdm.jpeg_entropy_decode(part, pinfo)), ref)
    rng2 = np.random.default_rng(9)
    refused = 0
    for it in range(40):                                                       # corrupt scans: same verdict, same message or same image
        b = bytearray(good)
        if it % 2:                                                             # a run of one bits (stuffed FF 00): no Huffman code is all ones
            p = int(rng2.integers(sos + 14, len(good) - 40))
            b[p:p + 16] = b"\xff\x00" * 8
        else:
            for p in rng2.integers(sos + 14, len(good) - 2, 6):
                b[p] = int(rng2.integers(0, 255))
        b = bytes(b)
        pinfo = sdm.jpeg_parse(b, 64, 48)
        try:
            ref = sdm.decode_color_rgb(b, sdm.COLOR_JPEG, 64, 48)
        except BFError as e:
            refused += 1
            with pytest.raises(BFError) as e2:
                sdm.jpeg_entropy_decode(b, pinfo)
            assert str(e2.value) == str(e)
        else:
            coef = sdm.jpeg_entropy_decode(b, pinfo)
            if coef is not None:                                               # (None: DC beyond int16 - the documented hand-back to the host decoder)
                assert np.array_equal(sdm.jpeg_reconstruct_host(pinfo, coef), ref)
    assert refused > 0


def test_device_entries_fail_loudly_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bundlefusion_amd import sensordata as sdm
    from bundlefusion_amd.capi import lib, default_app_state, default_bundling_state, sensor_desc, intrinsics_matrix
    one = np.zeros(64, np.uint8)
    p = one.ctypes.data_as(C.c_void_p)
    for call in (lambda: lib.bf_image_convert_depth_u16(p, p, C.c_float(1000.0), 8, None),
                 lambda: lib.bf_image_convert_rgb8_to_rgbx(p, p, 8, None)):
        assert call() != 0 and lib.bf_last_error()                             # no silent CPU fallback
    blob = sdm.encode_jpeg_rgb(np.zeros((8, 8, 3), np.uint8), 90)
    info = sdm.jpeg_parse(blob)
    assert lib.bf_jpeg_reconstruct_device(C.byref(info), p, p, p, None) != 0 and lib.bf_last_error()
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = 16, 12
    h = C.c_void_p()
    rc = lib.bf_image_manager_create(16, 12, 16, 12, C.byref(sensor_desc(16, 12, intrinsics_matrix(20, 20, 8, 6))), C.byref(gbs), 1, C.byref(h))
    assert rc != 0 and lib.bf_last_error()
    h = C.c_void_p()
    assert lib.bf_pipeline_create(C.byref(gas), C.byref(gbs), C.byref(sensor_desc(16, 12, intrinsics_matrix(20, 20, 8, 6))), C.byref(h)) != 0 and lib.bf_last_error()


def _write_sens(sdm, path, frames, size, color_compression, corrupt=None):
    """frames: [(depth u16, colour bytes)]; corrupt: index of a frame whose colour stream is damaged inside its headers"""
    w, h = size
    K = np.eye(4, dtype=np.float32); K[0, 0] = K[1, 1] = 50; K[0, 2] = w / 2; K[1, 2] = h / 2
    with sdm.SensorDataWriter(path, (w, h), (w, h), K, color_compression=color_compression) as wr:
        for i, (d, c) in enumerate(frames):
            if i == corrupt:
                c = c[:2] + b"\xff\xc2" + c[4:]                                  # an SOF2 marker where APP0 was: "progressive"
            wr.add_frame(np.eye(4, dtype=np.float32), d, c)


@pytest.mark.parametrize("compression", ["jpeg", "raw"])
def test_player_workers_deliver_frames_in_order(built, tmp_path, compression):
    """bf_sens_player over a null pipeline: frames leave in order with the same bytes for 1, 4 and 12 threads - the file's u16 depth and the
    entropy-decoded colour (JPEG) or the stored RGB8 (raw) - and more frames than slots pass through the ring."""
    from bundlefusion_amd import sensordata as sdm
    rng = np.random.default_rng(11)
    w, h, n = 40, 24, 31
    frames, want = [], []
    for i in range(n):
        d = rng.integers(0, 5000, (h, w)).astype(np.uint16)
        rgb = _image(w, h, ("smooth", "noise", "edges")[i % 3], rng)
        rgb[0, 0] = i
        blob = sdm.encode_jpeg_rgb(rgb, 92) if compression == "jpeg" else rgb.tobytes()
        frames.append((d, blob))
        want.append((d, sdm.jpeg_entropy_decode(blob, sdm.jpeg_parse(blob, w, h)) if compression == "jpeg" else rgb))
    path = tmp_path / "p.sens"
    _write_sens(sdm, path, frames, (w, h), sdm.COLOR_JPEG if compression == "jpeg" else sdm.COLOR_RAW)
    for threads in (1, 4, 12):
        sd = sdm.SensorData(path, use_pillow=False)
        with sdm.SensPlayer(None, sd, threads) as pl:
            for i in range(n):
                frame, depth, colour, info = pl.peek()
                assert frame == i and np.array_equal(depth, want[i][0]), (threads, i)
                assert (info is not None) == (compression == "jpeg")
                assert colour.dtype == want[i][1].dtype and np.array_equal(colour, want[i][1]), (threads, i)
                if info is not None:
                    assert np.array_equal(sdm.jpeg_reconstruct_host(info, colour), sdm.decode_color_rgb(frames[i][1], sdm.COLOR_JPEG, w, h))
                assert pl.next() is True
            assert pl.peek() is None and pl.next() is False and pl.next() is False
        sd.close()


def test_player_reports_a_corrupt_frame_at_its_place(built, tmp_path):
    from bundlefusion_amd import sensordata as sdm
    from bundlefusion_amd.capi import BFError, lib
    rng = np.random.default_rng(12)
    w, h, n, k = 24, 16, 20, 13
    frames = [(rng.integers(1, 3000, (h, w)).astype(np.uint16), sdm.encode_jpeg_rgb(_image(w, h, "noise", rng), 80)) for _ in range(n)]
    path = tmp_path / "c.sens"
    _write_sens(sdm, path, frames, (w, h), sdm.COLOR_JPEG, corrupt=k)
    for threads in (1, 4, 12):
        sd = sdm.SensorData(path, use_pillow=False)
        with sdm.SensPlayer(None, sd, threads) as pl:
            for i in range(k):
                assert pl.next() is True, (threads, i)                         # not earlier
            with pytest.raises(BFError, match="progressive"):
                pl.next()                                                      # at frame k
            for i in range(k + 1, n):
                assert pl.peek()[0] == i and pl.next() is True                 # not later: the frames behind it are intact
            assert pl.next() is False
        sd.close()
    sd = sdm.SensorData(path, use_pillow=False)
    h_ = C.c_void_p()
    assert lib.bf_sens_player_create(None, sd._h, 13, C.byref(h_)) != 0 and b"12" in lib.bf_last_error()      # the cap on decode threads
    sd.close()
