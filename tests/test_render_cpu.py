"""CPU tests (-m "not gpu") of the frame renderer's host side and of its definition: the new fixed sequences of include/bf_detmath.h against their numpy
restatement (bits), the restatement against float64 + libm (one quantisation step), the render-state reader, the PNG writer, and the planted cases
themselves (tests/render_ref.py; the GPU tests compare the kernels with the same restatement)."""
import ctypes as C
import os
import struct
import subprocess
import textwrap
import zlib

import numpy as np
import pytest

from tests import render_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# the runs of the planted G-buffer: (state overrides, use_material, tracking_lost)
BRIGHT = dict(s_lightDiffuse=(2.5, 2.0, 1.5, 1.0))               # diffuse terms above 1: pow(., 1.2) on both sides of 1


def light_along_a_normal():
    """a light direction for which -L is the normal of the flat patch at 1.25 m exactly: (0, 0, 1) points away from the camera, the patch's normal is (0, 0, -1)"""
    return dict(s_lightDirection=(0.0, 0.0, 1.0))


RUNS = [(None, False, False), (None, True, False), (None, False, True), (None, True, True), (BRIGHT, True, False), (light_along_a_normal(), False, False),
        (light_along_a_normal(), True, False)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_detmath_log_pow_match_the_restatement_bit_for_bit(tmp_path):
    """(a) bf_dm_log / bf_dm_pow compiled for the host give the bits of tests/render_ref.py on a grid: x in 2^-24 .. 8 with 1, 0, denormals and the values next
    to the denormal boundary, y in {1.2, 16, 1, 128}; against libm the error stays in the class the header states."""
    src = tmp_path / "dm.c"
    src.write_text(textwrap.dedent(r'''
        #include "bf_detmath.h"
        void dm_eval(const float* x, int n, float y, float* lg, float* pw) { for (int i = 0; i < n; ++i) { lg[i] = bf_dm_log(x[i]); pw[i] = bf_dm_pow(x[i], y); } }
    '''))
    so = str(tmp_path / "dm.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", so])
    lib = C.CDLL(so)
    tiny = F(1.17549435e-38)
    special = np.array([0.0, 1.0, 2.0 ** -24, 8.0, 1e-45, 3e-42, 1.1754942e-38, tiny, np.nextafter(tiny, F(0)), np.nextafter(tiny, F(1)), np.nextafter(F(1), F(0)),
                        np.nextafter(F(1), F(2)), 1.41421356, np.nextafter(F(1.41421356), F(2)), 0.5, 0.70710678, 2.0, 4.0], np.float32)
    rng = np.random.default_rng(3)
    x = np.concatenate([special, np.exp2(rng.uniform(-24, 3, 40000)).astype(np.float32), np.linspace(2.0 ** -24, 8.0, 20000, dtype=np.float32),
                        rng.uniform(0, 1, 20000).astype(np.float32)])
    for y in (1.2, 16.0, 1.0, 128.0):
        lg, pw = np.zeros_like(x), np.zeros_like(x)
        lib.dm_eval(x.ctypes.data_as(C.c_void_p), len(x), C.c_float(y), lg.ctypes.data_as(C.c_void_p), pw.ctypes.data_as(C.c_void_p))
        assert np.array_equal(_bits(lg), _bits(rr.dm_log(x)))
        assert np.array_equal(_bits(pw), _bits(rr.dm_pow(x, y)))
        pos = x > 0
        assert lg[0] == -np.inf and pw[0] == 0.0
        xd = x[pos].astype(np.float64)
        assert np.max(np.abs(lg[pos] - np.log(xd)) / np.maximum(np.abs(np.log(xd)), 1e-3)) < 4e-7
        arg = np.float64(F(y)) * np.log(xd)
        inr = np.abs(arg) < 80
        rel = np.abs(pw[pos][inr] - np.exp(arg[inr])) / np.exp(arg[inr])
        assert np.max(rel - np.abs(arg[inr]) * 2.0 ** -22) < 1e-6, float(np.max(rel))


def test_restatement_agrees_with_float64_libm_within_one_step():
    """(b) the planted cases shaded by the restatement and again in float64 with libm: the RGBA8 pictures differ by at most 1 per channel - errors of a few
    ulp cannot move a value by more than one quantisation step of 1 / 255."""
    Kinv = rr.planted_kinv()
    for (w, h) in ((67, 9), (128, 8), (2, 2), (65, 5)):
        depth, colors = rr.planted_gbuffer(w, h)
        for state, mat, lost in RUNS:
            _, a, ia = rr.shade(depth, colors, Kinv, state, mat, lost)
            _, b, ib = rr.shade64(depth, colors, Kinv, state, mat, lost)
            assert np.array_equal(ia["drawn"], ib["drawn"])
            diff = np.abs(a.astype(np.int32) - b.astype(np.int32))
            assert diff[..., :3].max() <= 1, (w, h, mat, lost, int(diff.max()))
            # alpha follows from the quantised colour (255 iff one of r, g, b is above 0): it may differ only in a pixel whose brightest channel moved between 0 and 1
            moved = np.minimum(a[..., :3].max(-1), b[..., :3].max(-1)) == 0
            assert np.array_equal(a[..., 3][~moved], b[..., 3][~moved])


PARAMS = '''
    // 0=Kinect; 8=SensorDataReader (for offline processing)
    s_sensorIdx = 8;
    s_generateVideo = true;
    s_generateVideoDir = "video out/";   // a quoted string
    s_topVideoTransformWorld = 0.0f 1.0f 0.0f 0.5f -1.0f 0.0f 0.0f 0.25f 0.0f 0.0f 1.0f 2.0f 0.0f 0.0f 0.0f 1.0f;
    s_topVideoCameraPose = 90.0f 0.1f 0.2f -3.0f; //rotation (deg around z axis), translation (m)
    s_topVideoMinMax = 0.5f 7.5f;
    s_integrationWidth = 640;	//input depth gets re-sampled to this width
    s_materialShininess 	= 24.0f;
    s_materialAmbient   	= 0.1f 0.2f 0.3f 0.4f;
    s_materialDiffuse 		= 0.5f 0.6f 0.7f 0.8f;
    s_materialSpecular 		= 0.9f 1.0f 1.1f 1.2f;
    s_lightAmbient 			= 1.3f 1.4f 1.5f 1.6f;
    s_lightDiffuse 			= 1.7f 1.8f 1.9f 2.0f;
    s_lightSpecular 		= 2.1f 2.2f 2.3f 2.4f;
    s_lightDirection 		= 1.0f -2.0f 3.0f;
    s_RenderMode = 2;
    s_renderingDepthDiscontinuityThresOffset = 0.02f;  // discontinuity offset in meter
    s_renderingDepthDiscontinuityThresLin	 = 0.005f; // additional discontinuity threshold per meter
'''


def test_render_state_reader(built, tmp_path):
    """(c) the rendering keys are read, vectors included; a file without them gives the defaults with numMissing == the number of fields; what
    bf_global_app_state_read makes of the same text does not change"""
    from bundlefusion_amd.capi import lib, GlobalAppState, RenderState, default_render_state
    f = tmp_path / "zParametersDefault.txt"
    f.write_text(textwrap.dedent(PARAMS))
    g, missing = default_render_state(f, with_missing=True)
    assert missing == 0
    near = lambda a, b: np.allclose(np.array(list(a), np.float32), np.array(b, np.float32), rtol=0, atol=0)
    assert g.s_materialShininess == 24.0 and g.s_RenderMode == 2 and g.s_generateVideo == 1 and g.s_generateVideoDir == b"video out/"
    assert near(g.s_materialAmbient, (0.1, 0.2, 0.3, 0.4)) and near(g.s_materialDiffuse, (0.5, 0.6, 0.7, 0.8)) and near(g.s_materialSpecular, (0.9, 1.0, 1.1, 1.2))
    assert near(g.s_lightAmbient, (1.3, 1.4, 1.5, 1.6)) and near(g.s_lightDiffuse, (1.7, 1.8, 1.9, 2.0)) and near(g.s_lightSpecular, (2.1, 2.2, 2.3, 2.4))
    assert near(g.s_lightDirection, (1.0, -2.0, 3.0))
    assert g.s_renderingDepthDiscontinuityThresOffset == F(0.02) and g.s_renderingDepthDiscontinuityThresLin == F(0.005)
    assert near(g.s_topVideoTransformWorld, (0, 1, 0, 0.5, -1, 0, 0, 0.25, 0, 0, 1, 2, 0, 0, 0, 1)) and near(g.s_topVideoCameraPose, (90, 0.1, 0.2, -3)) and near(g.s_topVideoMinMax, (0.5, 7.5))
    # without the keys: the shipped file's values
    bare = tmp_path / "bare.txt"
    bare.write_text("s_sensorIdx = 8;\ns_integrationWidth = 640;\n")
    d, missing = default_render_state(bare, with_missing=True)
    assert missing == len(RenderState._fields_) == 16
    ref = default_render_state()
    assert bytes(d) == bytes(ref)
    assert ref.s_materialShininess == 16.0 and ref.s_RenderMode == 1 and ref.s_generateVideo == 0 and ref.s_generateVideoDir == b"output/"
    assert near(ref.s_lightDiffuse, (0.6, 0.52944, 0.4566, 0.6)) and near(ref.s_lightDirection, (0, -1, 2)) and near(ref.s_materialAmbient, (0.75, 0.65, 0.5, 1.0))
    assert ref.s_renderingDepthDiscontinuityThresOffset == F(0.012) and ref.s_renderingDepthDiscontinuityThresLin == F(0.001)
    assert near(ref.s_topVideoTransformWorld, np.eye(4).reshape(16)) and near(ref.s_topVideoCameraPose, (0, 0, 0, 0)) and near(ref.s_topVideoMinMax, (0, 0))
    assert set(rr.DEFAULT_STATE) <= {n for n, _ in RenderState._fields_}
    for k, v in rr.DEFAULT_STATE.items():
        got = getattr(ref, k)
        assert near(got, v) if hasattr(got, "__len__") else got == F(v)
    # the app state of the same two texts: the rendering keys stay unknown to it, and so does its count of missing fields
    a, b = GlobalAppState(), GlobalAppState()
    na, nb = C.c_uint32(), C.c_uint32()
    assert lib.bf_global_app_state_read(str(f).encode(), C.byref(a), C.byref(na)) == 0
    assert lib.bf_global_app_state_read(str(bare).encode(), C.byref(b), C.byref(nb)) == 0
    assert bytes(a) == bytes(b) and na.value == nb.value and a.s_sensorIdx == 8 and a.s_integrationWidth == 640


def _read_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    chunks, o = [], 8
    while o < len(raw):
        n, typ = struct.unpack(">I4s", raw[o:o + 8])
        data = raw[o + 8:o + 8 + n]
        crc, = struct.unpack(">I", raw[o + 8 + n:o + 12 + n])
        assert crc == (zlib.crc32(typ + data) & 0xFFFFFFFF), typ
        chunks.append((typ, data))
        o += 12 + n
    assert o == len(raw)
    return chunks


@pytest.mark.parametrize("size", [(1, 1), (3, 2), (640, 480)])
def test_png_writer(built, tmp_path, size):
    """(d) bf_write_png_rgba8 parsed with struct + zlib: signature, IHDR, every chunk's CRC, filter bytes, and the pixels back byte for byte; the largest
    picture is more than 65535 bytes, the limit of one stored deflate block"""
    from bundlefusion_amd.capi import write_png_rgba8
    w, h = size
    img = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 4), dtype=np.uint8)
    path = tmp_path / "a.png"
    write_png_rgba8(path, img)
    chunks = _read_png(path)
    assert [c[0] for c in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"") and all(c[0] == b"IDAT" for c in chunks[1:-1]) and len(chunks) >= 3
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (w, h, 8, 6, 0, 0, 0)
    d = zlib.decompressobj()
    raw = d.decompress(b"".join(c[1] for c in chunks[1:-1])) + d.flush()
    assert d.eof and d.unused_data == b"" and len(raw) == h * (w * 4 + 1)
    if size == (640, 480):
        assert len(raw) > 65535
    rows = np.frombuffer(raw, np.uint8).reshape(h, w * 4 + 1)
    assert (rows[:, 0] == 0).all()
    assert np.array_equal(rows[:, 1:].reshape(h, w, 4), img)


def test_planted_cases_are_not_vacuous():
    """(e) in the restatement alone: at least half of the main case's pixels are drawn, every rejection reason occurs, the threshold quads sit where they are
    meant to, and pow sees arguments on both sides of 1"""
    from tests.calibrator_ref import quad_survives
    Kinv = rr.planted_kinv()
    depth, colors = rr.planted_gbuffer()
    assert depth.shape == (9, 67)
    target, rgba, info = rr.shade(depth, colors, Kinv)
    assert info["drawn"].mean() >= 0.5
    for name, m in info["reasons"].items():
        assert m.any(), name
    assert info["reasons"]["degenerate"][4, 32] and info["reasons"]["nocolor"][5, 8]
    assert (target[~info["drawn"]] == -np.inf).all() and (rgba[~info["drawn"]] == 0).all()
    # the NaN colour: drawn; black in the coloured picture, canonical NaNs in its float target
    tm, rm, im = rr.shade(depth, colors, Kinv, None, True, False)
    assert im["drawn"][5, 16] and (rm[5, 16] == 0).all() and (tm[5, 16, :3].view(np.uint32) == rr.QNAN_BITS).all()
    # the two threshold quads
    dmin, dmax = rr.spread_at_threshold(0.012, 0.001)
    assert (dmax - dmin) == F(0.012) + F(0.001) * (F(0.5) * (dmax + dmin))
    q = quad_survives(depth, 0.012, 0.001)
    assert q[0:2, 24:26].all() and not q[0:2, 38:40].any()
    assert not q[3:6, 11:14].any() and q[3:5, 19:21].all()                        # depth exactly 0.1 / just above it
    # pow: arguments above and below 1 (the bright light), and the specular argument reaches its ends
    _, _, ib = rr.shade(depth, colors, Kinv, BRIGHT, True, False)
    pa = ib["pow_args"]
    assert (pa > 1).any() and ((pa > 0) & (pa < 1)).any() and (pa == 0).any()
    # the light along a normal: the flat patch's normal is (0, 0, -1) exactly and n . (-L) is 1 there
    ta, _, ia = rr.shade(depth, colors, Kinv, light_along_a_normal(), False, False)
    assert ia["drawn"][7, 59]
    # both branches and the overlay give different pictures
    _, r1, _ = rr.shade(depth, colors, Kinv, None, False, True)
    assert not np.array_equal(rgba, rm) and not np.array_equal(rgba, r1) and (r1[..., 0] == r1[..., 2]).all() and (r1[..., 1] == r1[..., 2]).all()
    # mode 4's planted depths hit every hue sector, both clamp ends and the += 359 branch
    d4, dmin4, dmax4 = planted_depth_hsv()
    t4, r4, i4 = rr.depth_hsv(d4, dmin4, dmax4)
    g = i4["gate"]
    assert g.any() and (~g).any() and set(np.unique(i4["h"][g]).tolist()) == {0, 1, 2, 3, 4, 5}
    assert (i4["hue"][g] >= 239).any() and (i4["hue"][g] < 239).any()
    for hue in (60, 120, 180, 240, 300):
        assert (i4["hue"][g] == hue).any(), hue
    # A hue of exactly 0 cannot occur in binary32: it needs 360 x == 120 after rounding, i.e. x = 1 - z within 1.06e-8 of 1/3, but z lies in [0.5, 1) there, so x
    # is a multiple of 2^-24 and the nearest one is 1.99e-8 away.  The planted depths therefore hold the smallest hue above 0 and its neighbour in the += 359 branch.
    assert ((i4["hue"][g] > 0) & (i4["hue"][g] < 1e-4)).any() and (i4["hue"][g] == 359).any()


def planted_depth_hsv(w=67, h=9):
    """mode 4's inputs: exactly min and max, one ulp outside each, 0, -inf, NaN, depths whose hue is exactly 0, 60, ..., 300, depths in the += 359 branch, and
    both ends of the clamp (which the gate makes min and max themselves)"""
    dmin, dmax = F(0.5), F(4.0)
    rng = np.random.default_rng(11)
    d = rng.uniform(0.3, 4.3, (h, w)).astype(np.float32)
    flat = d.reshape(-1)
    sp = [dmin, dmax, np.nextafter(dmin, F(0)), np.nextafter(dmax, F(9)), np.nextafter(dmin, F(9)), np.nextafter(dmax, F(0)), 0.0, -np.inf, np.nan, np.inf]
    # hue = 360 (1 - z) - 120 for z <= 2/3, and 360 (1 - z) + 239 beyond: z = (240 - hue) / 360 resp. (599 - hue) / 360; the floats around the real
    # solution are searched for those whose hue is the sector boundary exactly in binary32
    for hue, z in [(hh, (240 - hh) / 360.0) for hh in (0, 60, 120, 180, 240)] + [(hh, (599 - hh) / 360.0) for hh in (300, 240, 345)]:
        d0 = F(dmin + (dmax - dmin) * F(z))
        cand = (d0 + np.arange(-300, 301, dtype=np.float32) * np.spacing(d0)).astype(np.float32)
        _, _, info = rr.depth_hsv(cand.reshape(1, -1), dmin, dmax)
        hit = np.nonzero(info["hue"].reshape(-1) == hue)[0]
        if len(hit) == 0:                                                  # (hue 0: see test_planted_cases_are_not_vacuous) the two depths around the boundary
            hh = info["hue"].reshape(-1)
            k = int(np.argmin(np.where(hh < 180, hh, np.inf)))
            hit = np.array([k, k + 1])
        sp.extend(cand[hit[:2]].tolist())
    flat[:len(sp)] = np.array(sp, np.float32)
    return d, dmin, dmax
