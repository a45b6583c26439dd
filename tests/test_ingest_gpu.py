"""GPU parity tests (-m gpu): the frame-ingest image operators (csrc/imageops.hip, bf_image_interleave_texels), the dense frame cache
(csrc/cache.hip) and the image manager (bf_image_manager_*) at edge shapes, through the C ABI vs the CPU oracle.

Tolerance: none.  Every operator here is compiled with -ffp-contract=off, tabulates its Gaussian taps on the host with the oracle's expf
and sums them in the oracle's order, so results are compared as BYTES.  Device outputs are pre-filled with a sentinel pattern and followed
by a guard tail: a pixel the oracle leaves unwritten must keep its sentinel bytes, and the tail must be untouched.

Shapes: widths 1, 2, 63, 64, 65, 130, 641 (one 64-wide tile row, its edges, partial tiles) x heights 1, 3, 4, 5, 481 (the 4-row tile and
its edges), plus 1280 x 960.  Cache: W x H of 81x61, 100x75, 17x13 (partial 16x12 tiles and a partial 64-pixel workgroup), 16x12 and 2x2,
colour at another size than depth, sigma 0 (unfiltered) and 3 (radius 6, the LDS limit).
"""
import numpy as np
import pytest

from bundlefusion_amd import synth
from bundlefusion_amd.capi import BFError, default_app_state, default_bundling_state, intrinsics_matrix, sensor_desc

pytestmark = pytest.mark.gpu

GUARD_BYTES = 4096
WIDTHS = (1, 2, 63, 64, 65, 130, 641)
HEIGHTS = (1, 3, 4, 5, 481)
SHAPES = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(1280, 960)]
ERODE = ((0, 1, 1), (1, 3, 9), (3, 3, 10), (3, 15, 49), (5, 40, 121))      # (structureSize, fracReq = a / b): all but 3/10 (the ingest's 0.3) land exactly on count / (2s+1)^2
SIGMAS = (0.25, 1.0, 2.0, 4.0)                                             # radius ceil(2 sigma) = 1, 2, 4, 8 (MAX_R)


@pytest.fixture(scope="module", autouse=True)
def _oracle_threads(oracle):
    oracle.set_threads(16)
    yield
    oracle.set_threads(1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frac(num, den):
    """num / den rounded to float32 as the kernels compute count / sum (a correctly rounded float32 division)"""
    return float(np.float32(num) / np.float32(den))


class _Out:
    """A device output image pre-filled with sentinel bytes and followed by a guard tail of sentinel bytes."""

    def __init__(self, shape, dtype, seed=0):
        import torch
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape)) * self.dtype.itemsize
        self.init = np.random.default_rng(seed).integers(0, 256, self.n + GUARD_BYTES, dtype=np.uint8)
        self.buf = torch.from_numpy(self.init.copy()).cuda()
        tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.uint32): torch.int32}[self.dtype]
        self.t = self.buf[:self.n].view(tdt).view(self.shape)

    def sentinel(self):
        """the image part of the sentinel, as the image's type (the oracle writes into a copy of it)"""
        return self.init[:self.n].view(self.dtype).reshape(self.shape)

    def check(self, expected, what):
        got = self.buf.cpu().numpy()
        assert np.array_equal(got[self.n:], self.init[self.n:]), what + ": guard tail written"
        exp = np.ascontiguousarray(expected).view(np.uint8).reshape(-1)
        assert exp.size == self.n
        bad = np.flatnonzero(got[:self.n] != exp)
        assert bad.size == 0, "%s: %d of %d bytes differ, first at element %d" % (what, bad.size, self.n, bad[0] // self.dtype.itemsize)


def _depth(w, h, seed):
    """Blocks of depth levels whose neighbours differ by just under or just over 0.05 (erosion's dThresh == the filter's sigmaR), a
    faint ramp, and sprinkled -inf, 0.0 and NaN."""
    rng = np.random.default_rng(seed)
    levels = np.float32([1.0, 1.0499, 1.0501, 1.0998, 1.1002])
    blk = rng.integers(0, len(levels), ((h + 1) // 2, (w + 2) // 3))
    d = np.repeat(np.repeat(levels[blk], 2, axis=0), 3, axis=1)[:h, :w]
    d = (d + np.float32(1e-6) * np.arange(w, dtype=np.float32)[None, :]).astype(np.float32)
    u = rng.random((h, w))
    d[u < 0.04] = -np.inf
    d[(u >= 0.04) & (u < 0.06)] = 0.0
    d[(u >= 0.06) & (u < 0.063)] = np.nan
    return np.ascontiguousarray(d)


def _color(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _shape_id(s):
    return "%dx%d" % s


# ------------------------------------------------------------------------------------------------ image operators
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_erode_depth_map(gpu, oracle, shape):
    w, h = shape
    d = _depth(w, h, w * 7 + h)
    din = _dev(d)
    for s, a, b in ERODE:
        frac = _frac(a, b)
        o = _Out((h, w), np.float32, seed=s)
        gpu.capi.image_erode_depth_map(o.t, din, s, 0.05, frac)
        o.check(oracle.erode_depth(d, s, 0.05, frac, out=o.sentinel()), "erode %s s=%d frac=%r" % (shape, s, frac))


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_gauss_filter_depth_map(gpu, oracle, shape):
    w, h = shape
    d = _depth(w, h, w * 5 + h)
    din = _dev(d)
    for sigma in SIGMAS:
        o = _Out((h, w), np.float32, seed=1)
        gpu.capi.image_gauss_filter_depth_map(o.t, din, sigma, 0.05)
        o.check(oracle.gauss_filter_depth(d, sigma, 0.05, out=o.sentinel()), "depth filter %s sigma=%g" % (shape, sigma))


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_gauss_filter_intensity(gpu, oracle, shape):
    w, h = shape
    img = np.random.default_rng(w * 3 + h).random((h, w)).astype(np.float32)
    iin = _dev(img)
    for sigma in SIGMAS:
        o = _Out((h, w), np.float32, seed=2)
        gpu.capi.image_gauss_filter_intensity(o.t, iin, sigma)
        o.check(oracle.gauss_filter_intensity(img, sigma, out=o.sentinel()), "intensity filter %s sigma=%g" % (shape, sigma))


# (input w, h) -> (output w, h): up, down, non-integer ratios both ways, ow = 2, input width or height 1
RESAMPLE = (((64, 4), (130, 5)), ((641, 481), (320, 240)), ((130, 5), (63, 3)), ((65, 3), (2, 2)), ((1, 481), (64, 5)), ((641, 1), (65, 4)),
            ((1, 1), (2, 2)), ((2, 3), (130, 4)), ((63, 5), (641, 481)), ((1280, 960), (641, 481)), ((641, 481), (2, 481)))


@pytest.mark.parametrize("pair", RESAMPLE, ids=lambda p: "%dx%d_to_%dx%d" % (p[0] + p[1]))
def test_resample(gpu, oracle, pair):
    (iw, ih), (ow, oh) = pair
    d, c = _depth(iw, ih, iw + ih), _color(iw, ih, iw * ih)
    o = _Out((oh, ow), np.float32, seed=3)
    gpu.capi.image_resample_float(o.t, _dev(d))
    o.check(oracle.resample_float(d, ow, oh, out=o.sentinel()), "resample float %s" % (pair,))
    o = _Out((oh, ow, 4), np.uint8, seed=4)
    gpu.capi.image_resample_uchar4(o.t, _dev(c))
    o.check(oracle.resample_uchar4(c, ow, oh, out=o.sentinel()), "resample uchar4 %s" % (pair,))
    o = _Out((oh, ow), np.float32, seed=5)
    gpu.capi.image_resample_to_intensity(o.t, _dev(c))
    o.check(oracle.resample_to_intensity(c, ow, oh, out=o.sentinel()), "resample to intensity %s" % (pair,))


@pytest.mark.parametrize("shape", ((1, 1), (65, 5), (130, 3), (641, 481)), ids=_shape_id)
def test_fused_forms_equal_their_composition(gpu, oracle, shape):
    """erosion + colour copies in one launch (second copy absent and present); the depth filter writing two outputs"""
    w, h = shape
    d, c = _depth(w, h, 11), _color(w, h, 12)
    din, cin = _dev(d), _dev(c)
    e = oracle.erode_depth(d, 3, 0.05, 0.3)
    for two in (False, True):
        o, c1, c2 = _Out((h, w), np.float32, 6), _Out((h, w, 4), np.uint8, 7), _Out((h, w, 4), np.uint8, 8)
        gpu.capi.image_erode_depth_map_and_copy(o.t, din, cin, c1.t, c2.t if two else None, 3, 0.05, 0.3)
        o.check(e, "erode_and_copy depth %s" % (shape,))
        c1.check(c, "erode_and_copy copy 1 %s" % (shape,))
        c2.check(c if two else c2.sentinel(), "erode_and_copy copy 2 %s (given: %s)" % (shape, two))
    g = oracle.gauss_filter_depth(e, 2.0, 0.05)
    o1, o2 = _Out((h, w), np.float32, 9), _Out((h, w), np.float32, 10)
    gpu.capi.image_gauss_filter_depth_map2(o1.t, o2.t, _dev(e), 2.0, 0.05)
    o1.check(g, "depth filter map2 output 1 %s" % (shape,))
    o2.check(g, "depth filter map2 output 2 %s" % (shape,))


def _texels(depth, color):
    n = depth.size
    t = np.empty((n, 8), np.uint8)
    t[:, :4] = np.ascontiguousarray(depth, np.float32).view(np.uint8).reshape(n, 4)
    t[:, 4:] = np.ascontiguousarray(color, np.uint8).reshape(n, 4)
    return t


@pytest.mark.parametrize("shape", ((1, 1), (63, 5), (641, 481), (1280, 960)), ids=_shape_id)
def test_interleave_texels(gpu, shape):
    """{depth bits, RGBX} per pixel; 1280 x 960 is more pixels than the 2048 x 256 threads of the grid-stride loop"""
    w, h = shape
    d, c = _depth(w, h, 13), _color(w, h, 14)
    o = _Out((h * w, 8), np.uint8, 11)
    gpu.capi.image_interleave_texels(o.t, _dev(d), _dev(c))
    o.check(_texels(d, c), "texels %s" % (shape,))


def test_refused_arguments(gpu):
    import torch
    w, h = 65, 5
    x, y = _dev(_depth(w, h, 15)), torch.zeros(h, w, device="cuda")
    c = _dev(_color(w, h, 16))
    cap = gpu.capi
    refused = [
        ("erode in place", lambda: cap.image_erode_depth_map(x, x)),
        ("erode_and_copy in place", lambda: cap.image_erode_depth_map_and_copy(x, x, c, c.clone())),
        ("depth filter in place", lambda: cap.image_gauss_filter_depth_map(x, x, 1.0, 0.05)),
        ("depth filter map2, output 1 in place", lambda: cap.image_gauss_filter_depth_map2(x, y, x, 1.0, 0.05)),
        ("depth filter map2, output 2 in place", lambda: cap.image_gauss_filter_depth_map2(y, x, x, 1.0, 0.05)),
        ("intensity filter in place", lambda: cap.image_gauss_filter_intensity(x, x, 1.0)),
        ("depth filter radius 9", lambda: cap.image_gauss_filter_depth_map(y, x, 4.01, 0.05)),
        ("depth filter map2 radius 9", lambda: cap.image_gauss_filter_depth_map2(y, y.clone(), x, 4.01, 0.05)),
        ("intensity filter radius 9", lambda: cap.image_gauss_filter_intensity(y, x, 4.01)),
    ]
    for ow, oh in ((1, 5), (5, 1), (1, 1)):
        for fn, dt, src in ((cap.image_resample_float, torch.float32, x), (cap.image_resample_uchar4, torch.uint8, c),
                            (cap.image_resample_to_intensity, torch.float32, c)):
            out = torch.zeros((oh, ow, 4) if dt == torch.uint8 else (oh, ow), dtype=dt, device="cuda")
            refused.append(("%s to %dx%d" % (fn.__name__, ow, oh), lambda fn=fn, out=out, src=src: fn(out, src)))
    before = x.cpu().numpy().copy()
    for what, call in refused:
        with pytest.raises(BFError):
            call()
            pytest.fail(what + " was accepted")
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy().view(np.uint8), before.view(np.uint8)), "a refused call wrote its input"
    # the largest accepted radius is 8
    cap.image_gauss_filter_depth_map(y, x, 4.0, 0.05)
    cap.image_gauss_filter_intensity(y, x, 4.0)


# ------------------------------------------------------------------------------------------------ cache
CACHE_SIZES = ((81, 61), (100, 75), (17, 13), (16, 12), (2, 2))
CACHE_SIGMAS = ((2.5, 1.0), (0.0, 0.0), (3.0, 3.0), (0.0, 3.0), (3.0, 0.0))      # (color_sigma, depth_sigma_d)
CACHE_KEYS = ("depth", "campos", "normals", "normals_u", "intensity", "derivs")


def _cache_input(k, dw, dh, cw, ch, seed):
    d, _, _, Kd = synth.scene_room(k, dw, dh)
    c = synth.scene_room(k, cw, ch)[1]
    rng = np.random.default_rng(seed)
    d = (d + rng.normal(0, 0.004, d.shape)).astype(np.float32)
    d[dh // 3: dh // 3 + 7, dw // 2: dw // 2 + 20] = -np.inf
    d[rng.random(d.shape) < 0.01] = -np.inf
    return np.ascontiguousarray(d), np.ascontiguousarray(c), intrinsics_matrix(Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"])


def _assert_cache_frame(g, o, what):
    for key in CACHE_KEYS:
        H, W = g[key].shape[:2]
        a, b = g[key].view(np.uint8).reshape(H * W, -1), np.ascontiguousarray(o[key]).view(np.uint8).reshape(H * W, -1)
        bad = np.flatnonzero((a != b).any(axis=1))
        assert bad.size == 0, "%s %s: %d pixels differ, first (x, y) = (%d, %d)" % (what, key, bad.size, bad[0] % W, bad[0] // W)


@pytest.mark.parametrize("size", CACHE_SIZES, ids=_shape_id)
@pytest.mark.parametrize("sigmas", CACHE_SIGMAS, ids=lambda s: "color%g_depth%g" % s)
def test_cache_store_frame_edge_shapes(gpu, oracle, size, sigmas):
    W, H = size
    cs, ds = sigmas
    dw, dh, cw, ch = 161, 121, 200, 150                     # colour at another size than depth; odd depth sizes
    d0, c0, K = _cache_input(40, dw, dh, cw, ch, 1)
    d1, c1, _ = _cache_input(700, dw, dh, cw, ch, 2)
    cache = gpu.capi.Cache(dw, dh, W, H, 2, K, color_sigma=cs, depth_sigma_d=ds, depth_sigma_r=0.05)
    o0 = oracle.cache_store_frame(d0, c0, W, H, K, cs, ds, 0.05)
    o1 = oracle.cache_store_frame(d1, c1, W, H, K, cs, ds, 0.05)
    what = "cache %dx%d sigmas %s" % (W, H, sigmas)
    cache.store_frame(_dev(d0), _dev(c0))
    _assert_cache_frame(cache.download_frame(0), o0, what + " frame 0")
    cache.store_frame(_dev(d1), _dev(c1))
    assert cache.num_frames() == 2
    _assert_cache_frame(cache.download_frame(1), o1, what + " frame 1")
    _assert_cache_frame(cache.download_frame(0), o0, what + " frame 0 after frame 1")
    with pytest.raises(BFError):
        cache.store_frame(_dev(d0), _dev(c0))                # more frames than max_images
    assert cache.num_frames() == 2
    cache.close()


def test_cache_refused_arguments(gpu):
    K = intrinsics_matrix(100.0, 100.0, 40.0, 30.0)
    for cs, ds in ((3.01, 1.0), (2.5, 3.01)):                 # radius 7 > 6, the LDS halo's limit
        with pytest.raises(BFError):
            gpu.capi.Cache(80, 60, 17, 13, 2, K, color_sigma=cs, depth_sigma_d=ds)
    cache = gpu.capi.Cache(80, 60, 17, 13, 2, K)
    c = _dev(_color(80, 60, 3))
    for dw, dh in ((81, 60), (80, 59)):
        with pytest.raises(BFError):
            cache.store_frame(_dev(np.ones((dh, dw), np.float32)), c)
    assert cache.num_frames() == 0
    cache.close()


# ------------------------------------------------------------------------------------------------ image manager
def _manager(gpu, dw, dh, cw, ch, wi, hi, erode=True, depth_filter=True, on_gpu=1, texels=False, max_images=None, submap=None):
    gas, gbs = default_app_state(), default_bundling_state()
    gas.s_integrationWidth, gas.s_integrationHeight = wi, hi
    gbs.s_widthSIFT, gbs.s_heightSIFT = cw, ch
    gbs.s_erodeSIFTdepth, gbs.s_depthFilter = int(erode), int(depth_filter)
    if max_images is not None:
        gbs.s_maxNumImages, gbs.s_submapSize = max_images, submap
    s = sensor_desc(dw, dh, intrinsics_matrix(0.8 * dw, 0.8 * dw, dw / 2, dh / 2))
    s.colorWidth, s.colorHeight = cw, ch
    im = gpu.capi.ImageManager(gas, gbs, s, on_gpu)
    if texels:
        im.set_store_texels(True)
    return im, gbs


def _expected_ingest(oracle, gbs, depth, color, wi, hi):
    """CUDAImageManager::process by tests/oracle_pipeline.py::_ingest's rules, colour resampled from its own size -> (raw, filtered) at
    sensor resolution and the (depth, colour) frame stored at integration resolution"""
    raw = depth
    if gbs.s_erodeSIFTdepth:
        raw = oracle.erode_depth(oracle.erode_depth(raw, 3, 0.05, 0.3), 3, 0.05, 0.3)
    filt = oracle.gauss_filter_depth(raw, gbs.s_depthSigmaD, gbs.s_depthSigmaR) if gbs.s_depthFilter else raw.copy()
    dh, dw = depth.shape
    ch, cw = color.shape[:2]
    sd = (filt if gbs.s_erodeSIFTdepth else raw) if (dw, dh) == (wi, hi) else oracle.resample_float(filt, wi, hi)
    sc = color if (cw, ch) == (wi, hi) else oracle.resample_uchar4(color, wi, hi)
    return raw, filt, sd, sc


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_ingest(im, frame, exp, color, what, last=True):
    raw, filt, sd, sc = exp
    d, c = im.get_integrate_frame_cpu(frame)
    assert _same(d, sd), what + ": stored depth of frame %d" % frame
    assert _same(c, sc), what + ": stored colour of frame %d" % frame
    if last:
        graw, gfilt, gcol = im.get_input_gpu()
        assert _same(graw, raw), what + ": raw sensor-resolution depth"
        assert _same(gfilt, filt), what + ": filtered sensor-resolution depth"
        assert _same(gcol, color), what + ": sensor-resolution colour"


def test_image_manager_fused_path_equals_host_input_and_unfused(gpu, oracle):
    """Equal sizes, erosion and filter on: device input takes the fused three-launch path; host input and device input with texels on take the
    unfused one.  All three store the same bytes, frame after frame (the input sets rotate)."""
    w, h = 130, 97
    frames = [(_depth(w, h, 20 + i), _color(w, h, 30 + i)) for i in range(5)]
    ims = {"device (fused)": _manager(gpu, w, h, w, h, w, h), "host": _manager(gpu, w, h, w, h, w, h),
           "device, texels on": _manager(gpu, w, h, w, h, w, h, texels=True)}
    for i, (d, c) in enumerate(frames):
        exp = _expected_ingest(oracle, ims["host"][1], d, c, w, h)
        for name, (im, _) in ims.items():
            got = im.process(d, c) if name == "host" else im.process_device(_dev(d), _dev(c))
            assert got and im.num_frames() == i + 1 and im.curr_frame_number() == i
            _assert_ingest(im, i, exp, c, "%s, frame %d" % (name, i))
            t = im.get_integrate_frame_texels(i)
            if name == "device, texels on":
                assert _same(t.reshape(-1, 8), _texels(exp[2], exp[3])), "texels of frame %d" % i
            else:
                assert t is None
    for i, (d, c) in enumerate(frames):
        exp = _expected_ingest(oracle, ims["host"][1], d, c, w, h)
        for name, (im, _) in ims.items():
            _assert_ingest(im, i, exp, c, "%s, frame %d after the last" % (name, i), last=False)


# (depth w, h), (colour w, h), (integration w, h)
MANAGER_SIZES = (((130, 97), (130, 97), (130, 97)), ((641, 479), (641, 479), (320, 240)), ((160, 120), (200, 150), (160, 120)),
                 ((161, 121), (160, 120), (160, 120)), ((97, 73), (130, 97), (64, 48)))


@pytest.mark.parametrize("sizes", MANAGER_SIZES, ids=lambda s: "d%dx%d_c%dx%d_i%dx%d" % (s[0] + s[1] + s[2]))
@pytest.mark.parametrize("erode,depth_filter", ((1, 1), (1, 0), (0, 1), (0, 0)), ids=("erode_filter", "erode", "filter", "neither"))
def test_image_manager_branches(gpu, oracle, sizes, erode, depth_filter):
    (dw, dh), (cw, ch), (wi, hi) = sizes
    frames = [(_depth(dw, dh, 40 + i), _color(cw, ch, 50 + i)) for i in range(2)]
    for device in (False, True):
        im, gbs = _manager(gpu, dw, dh, cw, ch, wi, hi, erode, depth_filter)
        for i, (d, c) in enumerate(frames):
            assert im.process_device(_dev(d), _dev(c)) if device else im.process(d, c)
            _assert_ingest(im, i, _expected_ingest(oracle, gbs, d, c, wi, hi), c, "%s input %s erode=%d filter=%d frame %d" % (
                "device" if device else "host", sizes, erode, depth_filter, i))
        _assert_ingest(im, 0, _expected_ingest(oracle, gbs, *frames[0], wi, hi), frames[0][1], "frame 0 after frame 1", last=False)
        im.close()


@pytest.mark.parametrize("sizes", MANAGER_SIZES[:3], ids=lambda s: "d%dx%d_c%dx%d_i%dx%d" % (s[0] + s[1] + s[2]))
def test_image_manager_frames_on_host(gpu, oracle, sizes):
    """storeFramesOnGPU = 0: the stored frames are host copies (the reference's default); no texels are kept"""
    (dw, dh), (cw, ch), (wi, hi) = sizes
    frames = [(_depth(dw, dh, 60 + i), _color(cw, ch, 70 + i)) for i in range(3)]
    im, gbs = _manager(gpu, dw, dh, cw, ch, wi, hi, on_gpu=0, texels=True)
    for i, (d, c) in enumerate(frames):
        assert im.process_device(_dev(d), _dev(c)) if i % 2 else im.process(d, c)
        _assert_ingest(im, i, _expected_ingest(oracle, gbs, d, c, wi, hi), c, "host frames %s frame %d" % (sizes, i))
        assert im.get_integrate_frame_texels(i) is None
    for i, (d, c) in enumerate(frames):
        _assert_ingest(im, i, _expected_ingest(oracle, gbs, d, c, wi, hi), c, "host frames %s frame %d after the last" % (sizes, i), last=False)
    im.close()


@pytest.mark.parametrize("texels", (False, True), ids=("fused", "texels"))
def test_image_manager_across_the_slab_boundary(gpu, oracle, texels):
    """260 tiny frames: the stored frames cross the 256-frame slab boundary and the four input sets rotate 65 times; frames 0, 255, 256 and
    the last (and their texels) still hold their own images."""
    w, h, n = 8, 6, 260
    frames = [(_depth(w, h, 1000 + i), _color(w, h, 2000 + i)) for i in range(n)]
    im, gbs = _manager(gpu, w, h, w, h, w, h, texels=texels)
    for i, (d, c) in enumerate(frames):
        assert im.process_device(_dev(d), _dev(c))
    assert im.num_frames() == n and im.curr_frame_number() == n - 1
    exp = {}
    for i in (0, 1, 254, 255, 256, 257, n - 1):
        exp[i] = _expected_ingest(oracle, gbs, *frames[i], w, h)
        _assert_ingest(im, i, exp[i], frames[i][1], "frame %d of %d" % (i, n), last=i == n - 1)
        t = im.get_integrate_frame_texels(i)
        if texels:
            assert _same(t.reshape(-1, 8), _texels(exp[i][2], exp[i][3])), "texels of frame %d" % i
        else:
            assert t is None
    im.reset()
    assert im.num_frames() == 0
    with pytest.raises(BFError):
        im.curr_frame_number()
    d, c = frames[7]
    assert im.process_device(_dev(d), _dev(c))
    _assert_ingest(im, 0, _expected_ingest(oracle, gbs, d, c, w, h), c, "first frame after reset")
    im.close()


def test_image_manager_stops_at_max_images(gpu):
    im, _ = _manager(gpu, 8, 6, 8, 6, 8, 6, max_images=2, submap=2)
    d, c = _depth(8, 6, 3), _color(8, 6, 4)
    for i in range(4):
        assert im.process(d, c)
    assert not im.process(d, c) and not im.process_device(_dev(d), _dev(c))
    assert im.num_frames() == 4
    im.close()
