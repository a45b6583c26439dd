"""Planted images for the SIFT detector (csrc/sift.hip), shared by tests/test_sift_cases_cpu.py (the proof, on the oracle, that every image still
drives the branch it is named after) and tests/test_sift_cases_gpu.py (the HIP kernels held to the oracle bit for bit).  Pure numpy: no GPU, no oracle.

A case is (name, intensity, depth, kwargs); kwargs are the detector parameters shared by capi.Sift and oracle_api.sift_run / sift_stages
(min_key_scale, feature_count_threshold, depth_min, depth_max).  Every image is 160 x 152 or smaller: there the per-level cap fmax =
clamp(int(w * h * 0.005), 32, 4096) of the raw key list and of the feature list is 32 (61 on octave 0 of 128 x 96) and a lattice of period 13 holds
several times as many extrema, far below the candidate buffer (cap = max(128, 5 fmax) = 160 / 305; the CPU test asserts that no case comes near it).

  lattice   I = 0.5 + a cos(2 pi (x + ph) / P) cos(2 pi (y + 2 ph) / (P + 0.5)): extrema every P / 2 pixels on the level whose scale fits P, most with two
            orientations (the four-fold symmetry), those of the first image rows with one when ph is no integer.
  mixed     P = 13 on the left half, P = 26 on the right, 4 x 4 block noise: keys on five levels with very different counts - what the two
            LimitFeatureCount passes and the scale gate need.
  blobs     isolated Gaussians: a blob of standard deviation b gives one key on the level whose scale fits b (b = 3: octave 0; 12: octave 2; 20: octave 3).

Level counts on the oracle (slots 0..11 = octave * 3 + DoG level; `raw` uncapped, `l0` after limit 0, `rs` after the reshape, `l1` after limit 1), as
tests/test_sift_cases_cpu.py prints and asserts them:
  cap64            64x64 P13 ph1.5, scale gate 0, threshold 0: raw[0] = 73 > fmax 32 (npad 128); l0 = rs = l1 = 32; 28 of the 32 keys have two orientations: 18 keys fill the list
  cap64_straddle   the same with depth -inf under its first two keys: raw[0] = 71; key 17 has two orientations and 31 in front of it: its second one is cut
  cap72x88         72x88 P13 ph1.5 (no multiple of the 32-pixel blur tile nor of the 16-pixel detect tile): raw[0] = 109, key 18 straddles the cap
  cap128_oct1      128x96 P26 ph1.5: raw[2] = 9 (npad 64), raw[3] = 63 > 32 on octave 1; rs = [0 0 18 32]
  cap128_oct0      128x96 P13: raw[0] = 221 > fmax 61 (npad 256)
  mixed_*          128x96, scale gate 0: raw = l0 = [61 5 11 17 0 1] (75 uncapped on slot 0; total 95), rs = [61 7 18 32 0 2] (total 120)
    thr 40: limit 0 keeps all (95 - 61 = 34 <= 40), limit 1 drops slots 0 and 1 (120 - 61 = 59, 59 - 7 = 52 > 40; 52 - 18 = 34)
    thr 20: limit 0 drops slots 0, 1 (29 - 11 = 18 <= 20), limit 1 drops slot 2 as well (52 - 18 = 34 > 20; 34 - 32 = 2)
    thr 34 = total - l0[0]: limit 0 keeps all, thr 33 drops slot 0;  thr 59 = total - rs[0]: limit 1 keeps all, thr 58 drops slot 0
    scale gate 0 / LEVEL0_SCALE (= slot 0's sigma * keyLocScale: kept by >=) / the next float above it (slot 0 goes) / 4.1 (only slot 5 stays)
  depth_*          the mixed image (keys on octaves 0 and 1) under a ramp depth map of another size (64x48 and 160x120 under 128x96; 64x48 under a 64x64 mixed
                   image, seed 1) with a row band of -inf, a column band below depth_min and one above depth_max, each across the look-up pixels of
                   several keys; depth128_inf_right: lattice P13 under 64x48, right part -inf: 61 features
  borders          96x80, blobs 4 pixels from each border and in two corners, keys on slots 0 and 1 within 3 sigma of all four borders, and keys on octave 2
  coarse64         64x64, one blob b = 16: the only key sits on slot 8 (octave 2, 16x16);  coarse96_oct3: 96x80, b = 20: slot 9 (octave 3, 12x10)
  constant         no key at all
"""
import numpy as np

DEPTH_MIN, DEPTH_MAX = 0.1, 4.0
# bf_sift_create: sigma0 = 1.6f * powf(2, 1.0f / 3); slot 0 has sigma = sigma0 * powf(2, 0) and keyLocScale 1
LEVEL0_SCALE = float(np.float32(1.6) * np.power(np.float32(2.0), np.float32(1.0) / np.float32(3.0), dtype=np.float32))


def fmax_of(w, h):
    """per-level cap of an octave of w x h pixels (bf_sift_create)"""
    return int(min(4096, max(32, int(np.float32(w * h) * np.float32(0.005)))))


def cand_cap_of(w, h):
    return min(8192, max(128, 5 * fmax_of(w, h)))


def lattice(W, H, P, a=0.4, ph=0.0):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return (0.5 + a * np.cos(2 * np.pi * (x + ph) / P) * np.cos(2 * np.pi * (y + 2 * ph) / (P + 0.5))).astype(np.float32)


def mixed(W=128, H=96, seed=2, amp=0.15):
    I = lattice(W, H, 13).astype(np.float64)
    I[:, W // 2:] = lattice(W, H, 26)[:, W // 2:]
    nz = np.random.default_rng(seed).uniform(-amp, amp, (H // 4, W // 4))
    return np.clip(I + np.kron(nz, np.ones((4, 4))), 0.0, 1.0).astype(np.float32)


def blobs(W, H, spec, base=0.2):
    """spec: (cx, cy, standard deviation, amplitude) per blob"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    I = np.full((H, W), base)
    for cx, cy, b, a in spec:
        I += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * b * b))
    return I.astype(np.float32)


def flat_depth(I, value=1.0):
    return np.full(I.shape, value, np.float32)


def depth_lookup(col, row, octave, W, H, dW, dH):
    """the depth pixel k_detect reads for the key (col, row) of an octave: roundf (half away from zero) of pos * (dW - 1) / (W - 1), in float32"""
    f = np.float32
    s = f(1 << octave)
    px = (s * f(col) + f(0.5)) * f(dW - 1) / f(W - 1)
    py = (s * f(row) + f(0.5)) * f(dH - 1) / f(H - 1)
    return int(np.floor(px + f(0.5))), int(np.floor(py + f(0.5)))


def ramp_depth(dW, dH, inf_rows=None, near_cols=None, far_cols=None):
    """every pixel its own depth (steps of 0.01 along x, 0.007 along y), crossed by a row band of -inf, a column band below depth_min and one above depth_max"""
    y, x = np.mgrid[0:dH, 0:dW].astype(np.float64)
    d = (0.5 + 0.01 * x + 0.007 * y).astype(np.float32)
    if inf_rows:
        d[inf_rows[0]:inf_rows[1], :] = -np.inf
    if near_cols:
        d[:, near_cols[0]:near_cols[1]] = np.float32(0.05)
    if far_cols:
        d[:, far_cols[0]:far_cols[1]] = np.float32(5.0)
    return d


NO_GATES = dict(min_key_scale=0.0, feature_count_threshold=0)
CAP64_KNOCKED_KEYS = [(5, 4), (11, 4)]          # (col, row) of the first two raster-order keys of slot 0 of cap64


def cap64():
    I = lattice(64, 64, 13, ph=1.5)
    return "cap64", I, flat_depth(I), dict(NO_GATES)


def cap64_straddle():
    I = lattice(64, 64, 13, ph=1.5)
    d = flat_depth(I)
    for col, row in CAP64_KNOCKED_KEYS:
        dx, dy = depth_lookup(col, row, 0, 64, 64, 64, 64)
        d[dy, dx] = -np.inf
    return "cap64_straddle", I, d, dict(NO_GATES)


def cap72x88():
    I = lattice(72, 88, 13, ph=1.5)
    return "cap72x88", I, flat_depth(I), dict(NO_GATES)


def cap128_oct1():
    I = lattice(128, 96, 26, ph=1.5)
    return "cap128_oct1", I, flat_depth(I), dict(NO_GATES)


def cap128_oct0():
    I = lattice(128, 96, 13, ph=1.5)
    return "cap128_oct0", I, flat_depth(I), dict(NO_GATES)


def _mixed(name, **kw):
    I = mixed()
    return name, I, flat_depth(I), dict(dict(min_key_scale=0.0, feature_count_threshold=0), **kw)


MIXED_RAW_TOTAL, MIXED_RAW0, MIXED_RS_TOTAL, MIXED_RS0 = 95, 61, 120, 61        # asserted on the oracle by the CPU test


def mixed_limit1_drops():
    return _mixed("mixed_limit1_drops", feature_count_threshold=40)


def mixed_both_drop():
    return _mixed("mixed_both_drop", feature_count_threshold=20)


def mixed_limit0_boundary():
    return _mixed("mixed_limit0_boundary", feature_count_threshold=MIXED_RAW_TOTAL - MIXED_RAW0)


def mixed_limit0_below_boundary():
    return _mixed("mixed_limit0_below_boundary", feature_count_threshold=MIXED_RAW_TOTAL - MIXED_RAW0 - 1)


def mixed_limit1_boundary():
    return _mixed("mixed_limit1_boundary", feature_count_threshold=MIXED_RS_TOTAL - MIXED_RS0)


def mixed_limit1_below_boundary():
    return _mixed("mixed_limit1_below_boundary", feature_count_threshold=MIXED_RS_TOTAL - MIXED_RS0 - 1)


def mixed_scale0():
    return _mixed("mixed_scale0")


def mixed_scale_boundary():
    return _mixed("mixed_scale_boundary", min_key_scale=LEVEL0_SCALE)


def mixed_scale_above_boundary():
    return _mixed("mixed_scale_above_boundary", min_key_scale=float(np.nextafter(np.float32(LEVEL0_SCALE), np.float32(10.0))))


def mixed_scale41():
    return _mixed("mixed_scale41", min_key_scale=4.1)


def mixed_defaults():
    """the pipeline's own parameters (scale gate 3.0, threshold 150)"""
    I = mixed()
    return "mixed_defaults", I, flat_depth(I), dict(min_key_scale=3.0, feature_count_threshold=150)


def depth128_half():
    return "depth128_half", mixed(), ramp_depth(64, 48, inf_rows=(13, 15), near_cols=(9, 11), far_cols=(45, 47)), dict(NO_GATES)


def depth128_wider():
    return "depth128_wider", mixed(), ramp_depth(160, 120, inf_rows=(32, 35), near_cols=(24, 27), far_cols=(113, 117)), dict(NO_GATES)


def depth64_rows_only():
    return "depth64_rows_only", mixed(64, 64, seed=1), ramp_depth(64, 48, inf_rows=(15, 17), near_cols=(13, 15), far_cols=(52, 54)), dict(NO_GATES)


def depth128_inf_right():
    I = lattice(128, 96, 13, ph=1.5)
    d = ramp_depth(64, 48)
    d[:, 40:] = -np.inf
    return "depth128_inf_right", I, d, dict(NO_GATES)


def borders():
    W, H, m, b, a = 96, 80, 4, 3.0, 0.7
    I = blobs(W, H, [(m, 40, b, a), (W - 1 - m, 40, b, a), (48, m, b, a), (48, H - 1 - m, b, a), (m, m, b, a), (W - 1 - m, H - 1 - m, b, a)])
    return "borders", I, flat_depth(I), dict(NO_GATES)


def coarse64():
    I = blobs(64, 64, [(32, 32, 16.0, 0.7)])
    return "coarse64", I, flat_depth(I), dict(NO_GATES)


def coarse96_oct3():
    I = blobs(96, 80, [(48, 40, 20.0, 0.7)])
    return "coarse96_oct3", I, flat_depth(I), dict(NO_GATES)


def constant():
    I = np.full((64, 64), 0.5, np.float32)
    return "constant", I, flat_depth(I), dict(NO_GATES)


def many_keys640():
    """The one image beyond 160 x 152 (not among CASE_NAMES): 640 x 480, lattices of period 13 | 16.5 | 21 side by side, threshold 0.  Slots 0, 1, 2 hold
    1536 + 1088 + 863 = 3487 raw keys, more than the 2048 workgroups k_orientation was launched with whatever the image: the keys behind the 2048th kept
    `no orientation` and were dropped.  1439 of them have one."""
    I = lattice(640, 480, 13).copy()
    I[:, 213:] = lattice(640, 480, 16.5)[:, 213:]
    I[:, 426:] = lattice(640, 480, 21)[:, 426:]
    return "many_keys640", I, flat_depth(I), dict(NO_GATES)


BUILDERS = [cap64, cap64_straddle, cap72x88, cap128_oct1, cap128_oct0,
            mixed_limit1_drops, mixed_both_drop, mixed_limit0_boundary, mixed_limit0_below_boundary, mixed_limit1_boundary, mixed_limit1_below_boundary,
            mixed_scale0, mixed_scale_boundary, mixed_scale_above_boundary, mixed_scale41, mixed_defaults,
            depth128_half, depth128_wider, depth64_rows_only, depth128_inf_right,
            borders, coarse64, coarse96_oct3, constant]
CASE_NAMES = [b.__name__ for b in BUILDERS]
CAP_CASES = ["cap64", "cap64_straddle", "cap72x88", "cap128_oct1", "cap128_oct0"]
_cache = {}


def case(name):
    """(name, intensity, depth, kwargs) of a case, built once; the arrays are read-only"""
    if name not in _cache:
        got = many_keys640() if name == "many_keys640" else BUILDERS[CASE_NAMES.index(name)]()
        assert got[0] == name
        got[1].setflags(write=False); got[2].setflags(write=False)
        _cache[name] = got
    return _cache[name]


def key_slots(level_counts):
    """slot (octave * 3 + DoG level) of every output feature: the key list is ordered by slot"""
    return np.repeat(np.arange(12), np.asarray(level_counts))


def blob_field():
    """The image of the float64 cross-check (test_sift_cases_cpu.py): isolated Gaussian blobs at integer centres, well apart and away from the borders.
    Amplitude 0.4, bright and dark: the ring of opposite sign around a blob is a line of near-ties (its determinant test sits at 0) and stays below the
    contrast threshold at this amplitude; at 0.5 it passes it.  Returns (intensity, [(cx, cy, b)])."""
    spec = [(20, 20, 2.5, 0.4), (50, 20, 3.0, -0.4), (84, 22, 3.5, 0.4), (124, 26, 4.0, -0.4), (24, 64, 5.0, 0.4), (72, 64, 6.0, -0.4),
            (32, 120, 9.0, -0.4), (104, 120, 9.0, 0.4)]        # the coarse blobs at multiples of 8: integer centres on octave 2 too
    return blobs(160, 152, spec, base=0.5), [(cx, cy, b) for cx, cy, b, a in spec]
