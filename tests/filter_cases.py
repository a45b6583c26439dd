"""Planted inputs of the match filter chain (Kabsch filter, surface-area filter, dense verification), shared by tests/test_match_filter_edge_cpu.py
(oracle against the compiled reference) and tests/test_match_filter_edge_gpu.py (HIP kernels against the oracle).  Pure numpy, fixed seeds: both tests
see the same bytes.

A Kabsch / surface-area case is one image pair.  Its key points live in ONE image slot of MAX_KEYS keys: the source image's keys in slots
[0, 128), the target image's in [128, 256); the filters address keys through the match indices only, so which image a slot belongs to does not
matter to them.  pack() lays a list of cases out as the key store of a manager with one image per case plus a current image and checks every index."""
import numpy as np

MAX_RAW, MAX_FILT = 128, 25
MAX_KEYS = 256
TGT = 128                                          # first key slot of the target image inside a case
W_IMG, H_IMG = 640, 480
K = np.eye(4, dtype=np.float32)
K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 583.0, 583.0, 319.5, 239.5
_K64 = K.astype(np.float64)
_K64inv = np.linalg.inv(_K64)


# ------------------------------------------------------------------------------------------------ geometry helpers
def _pose(rng, rot=0.12, trans=0.25):
    """a rigid motion: rotation by `rot` rad about a random axis, translation of length `trans` mostly along x (parallax in the image)"""
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(rot) * A + (1 - np.cos(rot)) * (A @ A)
    t = np.array([1.0, 0.15 * rng.normal(), 0.15 * rng.normal()]); t *= trans / np.linalg.norm(t)
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T


def _apply(T, P):
    return (T[:3, :3] @ P.T).T + T[:3, 3]


def keys_from_points(P):
    """key points (x, y, scale, depth) of camera-space points: the projection through K, as _keys_from_points of tests/test_ref_pin_cpu.py"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        uv = (_K64[:3, :3] @ P.T).T
        return np.c_[uv[:, 0] / uv[:, 2], uv[:, 1] / uv[:, 2], np.full(len(P), 3.0), P[:, 2]].astype(np.float32)


def _points_from_pixels(uv, z):
    uv = np.asarray(uv, np.float64).reshape(-1, 2); z = np.asarray(z, np.float64).reshape(-1)
    return (_K64inv[:3, :3] @ np.c_[uv[:, 0] * z, uv[:, 1] * z, z].T).T


def _spread(rng, n, T, min_px=9.0, zlo=1.2, zhi=3.0, fixed_src=None, fixed_tgt=None, box=(20, W_IMG - 20, 20, H_IMG - 20)):
    """n points in the source camera whose projections keep min_px from one another in BOTH images (and from the given fixed pixel positions)"""
    src = [] if fixed_src is None else [np.asarray(p, np.float64) for p in fixed_src]
    tgt = [] if fixed_tgt is None else [np.asarray(p, np.float64) for p in fixed_tgt]
    out = []
    for _ in range(200000):
        if len(out) == n:
            break
        uv = np.array([rng.uniform(box[0], box[1]), rng.uniform(box[2], box[3])])
        P = _points_from_pixels(uv, rng.uniform(zlo, zhi))[0]
        q = keys_from_points(_apply(T, P[None]))[0, :2].astype(np.float64)
        if all(np.hypot(*(uv - s)) > min_px for s in src) and all(np.hypot(*(q - s)) > min_px for s in tgt):
            src.append(uv); tgt.append(q); out.append(P)
    assert len(out) == n, "could not place %d spread points" % n
    return np.array(out).reshape(n, 3)


def _raw_case(family, name, P, Q, rng, n_counter=None, dist=None, **meta):
    """P, Q: matched camera-space points of the two images (at most 128 stored); n_counter: the raw match counter (may exceed 128, as the matcher's does)"""
    m = len(P)
    assert m == len(Q) and m <= MAX_RAW
    keys = np.zeros((MAX_KEYS, 4), np.float32)
    keys[:m] = keys_from_points(P); keys[TGT:TGT + m] = keys_from_points(Q)
    idx = np.zeros((MAX_RAW, 2), np.uint32)
    idx[:m, 0] = np.arange(m); idx[:m, 1] = TGT + np.arange(m)
    d = np.zeros(MAX_RAW, np.float32)
    d[:m] = np.sort(rng.uniform(0.05, 0.6, m)).astype(np.float32) if dist is None else dist
    return dict(family=family, name="%s/%s" % (family, name), keys=keys, idx=idx, dist=d, n=int(m if n_counter is None else n_counter), **meta)


def _inliers(rng, n, noise=0.002, **kw):
    T = _pose(rng)
    P = _spread(rng, n, T, **kw)
    Q = _apply(T, P) + rng.normal(0, noise, (n, 3))
    return T, P, Q


# ------------------------------------------------------------------------------------------------ Kabsch filter cases
NONFINITE = (-np.inf, np.inf, np.nan, 0.0)


def kabsch_cases():
    cases = []
    add = cases.append
    # clean inliers, n = 1 .. 160 (a counter above 128 with 128 entries stored)
    for n in (1, 2, 3, 4, 5, 6, 7, 12, 24, 25, 26, 40, 64, 127, 128, 129, 160):
        rng = np.random.default_rng(1000 + n)
        _, P, Q = _inliers(rng, min(n, MAX_RAW))
        add(_raw_case("clean", "n%d" % n, P, Q, rng, n_counter=n))
    # planted outliers at random positions
    for n in (16, 32, 64, 128):
        for k, nb in enumerate((1, n // 4, n // 2, 3 * n // 4)):
            for s in range(2):
                rng = np.random.default_rng(2000 + 100 * n + 10 * k + s)
                _, P, Q = _inliers(rng, n)
                bad = rng.choice(n, size=nb, replace=False)
                off = rng.uniform(0.1, 0.4, (nb, 3)) * rng.choice([-1.0, 1.0], (nb, 3))
                Q[bad] += off
                add(_raw_case("outliers", "n%d_bad%d_s%d" % (n, nb, s), P, Q, rng))
    # outliers at the head of the list: the removal loop goes down to three matches and restores the previous fit
    for n in (8, 20, 40):
        for k, pos in enumerate(((0,), (1,), (2,), (3,), (0, 1), (0, 3), (1, 2), (2, 3))):
            rng = np.random.default_rng(3000 + 10 * n + k)
            _, P, Q = _inliers(rng, n)
            for p in pos:
                Q[p] += rng.uniform(0.08, 0.3, 3) * rng.choice([-1.0, 1.0], 3)
            add(_raw_case("head", "n%d_at%s" % (n, "_".join(map(str, pos))), P, Q, rng))
    # pure garbage: unrelated point sets
    for n in (3, 5, 10, 30, 60, 128):
        for s in range(2):
            rng = np.random.default_rng(4000 + 10 * n + s)
            P = _spread(rng, n, np.eye(4))
            Q = _spread(rng, n, np.eye(4))
            add(_raw_case("garbage", "n%d_s%d" % (n, s), P, Q, rng))
    # degenerate geometry
    for n in (12, 30):                                 # coplanar (a tilted plane)
        rng = np.random.default_rng(5000 + n)
        T = _pose(rng)
        P = _spread(rng, n, T)
        uvz = keys_from_points(P).astype(np.float64)
        z = 2.0 + 0.001 * (uvz[:, 0] - 320.0) - 0.0005 * (uvz[:, 1] - 240.0)
        P = _points_from_pixels(uvz[:, :2], z)
        add(_raw_case("degenerate", "coplanar_n%d" % n, P, _apply(T, P) + rng.normal(0, 0.002, (n, 3)), rng))
    for n in (6, 12, 30):                              # collinear: condition number above 100, the verdict is invalid
        rng = np.random.default_rng(5100 + n)
        T = _pose(rng)
        s = np.linspace(-0.9, 0.9, n)
        P = np.c_[s, 0.3 * s + 0.05, 2.0 + 0.2 * s]
        add(_raw_case("degenerate", "collinear_n%d" % n, P, _apply(T, P) + rng.normal(0, 0.0005, (n, 3)), rng))
    for n in (8, 20):                                  # nearly coincident in space and in the image: all but one refused by the 5 px rule
        rng = np.random.default_rng(5200 + n)
        T = _pose(rng)
        P = np.array([0.1, -0.2, 2.0]) + rng.normal(0, 0.0005, (n, 3))
        add(_raw_case("degenerate", "coincident_n%d" % n, P, _apply(T, P), rng))
    for n in (8, 12):                                  # nearly coincident in space, spread in the image (a 3 cm cluster at 0.15 m: the noise is a tenth of its extent)
        rng = np.random.default_rng(5300 + n)
        T = _pose(rng, trans=0.02)
        P = _spread(rng, n, T, zlo=0.15, zhi=0.152, box=(270, 370, 190, 290))
        add(_raw_case("degenerate", "cluster_n%d" % n, P, _apply(T, P) + rng.normal(0, 0.002, (n, 3)), rng))
    # close key points
    for s in range(2):
        rng = np.random.default_rng(6000 + s)
        _, P, Q = _inliers(rng, 12)
        c = _raw_case("close", "repeated_s%d" % s, P, Q, rng); c["idx"][3] = c["idx"][1]; add(c)
        c = _raw_case("close", "shared_source_s%d" % s, P, Q, rng); c["idx"][5, 0] = c["idx"][2, 0]; add(c)
        for side in (0, 1):
            for name, gap in (("at5", np.float32(5.0)), ("above5", np.nextafter(np.float32(5.0), np.float32(np.inf)))):
                rng = np.random.default_rng(6100 + 10 * s + side)
                T = _pose(rng, rot=0.03)
                # raw match 0 at pixel (0, 200), depth 1.2 and raw match 1 at (gap, 200), depth 3.0 in image `side`; in the other image parallax moves them ~70 px apart
                uv = np.array([[0.0, 200.0], [float(gap), 200.0]])
                A = _points_from_pixels(uv, [1.2, 3.0])
                M = T if side == 0 else np.linalg.inv(T)
                B = _apply(M, A)
                ob = keys_from_points(B)[:, :2].astype(np.float64)
                assert np.hypot(*(ob[0] - ob[1])) > 30.0
                fs, ft = (uv, ob) if side == 0 else (ob, uv)
                R = _spread(rng, 8, T, fixed_src=fs, fixed_tgt=ft)
                P = np.r_[A if side == 0 else B, R]
                Q = np.r_[B if side == 0 else A, _apply(T, R) + rng.normal(0, 0.002, (8, 3))]
                c = _raw_case("close", "%s_image%d_s%d" % (name, side, s), P, Q, rng, gap_case=(name, side))
                k = c["keys"]
                a0, a1 = (0, 1) if side == 0 else (TGT, TGT + 1)
                k[a0, 0], k[a0, 1], k[a1, 0], k[a1, 1] = 0.0, 200.0, gap, 200.0      # the exact pixel values (the projection rounds them)
                add(c)
    # small n around minNumMatches, noisier
    for n in (1, 2, 3, 4, 5, 6):
        for s in range(2):
            rng = np.random.default_rng(7000 + 10 * n + s)
            _, P, Q = _inliers(rng, n, noise=0.004)
            add(_raw_case("small", "n%d_s%d" % (n, s), P, Q, rng))
    # twenty-five reached well before the list ends
    for n in (60, 100, 128, 140):
        rng = np.random.default_rng(8000 + n)
        _, P, Q = _inliers(rng, min(n, MAX_RAW), noise=0.001, min_px=14.0)
        add(_raw_case("early25", "n%d" % n, P, Q, rng, n_counter=n))
    # one key among the first ten raw matches with a non-finite (or zero) depth: the only route into the literal-sort fallback
    for s in range(2):
        for vi, val in enumerate(NONFINITE):
            for pi, pos in enumerate((0, 2, 5, 9)):
                rng = np.random.default_rng(9000 + 100 * s + 10 * vi + pi)
                _, P, Q = _inliers(rng, 30)
                c = _raw_case("nonfinite", "%s_at%d_s%d" % (str(val), pos, s), P, Q, rng, bad_value=float(val), bad_pos=pos)
                c["keys"][pos + (TGT if (vi + pi + s) % 2 else 0), 3] = np.float32(val)
                add(c)
    # distances are passed through only: equal and unsorted distances
    for n in (20, 40):
        rng = np.random.default_rng(9500 + n)
        _, P, Q = _inliers(rng, n)
        add(_raw_case("distances", "equal_n%d" % n, P, Q, rng, dist=np.full(n, 0.3, np.float32)))
        add(_raw_case("distances", "unsorted_n%d" % n, P, Q, rng, dist=rng.uniform(0.05, 0.6, n).astype(np.float32)))
    return cases


def greedy_addable(keys, idx, n):
    """the raw matches the 5 px rule alone (addMatch without any removal) would keep, in list order, up to 25: [(ix, iy)]"""
    kept = []
    for i in range(min(n, MAX_RAW)):
        if len(kept) >= MAX_FILT:
            break
        ai, aj = keys[idx[i, 0], :2], keys[idx[i, 1], :2]
        ok = True
        for kx, ky in kept:
            di = np.sqrt((ai[0] - keys[kx, 0]) * (ai[0] - keys[kx, 0]) + (ai[1] - keys[kx, 1]) * (ai[1] - keys[kx, 1]))
            dj = np.sqrt((aj[0] - keys[ky, 0]) * (aj[0] - keys[ky, 0]) + (aj[1] - keys[ky, 1]) * (aj[1] - keys[ky, 1]))
            if di <= 5 or dj <= 5:
                ok = False
                break
        if ok:
            kept.append((int(idx[i, 0]), int(idx[i, 1])))
    return kept


# ------------------------------------------------------------------------------------------------ surface-area cases
AREA_KINDS = ("spread", "coplanar", "collinear", "squeezed", "nonfinite")
AREA_SIZES = (1, 2, 3, 4, 5, 9, 16, 24, 25)


def area_cases():
    """filtered sets of n matches: dict(name, keys, fidx (n, 2))"""
    cases = []
    for ki, kind in enumerate(AREA_KINDS):
        for n in AREA_SIZES:
            rng = np.random.default_rng(20000 + 100 * ki + n)
            T = _pose(rng)
            P = np.c_[rng.uniform(-0.9, 0.9, n), rng.uniform(-0.7, 0.7, n), rng.uniform(1.2, 3.0, n)]
            if kind == "coplanar":
                P[:, 2] = 2.0 + 0.3 * P[:, 0] - 0.2 * P[:, 1]
            elif kind == "collinear":                   # extent across the line below 1e-5: area 0
                s = np.linspace(-0.8, 0.8, n) if n > 1 else np.zeros(1)
                P = np.c_[s, 0.25 * s, 2.0 + 0.125 * s]
            elif kind == "squeezed":
                P[:, :2] *= 0.05
            Q = _apply(T, P)
            keys = np.zeros((MAX_KEYS, 4), np.float32)
            keys[:n] = keys_from_points(P); keys[TGT:TGT + n] = keys_from_points(Q)
            if kind == "nonfinite":
                keys[(n // 2) + (TGT if n % 2 else 0), 3] = np.float32(NONFINITE[n % 4])
            fidx = np.c_[np.arange(n), TGT + np.arange(n)].astype(np.uint32)
            cases.append(dict(family=kind, name="%s/n%d" % (kind, n), keys=keys, fidx=fidx))
    return cases


# ------------------------------------------------------------------------------------------------ packing
def pack(cases, idx_key="idx"):
    """The key store of a manager with one image per case plus a current image (max_keys = MAX_KEYS): returns (allkeys [(len + 1) * MAX_KEYS, 4],
    [index pairs of each case with the case's image offset added], num_images).  Every index is checked against the key store here, before any
    of it is uploaded: no case may address memory outside it."""
    num_images = len(cases) + 1
    allkeys = np.zeros((num_images * MAX_KEYS, 4), np.float32)
    out = []
    for c, case in enumerate(cases):
        assert case["keys"].shape == (MAX_KEYS, 4) and case["keys"].dtype == np.float32
        allkeys[c * MAX_KEYS:(c + 1) * MAX_KEYS] = case["keys"]
        local = np.asarray(case[idx_key])
        assert local.dtype == np.uint32 and local.ndim == 2 and local.shape[1] == 2 and int(local.max()) < MAX_KEYS
        g = (local.astype(np.int64) + c * MAX_KEYS)
        assert g.min() >= 0 and g.max() < num_images * MAX_KEYS, case["name"]
        out.append(g.astype(np.uint32))
    return allkeys, out, num_images


def check_indices(idx, num_images, max_keys):
    """every key index of a list about to be uploaded lies inside the key store"""
    idx = np.asarray(idx)
    assert idx.size == 0 or (int(idx.min()) >= 0 and int(idx.max()) < num_images * max_keys), "match index outside the key store"
    return idx


# ------------------------------------------------------------------------------------------------ dense verification
# 32 x 160 is exactly DV_MAX_PIX pixels (the last size that is summed from LDS), 1024 x 32 exactly DV_THREADS threads; 160 x 120 and 128 x 150 take the
# recompute path; 33 x 17 and 31 x 33 have partial warps and a partial last row block
DENSE_GEOMETRIES = ((80, 60), (160, 120), (40, 30), (33, 17), (31, 33), (128, 150), (32, 160), (1024, 32))
DENSE_INPUT = (320, 240)
DENSE_FRAMES = (30, 35, 40)                         # scene_room frame numbers: previous, current, a third one for the trajectory test


def dense_inputs():
    """(frames, K): frames = [(depth, colour, camera-to-world)] of DENSE_FRAMES at 320 x 240 plus, last, a frame without any valid depth; K 4x4 f32"""
    from bundlefusion_amd import synth
    w, h = DENSE_INPUT
    src = [synth.scene_room(k, w, h) for k in DENSE_FRAMES]
    Kd = src[0][3]
    Kin = np.eye(4, dtype=np.float32)
    Kin[0, 0], Kin[1, 1], Kin[0, 2], Kin[1, 2] = Kd["fx"], Kd["fy"], Kd["mx"], Kd["my"]
    frames = [(np.ascontiguousarray(d, np.float32), np.ascontiguousarray(c), T.astype(np.float32)) for d, c, T, _ in src]
    frames.append((np.full((h, w), -np.inf, np.float32), frames[1][1], frames[1][2]))
    return frames, Kin


def cache_intrinsics(Kin, W, H):
    """intrinsics of the W x H cache frame of a DENSE_INPUT image, in the float32 arithmetic of the cache (CUDACache.cpp:20-24)"""
    w, h = DENSE_INPUT
    Kc = np.array(Kin, np.float32, copy=True)
    f = np.float32
    Kc[0, 0] = f(Kc[0, 0]) * (f(W) / f(w)); Kc[1, 1] = f(Kc[1, 1]) * (f(H) / f(h))
    Kc[0, 2] = f(Kc[0, 2]) * (f(W - 1) / f(w - 1)); Kc[1, 2] = f(Kc[1, 2]) * (f(H - 1) / f(h - 1))
    return Kc


def dense_transforms(frames):
    """[("gt", T), ("pushed", T)]: the transform from the previous frame (frames[0]) to the current one (frames[1]), and the same pushed 0.3 m"""
    rel = (np.linalg.inv(frames[1][2].astype(np.float64)) @ frames[0][2].astype(np.float64)).astype(np.float32)
    pushed = rel.copy(); pushed[0, 3] += np.float32(0.3)
    return [("gt", rel), ("pushed", pushed)]


def dense_flips(err, corr, default_ok):
    """(err_thresh, corr_thresh, expected verdict) around the oracle's err / corr: valid at err_thresh = err, invalid at the float below; valid at
    corr_thresh = corr, invalid at the float above; and the default thresholds"""
    e, c = np.float32(err), np.float32(corr)
    inf = np.float32(np.inf)
    return [(0.075, 0.02, bool(default_ok)),
            (float(e), 0.0, True), (float(np.nextafter(e, -inf)), 0.0, False),
            (10.0, float(c), True), (10.0, float(np.nextafter(c, inf)), False)]
