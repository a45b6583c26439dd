"""The frame renderer's definition (DESIGN.md "Frame rendering") restated in numpy: binary32 op by op, one rounding per operation (the library is built
without contraction and with IEEE division and square root, so the same sequence gives the same bits), including the fixed sequences bf_dm_exp /
bf_dm_log / bf_dm_pow of include/bf_detmath.h.

shade(depth, colors, Kinv, state, use_material, tracking_lost, thresh_offset, thresh_lin) -> (target float32 (h, w, 4), rgba8 uint8 (h, w, 4), info)
depth_hsv(depth, dmin, dmax) -> (target, rgba8)          rgbx(img) -> rgba8
shade64(...): the same picture in float64 with libm (a yardstick for the arithmetic, not a definition).
"""
import numpy as np

from tests.calibrator_ref import quad_survives

F = np.float32
NINF = F(-np.inf)
QNAN_BITS = np.uint32(0x7FC00000)

DEFAULT_STATE = dict(
    s_materialShininess=16.0, s_materialAmbient=(0.75, 0.65, 0.5, 1.0), s_materialDiffuse=(1.0, 0.9, 0.7, 1.0), s_materialSpecular=(1.0, 1.0, 1.0, 1.0),
    s_lightAmbient=(0.4, 0.4, 0.4, 1.0), s_lightDiffuse=(0.6, 0.52944, 0.4566, 0.6), s_lightSpecular=(0.3, 0.3, 0.3, 1.0), s_lightDirection=(0.0, -1.0, 2.0))


# --------------------------------------------------------------------------- include/bf_detmath.h
def dm_round(x):
    with np.errstate(invalid="ignore"):
        return np.where(x >= 0, x + F(0.5), x - F(0.5)).astype(np.float32).astype(np.int32).astype(np.float32)


def dm_exp(x):
    x = np.asarray(x, np.float32)
    zero = x < F(-87.0)
    with np.errstate(all="ignore"):
        x = np.where(x > F(87.0), F(87.0), x)
        x = np.where(zero | np.isnan(x), F(0.0), x)            # lanes the result does not come from
        k = dm_round(x * F(1.44269504088896341))
        r = x - k * F(0.693145751953125)
        r = r - k * F(1.42860682030941723212e-6)
        p = np.full_like(r, F(1.3888889e-3))
        for c in (8.3333338e-3, 4.1666668e-2, 1.6666667e-1, 0.5, 1.0, 1.0):
            p = p * r + F(c)
        scale = ((k.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(np.float32)
        out = p * scale
    assert out.dtype == np.float32
    return np.where(zero, F(0.0), out)


def dm_log(x):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        pos = x > 0
        v = np.where(pos, x, F(1.0))
        den = v < F(1.17549435e-38)
        v = np.where(den, v * F(8388608.0), v)
        e = np.where(den, -23, 0).astype(np.int32)
        u = v.view(np.uint32)
        e = e + (u >> np.uint32(23)).astype(np.int32) - 127
        m = ((u & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(np.float32)
        big = m > F(1.41421356237)
        m = np.where(big, m * F(0.5), m)
        e = e + big.astype(np.int32)
        f = m - F(1.0)
        s = f / (F(2.0) + f)
        z = s * s
        p = np.full_like(z, F(2.2222222e-1))
        for c in (2.8571430e-1, 4.0000001e-1, 6.6666669e-1):
            p = p * z + F(c)
        lm = F(2.0) * s + (s * z) * p
        ef = e.astype(np.float32)
        out = ef * F(0.693145751953125) + (ef * F(1.42860682030941723212e-6) + lm)
    assert out.dtype == np.float32
    return np.where(pos, out, NINF)


def dm_pow(x, y):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        pos = x > 0
        out = dm_exp(F(y) * dm_log(np.where(pos, x, F(1.0))))
    return np.where(pos, out, F(0.0)).astype(np.float32)


# --------------------------------------------------------------------------- helpers
def _dot4(m, a, b, c, d):
    return ((m[0] * a + m[1] * b) + m[2] * c) + m[3] * d


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(v):
    ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return [v[0] / ln, v[1] / ln, v[2] / ln]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _max0(a):
    return np.where(a > 0, a, np.zeros_like(a))


def quantize(c):
    """(uint8)(int)(min(max(c, 0), 1) * 255 + 0.5); NaN -> 0"""
    with np.errstate(invalid="ignore"):
        v = _max0(c)
        v = np.where(v < 1, v, np.ones_like(v))
        return (v * c.dtype.type(255.0) + c.dtype.type(0.5)).astype(np.int32).astype(np.uint8)


def present(target, drawn):
    """target (h, w, 4) -> RGBA8: r, g, b quantised, alpha 255 where one of them is above 0; a pixel that is not drawn gives 0"""
    h, w = drawn.shape
    out = np.zeros((h, w, 4), np.uint8)
    for k in range(3):
        out[..., k] = np.where(drawn, quantize(np.where(drawn, target[..., k], 0).astype(target.dtype)), 0)
    out[..., 3] = np.where((out[..., 0] > 0) | (out[..., 1] > 0) | (out[..., 2] > 0), 255, 0)
    return out


def positions(depth, Kinv, dtype=np.float32):
    depth = np.asarray(depth, dtype)
    Kinv = np.asarray(Kinv, dtype).reshape(4, 4)
    h, w = depth.shape
    x, y = np.meshgrid(np.arange(w, dtype=dtype), np.arange(h, dtype=dtype))
    d = np.where(np.isfinite(depth), depth, dtype(0.0))
    xd, yd = x * d, y * d
    return [_dot4(Kinv[0], xd, yd, d, d), _dot4(Kinv[1], xd, yd, d, d), _dot4(Kinv[3], xd, yd, d, d)]


def _shade(depth, colors, Kinv, state, use_material, tracking_lost, thresh_offset, thresh_lin, dtype, powf):
    T = dtype
    depth32 = np.ascontiguousarray(depth, np.float32)
    colors = np.ascontiguousarray(colors, np.float32)
    h, w = depth32.shape
    st = dict(DEFAULT_STATE); st.update(state or {})
    covered = quad_survives(depth32, thresh_offset, thresh_lin)
    fin = np.isfinite(depth32)
    P = positions(depth32.astype(T), Kinv, T)

    def shift(a, dx, dy, fill):
        p = np.full((h + 2, w + 2), fill, a.dtype)
        p[1:h + 1, 1:w + 1] = a
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    border = ~(shift(np.ones((h, w), bool), 0, 1, False) & shift(np.ones((h, w), bool), 0, -1, False) & shift(np.ones((h, w), bool), 1, 0, False) & shift(np.ones((h, w), bool), -1, 0, False))
    nonfinite = ~border & ~(shift(fin, 0, 1, False) & shift(fin, 0, -1, False) & shift(fin, 1, 0, False) & shift(fin, -1, 0, False))
    with np.errstate(all="ignore"):
        a = [shift(P[k], 0, 1, T(0)) - shift(P[k], 0, -1, T(0)) for k in range(3)]        # P(x, y+1) - P(x, y-1)
        b = [shift(P[k], 1, 0, T(0)) - shift(P[k], -1, 0, T(0)) for k in range(3)]        # P(x+1, y) - P(x-1, y)
        nr = _cross(a, b)
        ln = np.sqrt((nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2])
        degenerate = ~(np.isfinite(ln) & (ln > 0))
        nocolor = colors[..., 0] == NINF
        drawn = covered & ~border & ~nonfinite & ~degenerate & ~nocolor
        ln = np.where(drawn, ln, T(1.0))
        n = _normalize([nr[0] / ln, nr[1] / ln, nr[2] / ln])                              # RGBDRenderer's normalize, then PhongPS's own
        eye = _normalize([np.where(drawn, P[k], T(1.0)) for k in range(3)])
        L = _normalize([T(v) for v in st["s_lightDirection"]])
        i = [-L[0], -L[1], -L[2]]
        ndl = _dot3(n, i)
        two = T(2.0) * ndl
        R = _normalize([i[k] - two * n[k] for k in range(3)])
        rde = _max0(_dot3(R, eye))
        spec = powf(rde, T(st["s_materialShininess"]))
        pow_args = [rde[drawn]]
        col = colors.astype(T)
        LA, LD, LS = ([T(v) for v in st[k]] for k in ("s_lightAmbient", "s_lightDiffuse", "s_lightSpecular"))
        res = [None] * 4
        if use_material:
            andl = np.abs(ndl)
            for k in range(3):
                mat = col[..., k]
                amb = LA[k] * mat
                dif = powf((LD[k] * mat) * andl, T(1.2))
                pow_args.append(((LD[k] * mat) * andl)[drawn])
                spc = (LS[k] * mat) * spec
                res[k] = ((amb * T(0.5) + T(1.2) * dif) + T(0.8) * spc) * T(1.2)
            res[3] = np.ones((h, w), T)
        else:
            MA, MD, MS = ([T(v) for v in st[k]] for k in ("s_materialAmbient", "s_materialDiffuse", "s_materialSpecular"))
            mdl = _max0(ndl)
            for k in range(4):
                res[k] = (LA[k] * MA[k] + (LD[k] * MD[k]) * mdl) + (LS[k] * MS[k]) * spec
        if tracking_lost:
            res[0] = res[1] = res[2]
    for r in res:
        assert r.dtype == T
    target = np.stack(res, -1)
    rgba = present(target, drawn)
    reasons = dict(uncovered=~covered, border=covered & border, nonfinite=covered & nonfinite, degenerate=covered & ~border & ~nonfinite & degenerate,
                   nocolor=covered & ~border & ~nonfinite & ~degenerate & nocolor)
    return target, rgba, dict(drawn=drawn, reasons=reasons, pow_args=np.concatenate(pow_args))


def shade(depth, colors, Kinv, state=None, use_material=False, tracking_lost=False, thresh_offset=0.012, thresh_lin=0.001):
    target, rgba, info = _shade(depth, colors, Kinv, state, use_material, tracking_lost, thresh_offset, thresh_lin, np.float32, dm_pow)
    bits = target.view(np.uint32).copy()
    bits[np.isnan(target)] = QNAN_BITS                         # a NaN is written as the canonical quiet NaN
    bits[~info["drawn"]] = NINF.view(np.uint32)
    return bits.view(np.float32), rgba, info


def shade64(depth, colors, Kinv, state=None, use_material=False, tracking_lost=False, thresh_offset=0.012, thresh_lin=0.001):
    def powf(x, y):
        with np.errstate(all="ignore"):
            return np.where(x > 0, np.power(np.where(x > 0, x, 1.0), y), 0.0)
    return _shade(depth, colors, Kinv, state, use_material, tracking_lost, thresh_offset, thresh_lin, np.float64, powf)


# --------------------------------------------------------------------------- modes 3 and 4
def depth_hsv(depth, dmin, dmax):
    """depthToHSVDevice / convertDepthToRGB / convertHSVToRGB, then the presentation stage"""
    d = np.ascontiguousarray(depth, np.float32)
    dmin, dmax = F(dmin), F(dmax)
    with np.errstate(all="ignore"):
        gate = (d != NINF) & (d != 0) & (d >= dmin) & (d <= dmax)
        dd = np.where(gate, d, dmin)
        x = F(1.0) - (dd - dmin) / (dmax - dmin)
        x = np.where(x < 0, F(0.0), x)
        x = np.where(x > 1, F(1.0), x)
        x = F(360.0) * x - F(120.0)
        x = np.where(x < 0, x + F(359.0), x)
        hd = x / F(60.0)
        hi = np.where(hd > 0, hd, F(0.0)).astype(np.uint32)          # toward zero; NaN and negatives -> 0
        f = hd - hi.astype(np.float32)
        V, S = F(0.5), F(1.0)
        p = np.full_like(f, V * (F(1.0) - S))
        q = V * (F(1.0) - S * f)
        t = V * (F(1.0) - S * (F(1.0) - f))
        Vv = np.full_like(f, V)
    sel = [(Vv, t, p), (q, Vv, p), (p, Vv, t), (p, q, Vv), (t, p, Vv), (Vv, p, q)]
    case = np.where((hi == 0) | (hi == 6), 0, np.where(hi <= 4, hi, 5)).astype(np.int64)
    target = np.zeros(d.shape + (4,), np.float32)
    for k in range(3):
        target[..., k] = np.where(gate, np.choose(case, [s[k] for s in sel]), F(0.0))
    target[..., 3] = np.where(gate, F(1.0), F(0.0))
    bits = target.view(np.uint32).copy()
    bits[np.isnan(target)] = QNAN_BITS
    target = bits.view(np.float32)
    return target, present(target, np.ones(d.shape, bool)), dict(gate=gate, hue=np.where(gate, x, F(-1.0)), h=hi)


def rgbx(img):
    out = np.ascontiguousarray(img, np.uint8).copy()
    out[..., 3] = 255
    return out


# --------------------------------------------------------------------------- planted cases (shared by the CPU and the GPU tests)
def planted_kinv():
    """fx = fy = 64, principal point (32, 4): every entry is a power of two or a small integer times one, so that positions of depths with few
    mantissa bits are exact and the degenerate normal below is an exact zero"""
    K = np.eye(4, dtype=np.float64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 64.0, 64.0, 32.0, 4.0
    return np.linalg.inv(K).astype(np.float32)


def spread_at_threshold(thresh_offset, thresh_lin):
    """(dmin, dmax) in float32 with dmax - dmin == offset + lin * (0.5 * (dmax + dmin)) exactly, found by search"""
    off, lin = F(thresh_offset), F(thresh_lin)
    dmin = (F(1.0) + np.arange(4096, dtype=np.float32) * F(2.0 ** -12)).astype(np.float32)
    base = (dmin + (np.float64(off) + np.float64(lin) * dmin) / (1.0 - 0.5 * np.float64(lin))).astype(np.float32)      # the real solution, then the floats around it
    for j in range(-8, 9):
        cand = (base + F(j) * F(2.0 ** -23)).astype(np.float32)
        eq = (cand - dmin) == off + lin * (F(0.5) * (cand + dmin))
        if eq.any():
            k = int(np.argmax(eq))
            return dmin[k], cand[k]
    raise AssertionError("no float32 pair sits exactly on the threshold")


def planted_gbuffer(w=67, h=9, thresh_offset=0.012, thresh_lin=0.001, seed=5):
    """A smooth slanted surface with the edge cases of the G-buffer stage planted where the size allows.  Returns depth (h, w), colors (h, w, 4)."""
    rng = np.random.RandomState(seed)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    depth = (F(1.0) + F(0.0015) * x + F(0.0021) * y + F(0.0004) * np.sin(x * F(0.7)) * np.cos(y * F(0.9))).astype(np.float32)
    colors = np.concatenate([rng.uniform(0.02, 1.0, (h, w, 3)), np.ones((h, w, 1))], -1).astype(np.float32)
    if w >= 67 and h >= 9:
        depth[2, 5] = -np.inf; depth[7, 40:42] = -np.inf                  # holes
        depth[3:6, 11:14] = F(0.1)                                        # the near plane: not above it ...
        depth[3:6, 19:22] = np.nextafter(F(0.1), F(1.0))                  # ... and just above it
        dmin, dmax = spread_at_threshold(thresh_offset, thresh_lin)
        depth[0:3, 24:27] = dmin; depth[1, 25] = dmax                     # spread == offset + lin * mid: the four quads around it survive
        depth[0:3, 38:41] = dmin; depth[1, 39] = np.nextafter(dmax, F(4.0))     # an ulp above: they are dropped
        colors[5, 8, 0] = -np.inf                                         # no colour
        colors[5, 16, :3] = np.nan                                        # a NaN colour: drawn, black
        colors[7, 50:56, :3] = F(0.05)                                    # dark and bright: pow arguments on both sides of 1
        colors[1, 50:56, :3] = F(1.0)
        depth[6:9, 58:61] = F(1.25)                                       # a flat patch facing the camera
        # pixel (32, 4) lies on the principal point.  Its quad is flat at 1.5; the neighbours above and to the left hold -1.5 (finite, and not part of
        # its quad), which makes both differences (0, 0, 3): parallel, the cross product is an exact zero
        depth[4:6, 32:34] = F(1.5)
        depth[3, 32] = F(-1.5); depth[4, 31] = F(-1.5)
    return depth, colors
