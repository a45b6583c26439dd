"""Float64 restatement of the bundling solver's equations, taken from the reference's definitions (numpy only).

Paths are relative to the reference's FriedLiver/Source.  Nothing here is derived from the HIP kernels:
  * sparse term     Solver/SolverBundlingEquationsLie.h:42-148, Solver/LieDerivUtil.h (dAlpha/dBeta/dGamma, left perturbation)
  * dense term      Solver/SolverBundling.cu:30-306, Solver/SolverBundlingDenseUtil.h, Solver/ICPUtil.h (bilinear)
  * energy / max residual   SolverBundlingEquationsLie.h:27-57, CUDASolverBundling.cpp computeMaxResidual
  * PCG             SolverBundling.cu:755-1022 and the early-out at :1088-1093
  * SE(3)           Solver/LieDerivUtil.h:19-207 (exp / log), :301-307 (update exp(delta) * T)

Unknowns per image are ordered [t0 t1 t2 | w0 w1 w2] (the reference's dense layout).  Every assembled entry comes with its
float64 value, S = the sum of |term| (a cancelling difference inside a term counts with the magnitudes of its operands) and the
term count n, from which the GPU tests build per-entry float32 bounds.
"""
import numpy as np

FLOAT_EPSILON = 1e-6           # SolverUtil.h:9
MINF = -np.inf
INVALID = 0xFFFFFFFF


# ----------------------------------------------------------------------------------------------------------------- SE(3)
def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_se3(rot, trans):
    """4x4 of the se(3) vector (rot, trans): R = exp([rot]x), t = V(rot) trans (closed forms, float64)."""
    rot = np.asarray(rot, np.float64); trans = np.asarray(trans, np.float64)
    th = np.linalg.norm(rot)
    K = skew(rot)
    if th < 1e-4:                                         # series: the closed forms cancel catastrophically here
        A, B, Cc = 1.0 - th ** 2 / 6.0, 0.5 - th ** 2 / 24.0, 1.0 / 6.0 - th ** 2 / 120.0
    else:
        A = np.sin(th) / th; B = (1 - np.cos(th)) / th ** 2; Cc = (1 - A) / th ** 2
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * K + B * (K @ K)
    T[:3, 3] = (np.eye(3) + B * K + Cc * (K @ K)) @ trans
    return T


def log_se3(T):
    """(rot, trans) with exp_se3(rot, trans) == T; rotation angle in [0, pi]."""
    T = np.asarray(T, np.float64)
    R = T[:3, :3]
    c = np.clip((np.trace(R) - 1) / 2, -1.0, 1.0)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5
    s = np.linalg.norm(v)
    th = np.arctan2(s, c)
    if th < 1e-12:
        rot = v.copy()
    elif np.pi - th > 1e-6:
        rot = v * (th / s)
    else:                                                 # near pi: the axis from the symmetric part
        S = (R + R.T) / 2 - c * np.eye(3)
        k = int(np.argmax(np.diag(S)))
        ax = S[:, k] / np.linalg.norm(S[:, k])
        if ax @ v < 0:
            ax = -ax
        rot = ax * th
    K = skew(rot)
    if th < 1e-4:
        Vinv = np.eye(3) - 0.5 * K + (1.0 / 12.0 + th ** 2 / 720.0) * (K @ K)
    else:
        A = np.sin(th) / th; B = (1 - np.cos(th)) / th ** 2
        Vinv = np.eye(3) - 0.5 * K + (1 - A / (2 * B)) / th ** 2 * (K @ K)
    return rot, Vinv @ T[:3, 3]


def poses_to_matrices(rot, trans):
    return np.stack([exp_se3(r, t) for r, t in zip(np.asarray(rot, np.float64), np.asarray(trans, np.float64))])


def lie_columns(w):
    """[I | dAlpha dBeta dGamma] at world points w[..., 3] -> [..., 3, 6]: d(exp(delta) w)/d delta at delta = 0."""
    w = np.asarray(w, np.float64)
    J = np.zeros(w.shape[:-1] + (3, 6))
    J[..., 0, 0] = J[..., 1, 1] = J[..., 2, 2] = 1.0
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    J[..., 1, 3], J[..., 2, 3] = -z, y
    J[..., 0, 4], J[..., 2, 4] = z, -x
    J[..., 0, 5], J[..., 1, 5] = -y, x
    return J


# ----------------------------------------------------------------------------------------------------------------- accumulation
class System:
    """A (6N x 6N) and b = -J^T F (6N), with per-entry |term| sums S, term counts n and the smallest non-zero single |term|."""

    def __init__(self, n):
        d = 6 * n
        self.n = n
        self.A = np.zeros((d, d)); self.SA = np.zeros((d, d)); self.nA = np.zeros((d, d))
        self.b = np.zeros(d); self.Sb = np.zeros(d); self.nb = np.zeros(d)
        self.minA = np.full((d, d), np.inf)
        self.minb = np.full(d, np.inf)

    def add_rows(self, img_a, img_b, Ja, Jb, r, w, Ja_abs, Jb_abs, r_abs):
        """k terms of m residual rows: Jacobian blocks Ja (k,m,6) on the images img_a (k,), Jb on img_b, residuals r (k,m),
        weights w (k,) and magnitude bounds of each.  Ja or Jb None: that image has no Jacobian (image 0 in the dense term)."""
        d = 6 * self.n
        blocks = [(np.asarray(img_a), Ja, Ja_abs), (np.asarray(img_b), Jb, Jb_abs)]
        for ia, Xa, Xa_abs in blocks:
            if Xa is None:
                continue
            for ib, Xb, Xb_abs in blocks:
                if Xb is None:
                    continue
                val = w[:, None, None] * np.einsum("kma,kmb->kab", Xa, Xb)
                mag = np.abs(w)[:, None, None] * np.einsum("kma,kmb->kab", Xa_abs, Xb_abs)
                rows = (6 * ia)[:, None, None] + np.arange(6)[None, :, None]
                cols = (6 * ib)[:, None, None] + np.arange(6)[None, None, :]
                flat = (rows * d + cols).ravel()
                self.A += np.bincount(flat, val.ravel(), d * d).reshape(d, d)
                self.SA += np.bincount(flat, mag.ravel(), d * d).reshape(d, d)
                nz = (val != 0).ravel()
                self.nA += np.bincount(flat[nz], None, d * d).reshape(d, d)
                np.minimum.at(self.minA.reshape(-1), flat[nz], np.abs(val).ravel()[nz])
            vb = -w[:, None] * np.einsum("kma,km->ka", Xa, r)
            mb = np.abs(w)[:, None] * np.einsum("kma,km->ka", Xa_abs, r_abs)
            idx = ((6 * ia)[:, None] + np.arange(6)[None, :]).ravel()
            self.b += np.bincount(idx, vb.ravel(), d)
            self.Sb += np.bincount(idx, mb.ravel(), d)
            nz = (vb != 0).ravel()
            self.nb += np.bincount(idx[nz], None, d)
            np.minimum.at(self.minb, idx[nz], np.abs(vb).ravel()[nz])

    def __iadd__(self, o):
        self.A += o.A; self.SA += o.SA; self.nA += o.nA; self.b += o.b; self.Sb += o.Sb; self.nb += o.nb
        self.minA = np.minimum(self.minA, o.minA); self.minb = np.minimum(self.minb, o.minb)
        return self


def valid_corr(corr, n):
    return (corr["imgIdx_i"] != INVALID) & (corr["imgIdx_i"] < n) & (corr["imgIdx_j"] < n)


def _world(T, idx, p):
    T = np.asarray(T, np.float64)
    p = np.asarray(p, np.float64)
    R, t = T[idx, :3, :3], T[idx, :3, 3]
    return np.einsum("kab,kb->ka", R, p) + t, np.einsum("kab,kb->ka", np.abs(R), np.abs(p)) + np.abs(t)


def sparse_rows(corr, T, n):
    """Per valid correspondence: images, world points, r = T_i p_i - T_j p_j and the Jacobian blocks with the role signs."""
    c = corr[valid_corr(corr, n)]
    ii, jj = c["imgIdx_i"].astype(np.int64), c["imgIdx_j"].astype(np.int64)
    wi, mi = _world(T, ii, c["pos_i"]); wj, mj = _world(T, jj, c["pos_j"])
    return dict(i=ii, j=jj, wi=wi, wj=wj, mag=mi + mj, r=wi - wj, Ji=lie_columns(wi), Jj=-lie_columns(wj),
                Ji_abs=np.abs(lie_columns(mi)), Jj_abs=np.abs(lie_columns(mj)))


def sparse_system(corr, T, n, w_sparse):
    s = System(n)
    q = sparse_rows(corr, T, n)
    k = len(q["i"])
    if k:
        s.add_rows(q["i"], q["j"], q["Ji"], q["Jj"], q["r"], np.full(k, float(w_sparse)), q["Ji_abs"], q["Jj_abs"], q["mag"])
    return s


def sparse_preconditioner(corr, T, n):
    """EquationsLie.h:105-147: unweighted sums over every correspondence touching the image; dense terms are not in it.
    Returns (M^-1 [6N], the sums [6N], the term counts [6N])."""
    q = sparse_rows(corr, T, n)
    p = np.zeros((n, 6))
    for img, w in ((q["i"], q["wi"]), (q["j"], q["wj"])):
        cols = lie_columns(w)
        for a in range(3):
            p[:, 3 + a] += np.bincount(img, (cols[:, :, 3 + a] ** 2).sum(1), n)
        p[:, :3] += np.bincount(img, None, n)[:, None]
    cnt = np.repeat((np.bincount(q["i"], None, n) + np.bincount(q["j"], None, n))[:, None], 6, 1)
    minv = np.where(p > FLOAT_EPSILON, 1.0 / np.where(p > 0, p, 1.0), 1.0)
    return minv.reshape(-1), p.reshape(-1), cnt.reshape(-1)


def energy(corr, T, n, w_sparse):
    """EvalResidualDevice: sum_c w r.r over the valid correspondences; also the sum of |term| by operand magnitudes."""
    q = sparse_rows(corr, T, n)
    return float(w_sparse) * float((q["r"] ** 2).sum()), abs(float(w_sparse)) * float((q["mag"] ** 2).sum())


def max_residual(corr, T, n, w_sparse):
    """computeMaxResidual: max over correspondences of w max_k |r_k| and the smallest index attaining it; also the runner-up
    value and the operand magnitude of the winner."""
    v = np.nonzero(valid_corr(corr, n))[0]
    q = sparse_rows(corr, T, n)
    vals = np.zeros(len(corr)); mags = np.zeros(len(corr))
    vals[v] = (float(w_sparse) * np.abs(q["r"])).max(1)
    mags[v] = abs(float(w_sparse)) * q["mag"].max(1)
    k = int(np.argmax(vals))
    second = float(np.partition(vals, -2)[-2]) if len(vals) > 1 else 0.0
    return float(vals[k]), k, second, float(mags[k])


# ----------------------------------------------------------------------------------------------------------------- dense term
DEFAULTS = dict(dist=0.15, normal=0.97, color=0.1, grad_min=0.005, depth_min=0.5, depth_max=4.0, subsample=4)
PIX_MARGIN = 1e-4              # pixel coordinates: distance to a rounding or bilinear-floor boundary, in pixels


def _round(u):
    return np.sign(u) * np.floor(np.abs(u) + 0.5)                    # roundf: half away from zero


def _near_frac(u):
    with np.errstate(invalid="ignore"):
        f = u - np.floor(u)
        return (np.abs(f - 0.5) < PIX_MARGIN) | (f < PIX_MARGIN) | (f > 1 - PIX_MARGIN)


def _near(x, t, margin):
    with np.errstate(invalid="ignore"):
        return np.abs(x - t) < margin * abs(t)


def _finite(a):
    return np.where(np.isfinite(a), a, 0.0)


def bilinear(x, y, img):
    """ICPUtil.h:28-111: taps outside the image or with a MINF first channel are skipped and each row renormalised.
    img [H, W, K]; x, y [P] -> [P, K] (MINF where no tap is valid)."""
    H, W, K = img.shape
    x0 = np.floor(x).astype(np.int64); y0 = np.floor(y).astype(np.int64)
    al = x - x0; be = y - y0
    ss = np.zeros((len(x), K)); ww = np.zeros(len(x))
    for dy, wy in ((0, 1 - be), (1, be)):
        s = np.zeros((len(x), K)); wsum = np.zeros(len(x))
        for dx, wx in ((0, 1 - al), (1, al)):
            px, py = x0 + dx, y0 + dy
            ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
            v = np.full((len(x), K), MINF)
            v[ok] = img[py[ok], px[ok]]
            ok &= v[:, 0] != MINF
            s[ok] += wx[ok, None] * v[ok]
            wsum[ok] += wx[ok]
        ok = wsum > 0
        ss[ok] += wy[ok, None] * (s[ok] / wsum[ok, None])
        ww[ok] += wy[ok]
    out = np.full((len(x), K), MINF)
    ok = ww > 0
    out[ok] = ss[ok] / ww[ok, None]
    return out


def angle_of(tr):
    """computeAngleDiff (DenseUtil.h:416-424): the angle by which the transform turns (1,1,1)/sqrt(3)."""
    x = np.ones(3) / np.sqrt(3.0)
    return float(abs(np.arccos(np.clip(x @ (tr[:3, :3] @ x), -1.0, 1.0))))


def _project(cp, tr, K):
    fx, fy, cx, cy = K
    with np.errstate(invalid="ignore", divide="ignore"):
        q = cp @ tr[:3, :3].T + tr[:3, 3]
        return q, q[:, 0] * fx / q[:, 2] + cx, q[:, 1] * fy / q[:, 2] + cy


def _depth_to_camera(x, y, d, K):
    fx, fy, cx, cy = K
    with np.errstate(invalid="ignore"):
        return np.stack([(x - cx) / fx * d, (y - cy) / fy * d, d], 1)


def _in_range(z, p, margin):
    with np.errstate(invalid="ignore"):
        ok = (z > p["depth_min"]) & (z < p["depth_max"])
    return ok, _near(z, p["depth_min"], margin) | _near(z, p["depth_max"], margin)


def _target_pixel(u, v, W, H):
    bad = ~(np.isfinite(u) & np.isfinite(v))
    tx, ty = _round(np.where(bad, -1.0, u)), _round(np.where(bad, -1.0, v))
    ok = (tx >= 0) & (ty >= 0) & (tx < W) & (ty < H)
    return ok, np.clip(tx, 0, W - 1).astype(np.int64), np.clip(ty, 0, H - 1).astype(np.int64)


def overlap_count(fi, fj, tr, geom, p, margin):
    """FindImageImageCorr_Kernel at the subsampled pixels (DenseUtil.h:22-42): (count, borderline count)."""
    W, H, K = geom
    s = p["subsample"]
    t = np.arange(512)
    x = (t % (W // s)) * s; y = (t // (W // s)) * s
    keep = y * W + x < W * H
    x, y = x[keep], y[keep]
    cp = _depth_to_camera(x, y, fj["depth"][y, x].astype(np.float64), K)
    ok, flag = _in_range(cp[:, 2], p, margin)
    q, u, v = _project(cp, tr, K)
    flag |= ok & (_near_frac(u) | _near_frac(v))
    okp, txc, tyc = _target_pixel(u, v, W, H)
    ok &= okp
    ct = _depth_to_camera(txc, tyc, fi["depth"][tyc, txc].astype(np.float64), K)
    ok2, fl2 = _in_range(ct[:, 2], p, margin)
    flag |= ok & fl2
    ok &= ok2
    with np.errstate(invalid="ignore"):
        dist = np.linalg.norm(q - ct, axis=1)
        flag |= ok & _near(dist, p["dist"], margin)
        ok &= dist <= p["dist"]
    return int(ok.sum()), int(flag.sum())


def weight_count(fi, fj, tr, geom, p, margin):
    """FindDenseCorrespondences_Kernel with uchar4 normals (DenseUtil.h:152-184) over every pixel: (count, borderline count)."""
    W, H, K = geom
    idx = np.arange(W * H)
    cp = _depth_to_camera(idx % W, idx // W, fj["depth"].reshape(-1).astype(np.float64), K)
    nu = fj["normals_u"].reshape(-1, 4)
    ok, flag = _in_range(cp[:, 2], p, margin)
    ok &= (nu != 0).any(1)
    nj = (nu[:, :3].astype(np.float64) / 255.0 * 2.0 - 1.0) @ tr[:3, :3].T
    q, u, v = _project(cp, tr, K)
    flag |= ok & (_near_frac(u) | _near_frac(v))
    okp, txc, tyc = _target_pixel(u, v, W, H)
    ok &= okp
    ct = _depth_to_camera(txc, tyc, fi["depth"][tyc, txc].astype(np.float64), K)
    ok2, fl2 = _in_range(ct[:, 2], p, margin)
    flag |= ok & fl2
    ok &= ok2
    nt = fi["normals_u"][tyc, txc]
    ok &= (nt != 0).any(1)
    nT = nt[:, :3].astype(np.float64) / 255.0 * 2.0 - 1.0
    with np.errstate(invalid="ignore"):
        dist = np.linalg.norm(q - ct, axis=1)
        dn = (nj * nT).sum(1)
        flag |= ok & (_near(dist, p["dist"], margin) | _near(dn, p["normal"], margin))
        ok &= (dn >= p["normal"]) & (dist <= p["dist"])
    return int(ok.sum()), int(flag.sum())


def pair_weight(count):
    """WeightDenseCorrespondences_Kernel (SolverBundling.cu:162-180)."""
    if count <= 0:
        return 0.0
    return 0.0 if count < 800 else 1.0 / min(np.log(count), 9.0)


def dense_pair_rows(fi, fj, Ti, Tj, geom, p, w_depth, w_color, pw, margin):
    """BuildDenseSystem_Kernel for the pair (i target, j source): the depth and colour rows of every pixel that is accepted
    or borderline.  Returns (row sets, #accepted, #borderline); a row set holds the Jacobians Xi, Xj (k,6) of the residual
    r (k,), the weights w, magnitude bounds X_abs / r_abs, the accept / borderline masks and the geometry (cs, ct, nt, dI)."""
    W, H, K = geom
    fx, fy = K[0], K[1]
    Ti = np.asarray(Ti, np.float64); Tj = np.asarray(Tj, np.float64)
    Tii = np.linalg.inv(Ti)
    tr = Tii @ Tj
    cp4 = fj["campos"].reshape(-1, 4).astype(np.float64)
    nj4 = fj["normals"].reshape(-1, 4).astype(np.float64)
    ok, flag = _in_range(cp4[:, 2], p, margin)
    sel = np.nonzero((ok | flag) & (nj4[:, 0] != MINF) & np.isfinite(cp4[:, 2]))[0]
    ok, flag = ok[sel], flag[sel]
    cs = cp4[sel, :3]
    n4 = nj4[sel] @ tr.T
    cst, u, v = _project(cs, tr, K)
    okp, _, _ = _target_pixel(u, v, W, H)
    ok &= okp
    flag |= _near_frac(u) | _near_frac(v)
    ci = bilinear(u, v, fi["campos"].astype(np.float64))
    ni = bilinear(u, v, fi["normals"].astype(np.float64))
    ok2, fl2 = _in_range(ci[:, 2], p, margin)
    flag |= fl2
    ok &= ok2 & (ni[:, 0] != MINF)
    have = np.isfinite(ci[:, 2]) & (ni[:, 0] != MINF)
    ct, nt = _finite(ci[:, :3]), _finite(ni[:, :3])
    dist = np.linalg.norm(cst - ct, axis=1)
    dn = (n4 * _finite(ni)).sum(1)
    flag |= _near(dist, p["dist"], margin) | _near(dn, p["normal"], margin)
    ok &= (dn >= p["normal"]) & (dist <= p["dist"])
    flag &= have
    # d cst / d delta for a left perturbation of T_j (source) and of T_i (target); w = T_j cs is the world point
    w = cs @ Tj[:3, :3].T + Tj[:3, 3]
    wmag = np.abs(cs) @ np.abs(Tj[:3, :3]).T + np.abs(Tj[:3, 3])
    dj = np.einsum("ab,kbc->kac", Tii[:3, :3], lie_columns(w))
    dabs = np.einsum("ab,kbc->kac", np.abs(Tii[:3, :3]), np.abs(lie_columns(wmag)))
    di = -dj
    out = []
    if w_depth > 0:                                      # :244-277, point to plane
        res = ((ct - cst) * nt).sum(1)
        out.append(dict(kind="depth", accept=ok, border=flag, w=w_depth * pw * np.maximum(0.0, 1.0 - ct[:, 2] / 2.0) ** 2.5, r=res,
                        r_abs=((np.abs(ct) + np.abs(cst)) * np.abs(nt)).sum(1),
                        Xi=-np.einsum("kac,ka->kc", di, nt), Xj=-np.einsum("kac,ka->kc", dj, nt),
                        X_abs=np.einsum("kac,ka->kc", dabs, np.abs(nt)), cs=cs, ct=ct, nt=nt))
    if w_color > 0:                                      # :278-304, intensity
        dI = bilinear(u, v, fi["derivs"].astype(np.float64))
        iT = bilinear(u, v, fi["intensity"].astype(np.float64)[:, :, None])[:, 0]
        isrc = fj["intensity"].reshape(-1).astype(np.float64)[sel]
        with np.errstate(invalid="ignore"):
            res = iT - isrc
            grad = np.sqrt(dI[:, 0] ** 2 + dI[:, 1] ** 2)
            okc = ok & (dI[:, 0] != MINF) & (np.abs(res) < p["color"]) & (grad > p["grad_min"])
            flagc = ((flag | _near(np.abs(res), p["color"], margin) | _near(grad, p["grad_min"], margin))
                     & np.isfinite(res) & (dI[:, 0] != MINF) & have & (ok | flag))
        dIc, resc = _finite(dI), _finite(res)
        z = cst[:, 2]
        P = np.zeros((len(z), 2, 3))
        P[:, 0, 0] = fx / z; P[:, 0, 2] = -fx * cst[:, 0] / z ** 2; P[:, 1, 1] = fy / z; P[:, 1, 2] = -fy * cst[:, 1] / z ** 2
        g = np.einsum("kp,kpa->ka", dIc, P)
        g_abs = np.einsum("kp,kpa->ka", np.abs(dIc), np.abs(P))
        out.append(dict(kind="color", accept=okc, border=flagc, w=w_color * pw * np.maximum(0.0, 1.0 - np.abs(resc) / (1.15 * p["color"])),
                        r=resc, r_abs=np.abs(_finite(iT)) + np.abs(_finite(isrc)),
                        Xi=np.einsum("ka,kac->kc", g, di), Xj=np.einsum("ka,kac->kc", g, dj), X_abs=np.einsum("ka,kac->kc", g_abs, dabs),
                        cs=cs, dI=dIc))
    return out, int(ok.sum()), int(flag.sum())


def dense_system(frames, T, geom, w_depth, w_color, use_pairwise=True, params=None, margin=1e-4, valid=None):
    """The dense term of one Gauss-Newton iteration at the poses T.  frames: per image the cache's downloaded arrays (depth,
    campos, normals, normals_u, intensity, derivs); geom = (W, H, (fx, fy, cx, cy)).  Returns (System of the pixels the float64
    decisions accept, System of the borderline pixels' terms = the allowance, one info dict per candidate pair)."""
    p = dict(DEFAULTS, **(params or {}))
    n = len(frames)
    T = np.asarray(T, np.float64)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    value, allow = System(n), System(n)
    info = []
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)] if use_pairwise else [(i, i + 1) for i in range(n - 1)]
    for i, j in pairs:
        if not (valid[i] and valid[j]):
            continue
        tr = np.linalg.inv(T[i]) @ T[j]
        ang = angle_of(tr)
        rec = dict(i=i, j=j, angle=ang, angle_border=abs(ang - 0.52) < margin * 0.52, pw=0.0, accepted=0, border=0)
        info.append(rec)
        if not ang < 0.52:
            continue
        rec["overlap"], rec["overlap_border"] = overlap_count(frames[i], frames[j], tr, geom, p, margin)
        if rec["overlap"] <= 10:
            continue
        cnt, cb = weight_count(frames[i], frames[j], tr, geom, p, margin)
        pw = pair_weight(cnt)
        rec.update(count=cnt, count_border=cb, pw=pw)
        if pw == 0.0:
            continue
        # a count off by the borderline pixels moves 1/log(count): that relative change joins the pair's allowance
        pw_err = max(abs(pair_weight(cnt + s * cb) - pw) for s in (-1, 1)) / pw if cb else 0.0
        rows, rec["accepted"], rec["border"] = dense_pair_rows(frames[i], frames[j], T[i], T[j], geom, p, w_depth, w_color, pw, margin)
        for q in rows:
            Xi = q["Xi"][:, None, :] if i > 0 else None
            Xj = q["Xj"][:, None, :] if j > 0 else None
            terms = ((q["accept"], value, q["w"]), (q["border"], allow, q["w"]), (q["accept"], allow, q["w"] * pw_err))
            for mask, target, wv in terms:
                k = int(mask.sum())
                if not k or not wv.any():
                    continue
                Xa = q["X_abs"][mask][:, None, :]
                if target is allow:          # the allowance holds magnitudes
                    target.add_rows(np.full(k, i), np.full(k, j), Xa if i > 0 else None, Xa if j > 0 else None,
                                    q["r_abs"][mask][:, None], np.abs(wv[mask]), Xa, Xa, q["r_abs"][mask][:, None])
                else:
                    target.add_rows(np.full(k, i), np.full(k, j), Xi[mask] if i > 0 else None, Xj[mask] if j > 0 else None,
                                    q["r"][mask][:, None], wv[mask], Xa, Xa, q["r_abs"][mask][:, None])
    return value, allow, info


# ----------------------------------------------------------------------------------------------------------------- PCG
def pcg(A, b, minv, n_iter, early_out=True):
    """SolverBundling.cu:755-1022 in float64 over the variables (image 0 is not one).  Returns (delta [6N], iterations run)."""
    A = np.asarray(A, np.float64); M = np.asarray(minv, np.float64)
    d = len(b)
    x = np.zeros(d); r = np.zeros(d); r[6:] = np.asarray(b, np.float64)[6:]
    p = M * r
    rz = r @ p
    it = 0
    for lin in range(n_iter):
        it += 1
        last = lin == n_iter - 1
        Ap = np.zeros(d); Ap[6:] = A[6:, 6:] @ p[6:]
        pAp = p @ Ap
        alpha = rz / pAp if pAp > FLOAT_EPSILON else 0.0
        x += alpha * p
        r -= alpha * Ap
        rz_new = (M * r) @ r
        if early_out and abs(pAp) < 5e-7:
            last = True
        beta = rz_new / rz if rz > FLOAT_EPSILON else 0.0
        rz = rz_new
        p = M * r + beta * p
        p[:6] = 0.0
        if last:
            break
    return x, it


def linear_residual(A, b, minv, x):
    """||b - A x||_M / ||b||_M over the variables (images >= 1)."""
    A = np.asarray(A, np.float64)[6:, 6:]; b = np.asarray(b, np.float64)[6:]; M = np.asarray(minv, np.float64)[6:]
    res = b - A @ np.asarray(x, np.float64)[6:]
    return float(np.sqrt((M * res) @ res) / np.sqrt((M * b) @ b))
