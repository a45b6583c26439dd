"""The voxel update (integrateDepthMapKernel<deIntegrate>, CUDASceneRepHashSDF.cu:420-521) restated in float64 numpy, for tests/voxel_update_cases.py.

Written from the definition, per voxel and independent of the kernels' packed forms: every voxel of every allocated block is projected with the float32
inverse pose (the transform the product and the oracle project with), sampled, checked and applied.
  block test   the block-in-frustum test on the block's centre, as tests/test_tsdf_fast_gpu.py::_explain states it;
  in image     hx = x fx / z + mx + 0.5 in (-1, W), hy likewise in (-1, H): the int conversion truncates toward zero, so (-1, 0) is pixel 0;
  validity     the frame has colour, depth is not -inf, depth < m_maxIntegrationDistance, |sdf| < m_truncation + m_truncScale depth (this bound in the
               definition's own float32 operations: it is a comparison between stored float32 values, and the edge cases of voxel_update_cases sit one step from it);
  apply        integrate: colour 0.2 c + 0.8 o (c where the weight is 0), rounded, clamped to [0, 254]; sdf (s + o w) / (1 + w); weight min(weightMax, 1 + w).
               de-integrate: colour (o w - c) / (w - 1) rounded half away from zero, clamped to [0, 254]; sdf (o w - s) / (w - 1); weight max(0, w - 1), and
               the all-zero voxel where that weight is <= 0.001.
The integration weight of a sample is 1 (the definition overwrites its own weightUpdate).
"""
import numpy as np

from bundlefusion_amd.capi import FREE_ENTRY, VOX_PER_BLOCK


def inverse44_f32(T):
    """bf::inverse44 (csrc/bf_device.h) operation by operation in float32: the world -> camera transform both the product and the oracle project voxels with"""
    m = np.asarray(T, np.float32).reshape(16)
    f = np.float32
    adj = np.zeros(16, np.float32)
    for r in range(4):
        for c in range(4):
            rows = [i for i in range(4) if i != c]; cols = [j for j in range(4) if j != r]
            s_ = f(-1.0) if ((r + c) & 1) else f(1.0)
            A = lambda i, j: m[rows[i] * 4 + cols[j]]
            adj[r * 4 + c] = f(f(f(f(f(f(s_ * A(0, 0)) * A(1, 1)) * A(2, 2)) - f(f(f(s_ * A(0, 0)) * A(1, 2)) * A(2, 1))) - f(f(f(s_ * A(1, 0)) * A(0, 1)) * A(2, 2))) +
                                 f(f(f(s_ * A(1, 0)) * A(0, 2)) * A(2, 1)))
            adj[r * 4 + c] = f(f(adj[r * 4 + c] + f(f(f(s_ * A(2, 0)) * A(0, 1)) * A(1, 2))) - f(f(f(s_ * A(2, 0)) * A(0, 2)) * A(1, 1)))
    det = f(f(f(f(m[0] * adj[0]) + f(m[1] * adj[4])) + f(m[2] * adj[8])) + f(m[3] * adj[12]))
    detr = f(f(1.0) / det)
    return (adj * detr).astype(np.float32).reshape(4, 4)


class State:
    """A volume's voxels in float64: sdf [n], weight [n], colour [n, 3] (alpha is 255 where a voxel was ever written and not reset, 0 otherwise)"""

    def __init__(self, vox):
        self.sdf = vox["sdf"].astype(np.float64)
        self.weight = vox["weight"].astype(np.float64)
        self.colour = vox["color"][:, :3].astype(np.float64)
        self.alpha = vox["color"][:, 3].astype(np.int64)


def voxel_index(hash_np):
    """-> (idx [m], coordinates [m, 3] int64, block key [m, 3]) of the voxels of every allocated block, m = 512 x blocks"""
    occ = hash_np[hash_np["ptr"] != FREE_ENTRY]
    pos, ptr = occ["pos"].astype(np.int64), occ["ptr"].astype(np.int64)
    l = np.arange(VOX_PER_BLOCK)
    loc = np.stack([l & 7, (l >> 3) & 7, l >> 6], 1)
    idx = (ptr[:, None] + l[None, :]).reshape(-1)
    coord = (pos[:, None, :] * 8 + loc[None, :, :]).reshape(-1, 3)
    return idx, coord, np.repeat(pos, VOX_PER_BLOCK, axis=0)


def project(coord, key, T, cam, p):
    """-> dict: hx, hy (image coordinates + 0.5), z (camera space), block (the voxel's block passes the frustum test), all float64 from the float32 inverse pose"""
    f32 = np.float32
    vox = f32(p.m_virtualVoxelSize)
    X = (coord.astype(f32) * vox).astype(np.float64)                       # virtualVoxelPosToWorld: one float32 product per axis
    M = inverse44_f32(T).astype(np.float64)
    pc = X @ M[:3, :3].T + M[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        hx = pc[:, 0] * float(cam.fx) / pc[:, 2] + float(cam.mx) + 0.5
        hy = pc[:, 1] * float(cam.fy) / pc[:, 2] + float(cam.my) + 0.5
        BC = (key * 8).astype(f32).astype(np.float64) * float(vox) + float(vox) * 3.5
        bc = BC @ M[:3, :3].T + M[:3, 3]
        W_, H_ = cam.m_imageWidth, cam.m_imageHeight
        zmin, zmax = float(cam.m_sensorDepthWorldMin), float(cam.m_sensorDepthWorldMax)
        bx = (2.0 * (bc[:, 0] * float(cam.fx) / bc[:, 2] + float(cam.mx)) - (W_ - 1.0)) / (W_ - 1.0) * 0.95
        by = ((H_ - 1.0) - 2.0 * (bc[:, 1] * float(cam.fy) / bc[:, 2] + float(cam.my))) / (H_ - 1.0) * 0.95
        bz = (bc[:, 2] - zmin) / (zmax - zmin) * 0.95
        block = ~((bx < -1.0) | (bx > 1.0) | (by < -1.0) | (by > 1.0) | (bz < 0.0) | (bz > 1.0)) & np.isfinite(bx) & np.isfinite(by)
    return dict(hx=hx, hy=hy, z=pc[:, 2], block=block)


def sample(hash_np, T, depth, has_colour, cam, p):
    """The sample of every voxel of every allocated block -> (idx [m], ok [m], sdf [m] float64, pixel (py, px))"""
    idx, coord, key = voxel_index(hash_np)
    pr = project(coord, key, T, cam, p)
    W_, H_ = cam.m_imageWidth, cam.m_imageHeight
    hx, hy = pr["hx"], pr["hy"]
    inimg = pr["block"] & np.isfinite(hx) & np.isfinite(hy) & (hx > -1.0) & (hx < W_) & (hy > -1.0) & (hy < H_)
    px = np.where(inimg, np.trunc(np.where(inimg, hx, 0.0)), 0).astype(np.int64)
    py = np.where(inimg, np.trunc(np.where(inimg, hy, 0.0)), 0).astype(np.int64)
    dep32 = np.ascontiguousarray(depth, np.float32)[py, px]
    dep = dep32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        sdf = dep - pr["z"]
        trunc = (np.float32(p.m_truncation) + np.float32(p.m_truncScale) * dep32).astype(np.float64)      # two float32 operations, as getTruncation
        ok = inimg & bool(has_colour) & (dep32 != -np.inf) & (dep < float(np.float32(p.m_maxIntegrationDistance))) & (np.abs(sdf) < trunc)
    return idx, ok, np.where(ok, sdf, 0.0), (py, px)


def round_half_away(q):
    return np.sign(q) * np.floor(np.abs(q) + 0.5)


def apply(kind, st, idx, ok, sdf, col, weight_max):
    """voxelApply on the voxels idx[ok] of `st` (in place); col [m, 3] float64: the sample's colour"""
    i = idx[ok]
    s, c = sdf[ok], col[ok]
    so, wo, co = st.sdf[i], st.weight[i], st.colour[i]
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "in":
            first = (wo == 0)[:, None]
            cn = np.clip(round_half_away(np.where(first, c, 0.2 * c + 0.8 * co)), 0.0, 254.0)
            sn = (s + so * wo) / (1.0 + wo)
            wn = np.minimum(float(weight_max), 1.0 + wo)
            an = np.full(len(i), 255)
        else:
            den = wo - 1.0
            q = (co * wo[:, None] - c) / den[:, None]
            cn = np.clip(np.nan_to_num(round_half_away(q), nan=0.0, posinf=254.0, neginf=0.0), 0.0, 254.0)
            sn = (so * wo - s) / den
            wn = np.maximum(0.0, den)
            dead = wn <= 0.001
            cn = np.where(dead[:, None], 0.0, cn); sn = np.where(dead, 0.0, sn); wn = np.where(dead, 0.0, wn)
            an = np.where(dead, 0, 255)
    st.sdf[i], st.weight[i], st.colour[i], st.alpha[i] = sn, wn, cn, an


def run(kind, st, hash_np, T, depth, colour, cam, p):
    """One operator ("in" / "de") on the state, over the blocks of hash_np (the table the operator's update pass sees: after its allocation).
    -> (idx, ok): the voxels of allocated blocks and which of them the operator updated"""
    idx, ok, sdf, (py, px) = sample(hash_np, T, depth, colour is not None, cam, p)
    col = np.zeros((len(idx), 3)) if colour is None else np.ascontiguousarray(colour)[py, px, :3].astype(np.float64)
    apply(kind, st, idx, ok, sdf, col, p.m_integrationWeightMax)
    return idx, ok
