// The point-cloud accumulator (pointcloud.hip): the object behind include/bf_pointcloud.h and the per-pixel arithmetic of its definition (DESIGN.md 1 "Point
// cloud"), written once for the kernel and for the host route.  Binary32 op by op (-ffp-contract=off), IEEE division and square root.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bf_pointcloud.h"
#include "bf_device.h"
#include "bf_resources.h"

namespace bf {

// what does not depend on the pixel: rows 0 - 2 of the inverse intrinsics and of the pose, the depth gate and the thinning's 1.0 / (double)cellSize
struct PcFrame {
    float k[12], t[12];
    float maxDepth;
    int thin;
    double inv;
    int w, h;
};

struct PcPoint { f3 P, N; uint32_t rgba; };

BF_HD float pcDot(const float* r, float a, float b, float c, float d) { return ((r[0] * a + r[1] * b) + r[2] * c) + r[3] * d; }
BF_HD bool pcFinite(float v) { return fabsf(v) < BF_PINF; }                          // false for NaN too
BF_HD bool pcHasPosition(float d) { return d > 0.0f && d < BF_PINF; }                 // false for -inf, +inf, NaN, 0 and negative depths
// depthToCamera (SiftVisualization.cpp:498-503) with the whole inverse matrix
BF_HD f3 pcPosition(const PcFrame& F, int x, int y, float d) {
    const float xd = (float)x * d, yd = (float)y * d;
    return mk3(pcDot(F.k, xd, yd, d, 1.0f), pcDot(F.k + 4, xd, yd, d, 1.0f), pcDot(F.k + 8, xd, yd, d, 1.0f));
}
BF_HD long long pcCell(float P, double inv) { return (long long)floor((double)P * inv); }
// the gates that follow "five positions and an interior pixel" (getNormal :505-525, computePointCloud :536-560).  texel: the RGBX8 colour, r in the low byte
BF_HD bool pcCandidate(const PcFrame& F, f3 p, f3 xm, f3 xp, f3 ym, f3 yp, uint32_t texel, PcPoint& out) {
    if (!(p.z < F.maxDepth)) return false;
    const f3 a = xp - xm, b = yp - ym;
    const f3 n = cross3(a, b);
    const float l = __builtin_sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z);
    if (!(l > 0.0f && l < BF_PINF)) return false;
    if ((texel & 0x00ffffffu) == 0u) return false;
    const float ml = -l;
    const f3 nn = mk3(n.x / ml, n.y / ml, n.z / ml);
    out.P = mk3(pcDot(F.t, p.x, p.y, p.z, 1.0f), pcDot(F.t + 4, p.x, p.y, p.z, 1.0f), pcDot(F.t + 8, p.x, p.y, p.z, 1.0f));
    if (!(pcFinite(out.P.x) && pcFinite(out.P.y) && pcFinite(out.P.z))) return false;
    if (F.thin) {
        const double lo = -2147483648.0, hi = 2147483647.0;
        const double cx = floor((double)out.P.x * F.inv), cy = floor((double)out.P.y * F.inv), cz = floor((double)out.P.z * F.inv);
        if (!(cx >= lo && cx <= hi && cy >= lo && cy <= hi && cz >= lo && cz <= hi)) return false;
    }
    out.N = mk3((F.t[0] * nn.x + F.t[1] * nn.y) + F.t[2] * nn.z, (F.t[4] * nn.x + F.t[5] * nn.y) + F.t[6] * nn.z, (F.t[8] * nn.x + F.t[9] * nn.y) + F.t[10] * nn.z);
    out.rgba = (texel & 0x00ffffffu) | 0xff000000u;
    return true;
}

}  // namespace bf

struct bf_point_cloud {
    bf_point_cloud_params params;
    double inv = 0.0;                    // 1.0 / (double)cellSize
    bool thin = false;
    uint32_t slots = 0;                  // of the cell table, a power of two
    // per frame: one staging record (two float4) per pixel, per pixel the table slot it owns (or NONE), per tile of 1024 pixels its count / offset, the frame's total
    float4* d_stage = nullptr; uint32_t *d_own = nullptr, *d_tiles = nullptr, *d_total = nullptr;
    uint32_t* d_table = nullptr;
    float *d_positions = nullptr, *d_normals = nullptr; uint32_t* d_colors = nullptr;
    uint32_t numPoints = 0;
    bool overflowed = false;
    hipStream_t stream = nullptr;
    bf::Resources res;
};
