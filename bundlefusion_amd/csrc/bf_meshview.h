// One (point, frame) pair of the passes that take colour from the key frames - the recolouring of the vertices (meshrecolour.hip) and the texture atlas
// (meshtexture.hip): the frame table as the kernels read it and rules 2 - 6 of include/bf_hip.h's definition next to bf_marching_cubes_recolour, one copy for both
// passes, for the kernels and for the one-core routes alike (the library is built without contraction: one rounding per operation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/bf_hip.h"
#include "bf_device.h"

namespace bf {

// one frame as the kernels read it: the images, rows 0 - 2 of mesh to camera, the camera centre (80 bytes; indexed by a loop counter
// alone, so every lane reads the same address and the compiler fetches it through the scalar path)
struct RcFrame { const float* depth; const uint8_t* color; float W[12]; float o[3]; float pad; };
struct RcCamera { float fx, fy, cx, cy; int w, h; };
struct RcView { float wgt, val[3]; };

BF_HD bool finiteF(float x) { return x > BF_MINF && x < BF_PINF; }          // (a NaN fails both comparisons)
BF_HD float bilinear(uint32_t c00, uint32_t c10, uint32_t c01, uint32_t c11, int shift, float a, float b) {
    const float f00 = (float)((c00 >> shift) & 0xFFu), f10 = (float)((c10 >> shift) & 0xFFu), f01 = (float)((c01 >> shift) & 0xFFu), f11 = (float)((c11 >> shift) & 0xFFu);
    const float top = f00 + a * (f10 - f00), bot = f01 + a * (f11 - f01);
    return top + b * (bot - top);
}
// rules 2 - 6 of one (point, frame) pair whose point passed rule 1: the pair's code; a view's weight and sample in `view`.  Params: bf_mesh_recolour_params or
// bf_mesh_texture_params (the five floats they share)
template <typename Params>
BF_HD uint32_t pairOf(f3 P, f3 N, const RcFrame& f, const RcCamera& cam, const Params& p, RcView& view) {
    const float p0 = ((f.W[0] * P.x + f.W[1] * P.y) + f.W[2] * P.z) + f.W[3] * 1.0f;
    const float p1 = ((f.W[4] * P.x + f.W[5] * P.y) + f.W[6] * P.z) + f.W[7] * 1.0f;
    const float z = ((f.W[8] * P.x + f.W[9] * P.y) + f.W[10] * P.z) + f.W[11] * 1.0f;
    if (!(z >= p.depthMin && z <= p.depthMax)) return BF_RECOLOUR_RANGE;
    const float u = (p0 * cam.fx) / z + cam.cx, v = (p1 * cam.fy) / z + cam.cy;
    if (!(u >= 0.0f && u < (float)(cam.w - 1) && v >= 0.0f && v < (float)(cam.h - 1))) return BF_RECOLOUR_IMAGE;
    const int x0 = (int)u, y0 = (int)v;
    const float a = u - (float)x0, b = v - (float)y0;
    const f3 c = mk3(f.o[0] - P.x, f.o[1] - P.y, f.o[2] - P.z);
    const float l = __builtin_sqrtf((c.x * c.x + c.y * c.y) + c.z * c.z);
    if (!(l > 0.0f && l < BF_PINF)) return BF_RECOLOUR_FACING;
    const float cosv = BF_RECOLOUR_NORMAL_SIGN * (((N.x * c.x + N.y * c.y) + N.z * c.z) / l);
    if (!(cosv >= p.minCos)) return BF_RECOLOUR_FACING;
    const float tol = p.depthTolerance + p.depthToleranceLin * z;
    const size_t i00 = (size_t)y0 * (size_t)cam.w + (size_t)x0, i01 = i00 + (size_t)cam.w;          // x0 + 1 <= w - 1 and y0 + 1 <= h - 1: rule 3
    const float d00 = f.depth[i00], d10 = f.depth[i00 + 1], d01 = f.depth[i01], d11 = f.depth[i01 + 1];
    if (!(finiteF(d00) && d00 > 0.0f && fabsf(d00 - z) <= tol)) return BF_RECOLOUR_OCCLUDED;
    if (!(finiteF(d10) && d10 > 0.0f && fabsf(d10 - z) <= tol)) return BF_RECOLOUR_OCCLUDED;
    if (!(finiteF(d01) && d01 > 0.0f && fabsf(d01 - z) <= tol)) return BF_RECOLOUR_OCCLUDED;
    if (!(finiteF(d11) && d11 > 0.0f && fabsf(d11 - z) <= tol)) return BF_RECOLOUR_OCCLUDED;
    const uint32_t* __restrict__ px = reinterpret_cast<const uint32_t*>(f.color);                   // RGBX8, little-endian: r | g << 8 | b << 16
    const uint32_t c00 = px[i00], c10 = px[i00 + 1], c01 = px[i01], c11 = px[i01 + 1];
    if (!(c00 & 0xFFFFFFu) || !(c10 & 0xFFFFFFu) || !(c01 & 0xFFFFFFu) || !(c11 & 0xFFFFFFu)) return BF_RECOLOUR_COLOUR;
    view.wgt = (cosv * cosv) / (z * z);
    view.val[0] = bilinear(c00, c10, c01, c11, 0, a, b);
    view.val[1] = bilinear(c00, c10, c01, c11, 8, a, b);
    view.val[2] = bilinear(c00, c10, c01, c11, 16, a, b);
    return BF_RECOLOUR_VIEW;
}

inline RcCamera cameraOf(const float* K, uint32_t w, uint32_t h) { RcCamera c; c.fx = K[0]; c.fy = K[5]; c.cx = K[2]; c.cy = K[6]; c.w = (int)w; c.h = (int)h; return c; }
inline RcFrame frameOf(const bf_mesh_recolour_frame& f) {
    RcFrame r; r.depth = f.d_depth; r.color = f.d_colorRGBX; memcpy(r.W, f.meshToCamera, sizeof r.W); memcpy(r.o, f.cameraCentre, sizeof r.o); r.pad = 0.0f;
    return r;
}

}  // namespace bf
