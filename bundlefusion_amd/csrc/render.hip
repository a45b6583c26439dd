// The reconstruction as a picture for gfx950: DX11RGBDRenderer::RenderDepthMap (Shaders/RGBDRenderer.hlsl), DX11PhongLighting::render (Shaders/PhongLighting.hlsl:
// PhongPS) and DX11QuadDrawer::RenderQuad without Direct3D.  The reference's view matrix is the identity, so mesh vertex (x, y) lands on pixel (x, y) and its
// three passes are one pass per pixel - DESIGN.md "Frame rendering" states the definition and its departure; tests/render_ref.py is the same in numpy, and the two
// are compared as bits.
//   k_render_shade      a 64x4 tile of pixels per workgroup, one lane per pixel.  The tile's depths with a one-pixel halo (66 x 6: the normals' four neighbours
//                       and the quads' far corners) go into LDS once, and each vertex's camera-space position is formed once there, not five times per pixel.
//                       Row stride 67 words: odd, so the lanes of a wave read consecutive banks.  Colours and the float target move as 16-byte vectors.
//                       What does not depend on the pixel (the light direction, the products of light and material) is computed once on the host.
//   k_render_depth_hsv  depthToHSVDevice + presentation, k_render_rgbx: one pass each.
// All arithmetic is binary32 op by op (-ffp-contract=off, IEEE division and square root); pow is bf_dm_pow of include/bf_detmath.h.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/bf_detmath.h"
#include "../../include/bf_render.h"
#include "bf_device.h"
#include "bf_resources.h"

using namespace bf;

struct bf_frame_renderer {
    uint32_t width = 0, height = 0;
    float4* d_target = nullptr;
    uint32_t* d_rgba = nullptr;
    hipStream_t stream = nullptr;
    bf::Resources res;
};

namespace {

constexpr int TW = 64, TH = 4;                        // pixels per tile
constexpr int VW = TW + 2, VH = TH + 2;               // with the halo
constexpr int VS = VW + 1;                            // row stride in words (odd)
constexpr float Z_NEAR = 0.1f;                        // DEPTH_WORLD_MIN of the shader
constexpr uint32_t QNAN_BITS = 0x7fc00000u;

struct ShadeArgs {
    float k0[4], k1[4], k3[4];                        // rows 0, 1 and 3 of the inverse intrinsics
    float i[3];                                       // -normalize(lightDir)
    float A[4], D[4], S[4];                           // useMaterial: the light's ambient / diffuse / specular; otherwise their products with the material's
    float shininess, threshOffset, threshLin;
    int w, h, useMaterial, overlay;
};

BF_DEV float dot4(const float* m, float a, float b, float c, float d) { return ((m[0] * a + m[1] * b) + m[2] * c) + m[3] * d; }
BF_DEV float dot3v(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
BF_DEV float len3(f3 v) { return bf_dm_sqrt((v.x * v.x + v.y * v.y) + v.z * v.z); }
BF_DEV f3 normalize3(f3 v) { const float l = len3(v); return mk3(v.x / l, v.y / l, v.z / l); }
BF_DEV bool depthOk(float d) { return d > Z_NEAR && d < BF_PINF; }           // false for <= 0.1, -inf, +inf and NaN
BF_DEV bool finite(float d) { return fabsf(d) < BF_PINF; }                    // false for NaN too
BF_DEV float max0(float a) { return a > 0.0f ? a : 0.0f; }                    // NaN -> 0
BF_DEV float canon(float v) { return v != v ? __uint_as_float(QNAN_BITS) : v; }

// QuadPS3 + the copy to an R8G8B8A8 target: (uint8)(int)(min(max(c, 0), 1) * 255 + 0.5), NaN -> 0
BF_DEV uint32_t quant(float c) {
    float v = max0(c);
    v = v < 1.0f ? v : 1.0f;
    return (uint32_t)(int)(v * 255.0f + 0.5f);
}
// r, g, b quantised; alpha 255 where one of them is above 0 (renderToFile, DepthSensing.cpp:1183-1186)
BF_DEV uint32_t present(float r, float g, float b) {
    const uint32_t R = quant(r), G = quant(g), B = quant(b);
    const uint32_t rgb = R | (G << 8) | (B << 16);
    return rgb ? (rgb | 0xff000000u) : 0u;
}

__global__ __launch_bounds__(256) void k_render_shade(float4* __restrict__ target, uint32_t* __restrict__ rgba, const float* __restrict__ depth,
                                                      const float4* __restrict__ colors, ShadeArgs A) {
    __shared__ float sD[VH * VS], sX[VH * VS], sY[VH * VS], sZ[VH * VS];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    for (int t = threadIdx.y * TW + threadIdx.x; t < VH * VW; t += TW * TH) {
        const int ly = t / VW, lx = t - ly * VW, x = x0 - 1 + lx, y = y0 - 1 + ly;
        const bool in = x >= 0 && y >= 0 && x < A.w && y < A.h;
        const float d = in ? depth[(size_t)y * A.w + x] : 0.0f;                 // a corner outside the image reads 0
        const float dp = finite(d) ? d : 0.0f;                                  // (a position nobody uses)
        const float xd = (float)x * dp, yd = (float)y * dp;
        const int o = ly * VS + lx;
        sD[o] = d;
        sX[o] = dot4(A.k0, xd, yd, dp, dp); sY[o] = dot4(A.k1, xd, yd, dp, dp); sZ[o] = dot4(A.k3, xd, yd, dp, dp);
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    const size_t idx = (size_t)y * A.w + x;
    const float4 col = colors[idx];
    const int c = (threadIdx.y + 1) * VS + threadIdx.x + 1;                     // this pixel; c - 1 / c + 1 / c - VS / c + VS: its neighbours
    bool drawn = false;
    f3 n = mk3(0.0f, 0.0f, 0.0f);
    {
        // the quad stage (RGBDRendererGS): quad (x, y) has the corners (x, y) (x, y+1) (x+1, y) (x+1, y+1)
        const float d0 = sD[c], d1 = sD[c + VS], d2 = sD[c + 1], d3 = sD[c + VS + 1];
        bool ok = depthOk(d0) && depthOk(d1) && depthOk(d2) && depthOk(d3);
        const float dmax = fmaxf(fmaxf(d0, d1), fmaxf(d2, d3)), dmin = fminf(fminf(d0, d1), fminf(d2, d3));
        ok = ok && !(dmax - dmin > A.threshOffset + A.threshLin * (0.5f * (dmax + dmin)));
        // the normal's neighbours: inside the image and finite (the departure from the shader)
        ok = ok && x > 0 && y > 0 && x + 1 < A.w && y + 1 < A.h;
        ok = ok && finite(sD[c - 1]) && finite(sD[c - VS]);                      // (x+1, y) and (x, y+1) passed depthOk
        ok = ok && !(col.x == BF_MINF);
        if (ok) {
            const f3 a = mk3(sX[c + VS] - sX[c - VS], sY[c + VS] - sY[c - VS], sZ[c + VS] - sZ[c - VS]);      // P(x, y+1) - P(x, y-1)
            const f3 b = mk3(sX[c + 1] - sX[c - 1], sY[c + 1] - sY[c - 1], sZ[c + 1] - sZ[c - 1]);            // P(x+1, y) - P(x-1, y)
            const f3 nr = mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
            const float l = len3(nr);
            if (l > 0.0f && l < BF_PINF) { drawn = true; n = mk3(nr.x / l, nr.y / l, nr.z / l); }
        }
    }
    if (!drawn) {
        target[idx] = make_float4(BF_MINF, BF_MINF, BF_MINF, BF_MINF);
        rgba[idx] = 0u;
        return;
    }
    // PhongPS
    n = normalize3(n);
    const f3 eye = normalize3(mk3(sX[c], sY[c], sZ[c]));
    const f3 i = mk3(A.i[0], A.i[1], A.i[2]);
    const float ndl = dot3v(n, i);
    const float two = 2.0f * ndl;
    const f3 R = normalize3(mk3(i.x - two * n.x, i.y - two * n.y, i.z - two * n.z));      // reflect(-L, n)
    const float spec = bf_dm_pow(max0(dot3v(R, eye)), A.shininess);
    float rx, ry, rz, rw;
    if (A.useMaterial) {
        const float andl = fabsf(ndl);
        const float dx = bf_dm_pow((A.D[0] * col.x) * andl, 1.2f), dy = bf_dm_pow((A.D[1] * col.y) * andl, 1.2f), dz = bf_dm_pow((A.D[2] * col.z) * andl, 1.2f);
        rx = (((A.A[0] * col.x) * 0.5f + 1.2f * dx) + 0.8f * ((A.S[0] * col.x) * spec)) * 1.2f;
        ry = (((A.A[1] * col.y) * 0.5f + 1.2f * dy) + 0.8f * ((A.S[1] * col.y) * spec)) * 1.2f;
        rz = (((A.A[2] * col.z) * 0.5f + 1.2f * dz) + 0.8f * ((A.S[2] * col.z) * spec)) * 1.2f;
        rw = 1.0f;
    } else {
        const float mdl = max0(ndl);
        rx = (A.A[0] + A.D[0] * mdl) + A.S[0] * spec;
        ry = (A.A[1] + A.D[1] * mdl) + A.S[1] * spec;
        rz = (A.A[2] + A.D[2] * mdl) + A.S[2] * spec;
        rw = (A.A[3] + A.D[3] * mdl) + A.S[3] * spec;
    }
    if (A.overlay) { rx = rz; ry = rz; }                                         // g_overlayColor.x == -1: tracking lost, grey
    rx = canon(rx); ry = canon(ry); rz = canon(rz); rw = canon(rw);
    target[idx] = make_float4(rx, ry, rz, rw);
    rgba[idx] = present(rx, ry, rz);
}

// depthToHSVDevice / convertDepthToRGB / convertHSVToRGB (CameraUtil.cu:1633-1699), H in degrees, S = 1, V = 0.5
__global__ __launch_bounds__(256) void k_render_depth_hsv(float4* __restrict__ target, uint32_t* __restrict__ rgba, const float* __restrict__ depth, uint32_t n,
                                                          float dmin, float dmax) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n) return;
    const float d = depth[idx];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (d != BF_MINF && d != 0.0f && d >= dmin && d <= dmax) {
        float x = 1.0f - (d - dmin) / (dmax - dmin);
        if (x < 0.0f) x = 0.0f;
        if (x > 1.0f) x = 1.0f;
        x = 360.0f * x - 120.0f;
        if (x < 0.0f) x += 359.0f;
        const float hd = x / 60.0f;
        const uint32_t h = f2u(hd);
        const float f = hd - (float)h;
        const float V = 0.5f, S = 1.0f;
        const float p = V * (1.0f - S), q = V * (1.0f - S * f), t = V * (1.0f - S * (1.0f - f));
        if (h == 0u || h == 6u) o = make_float4(V, t, p, 1.0f);
        else if (h == 1u) o = make_float4(q, V, p, 1.0f);
        else if (h == 2u) o = make_float4(p, V, t, 1.0f);
        else if (h == 3u) o = make_float4(p, q, V, 1.0f);
        else if (h == 4u) o = make_float4(t, p, V, 1.0f);
        else o = make_float4(V, p, q, 1.0f);
        o.x = canon(o.x); o.y = canon(o.y); o.z = canon(o.z);
    }
    target[idx] = o;
    rgba[idx] = present(o.x, o.y, o.z);
}

__global__ __launch_bounds__(256) void k_render_rgbx(uint32_t* __restrict__ rgba, const uint32_t* __restrict__ rgbx, uint32_t n) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx < n) rgba[idx] = rgbx[idx] | 0xff000000u;
}

void normalizeHost(const float v[3], float out[3]) {
    const float l = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    out[0] = v[0] / l; out[1] = v[1] / l; out[2] = v[2] / l;
}

}  // namespace

extern "C" {

int bf_ray_cast_intrinsics_inv(const bf_ray_cast_params* p, float out[16]) {
    BF_REQUIRE(p && out, "null argument");
    for (int k = 0; k < 16; ++k) out[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    out[0] = 1.0f / p->fx; out[2] = -p->mx / p->fx;
    out[5] = 1.0f / p->fy; out[6] = -p->my / p->fy;
    return BF_OK;
}

int bf_frame_renderer_create(uint32_t width, uint32_t height, bf_frame_renderer** out) {
    BF_REQUIRE(out && width > 0 && height > 0 && width < 32768 && height < 32768, "bad image size");
    bf_frame_renderer* r = new bf_frame_renderer;
    bf::CreateGuard<bf_frame_renderer> guard(r, bf_frame_renderer_destroy);
    r->width = width; r->height = height;
    const size_t n = (size_t)width * height;
    BF_TRY(r->res.device(&r->d_target, n));
    BF_TRY(r->res.device(&r->d_rgba, n));
    *out = guard.dismiss();
    return BF_OK;
}

int bf_frame_renderer_destroy(bf_frame_renderer* r) {
    if (!r) return BF_OK;
    (void)hipStreamSynchronize(r->stream);
    delete r;
    return BF_OK;
}

int bf_frame_renderer_set_stream(bf_frame_renderer* r, void* s) { BF_REQUIRE(r, "null renderer"); r->stream = (hipStream_t)s; return BF_OK; }

int bf_frame_renderer_shade(bf_frame_renderer* r, const float* d_depth, const float* d_colors, const float Kinv[16], const bf_render_state* st, int useMaterial,
                            int trackingLost, float threshOffset, float threshLin) {
    BF_REQUIRE(r && d_depth && d_colors && Kinv && st, "null argument");
    ShadeArgs A;
    memcpy(A.k0, Kinv + 0, 16); memcpy(A.k1, Kinv + 4, 16); memcpy(A.k3, Kinv + 12, 16);
    float L[3];
    normalizeHost(st->s_lightDirection, L);
    for (int k = 0; k < 3; ++k) A.i[k] = -L[k];
    for (int k = 0; k < 4; ++k) {
        if (useMaterial) { A.A[k] = st->s_lightAmbient[k]; A.D[k] = st->s_lightDiffuse[k]; A.S[k] = st->s_lightSpecular[k]; }
        else { A.A[k] = st->s_lightAmbient[k] * st->s_materialAmbient[k]; A.D[k] = st->s_lightDiffuse[k] * st->s_materialDiffuse[k]; A.S[k] = st->s_lightSpecular[k] * st->s_materialSpecular[k]; }
    }
    A.shininess = st->s_materialShininess; A.threshOffset = threshOffset; A.threshLin = threshLin;
    A.w = (int)r->width; A.h = (int)r->height; A.useMaterial = useMaterial ? 1 : 0; A.overlay = trackingLost ? 1 : 0;
    k_render_shade<<<dim3(div_up(r->width, TW), div_up(r->height, TH)), dim3(TW, TH), 0, r->stream>>>(r->d_target, r->d_rgba, d_depth, (const float4*)d_colors, A);
    BF_HIP_TRY(hipGetLastError());
    return BF_OK;
}

int bf_frame_renderer_depth_hsv(bf_frame_renderer* r, const float* d_depth, float minDepth, float maxDepth) {
    BF_REQUIRE(r && d_depth, "null argument");
    const uint32_t n = r->width * r->height;
    k_render_depth_hsv<<<div_up(n, 256), 256, 0, r->stream>>>(r->d_target, r->d_rgba, d_depth, n, minDepth, maxDepth);
    BF_HIP_TRY(hipGetLastError());
    return BF_OK;
}

int bf_frame_renderer_rgbx(bf_frame_renderer* r, const uint8_t* d_rgbx) {
    BF_REQUIRE(r && d_rgbx, "null argument");
    const uint32_t n = r->width * r->height;
    k_render_rgbx<<<div_up(n, 256), 256, 0, r->stream>>>(r->d_rgba, (const uint32_t*)d_rgbx, n);
    BF_HIP_TRY(hipGetLastError());
    return BF_OK;
}

int bf_frame_renderer_get_images(bf_frame_renderer* r, const float** d_target, const uint8_t** d_rgba8) {
    BF_REQUIRE(r, "null renderer");
    if (d_target) *d_target = (const float*)r->d_target;
    if (d_rgba8) *d_rgba8 = (const uint8_t*)r->d_rgba;
    return BF_OK;
}

int bf_frame_renderer_download_rgba8(bf_frame_renderer* r, uint8_t* h_out) {
    BF_REQUIRE(r && h_out, "null argument");
    BF_HIP_TRY(hipMemcpyAsync(h_out, r->d_rgba, (size_t)r->width * r->height * 4, hipMemcpyDeviceToHost, r->stream));
    BF_HIP_TRY(hipStreamSynchronize(r->stream));
    return BF_OK;
}

}  // extern "C"
