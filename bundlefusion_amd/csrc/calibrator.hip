// Depth-to-colour registration for gfx950: CUDAImageCalibrator (CUDAImageCalibrator.h/.cpp) without Direct3D.  The reference renders the depth image as a
// triangle mesh into the colour camera (DX11RGBDRenderer::RenderDepthMap, Shaders/RGBDRenderer.hlsl); this is a rasteriser with a definition of its
// own that follows that shader stage by stage - DESIGN.md "Depth registration" states it, its three departures and why.  tests/calibrator_ref.py is the
// same definition in numpy, and the two are compared as bits.
//   k_calib_raster    a 64x4 tile of quads per workgroup, one lane per quad.  The (64+1) x (4+1) vertices of the tile are projected ONCE each into LDS
//                     (a vertex belongs to four quads = six triangles), then every lane tests its quad, sets up its two triangles from LDS and walks
//                     their bounding boxes (a pixel or two each at sensor baselines), resolving the per-pixel minimum with a 32-bit atomicMin on the
//                     float's bits (all values are positive floats, which order as unsigned integers) in a scratch plane armed to +inf.
//   k_calib_resolve   scratch -> the depth image (+inf -> -inf) and re-arms the scratch: two launches per frame, no memset.
// All arithmetic is binary32 op by op (-ffp-contract=off, IEEE division) up to the 1/256-pixel snap; coverage and the edge functions are integers.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bf_device.h"
#include "bf_resources.h"

using namespace bf;

struct bf_image_calibrator {
    uint32_t width = 0, height = 0;
    uint32_t* d_scratch = nullptr;          // width * height words; +inf (as bits) between frames
    hipStream_t stream = nullptr;
    bf::Resources res;
};

namespace {

constexpr int TW = 64, TH = 4;                       // quads per tile
constexpr int VW = TW + 1, VH = TH + 1;              // vertices per tile (row stride 65 words: lanes of a wave read consecutive banks)
constexpr uint32_t PINF_BITS = 0x7f800000u;
constexpr float Z_NEAR = 0.1f, Z_FAR = 20.0f;        // DEPTH_WORLD_MIN / DEPTH_WORLD_MAX of the shader
constexpr float UV_LIMIT = 1048576.0f;               // a vertex farther than 2^20 pixels from the origin is not drawn (keeps the snapped coordinates in 29 bits)

struct CalibArgs { m44 Kc, KdInv, E; float threshOffset, threshLin; int w, h; };

struct Vtx { int U, V; float z; bool ok; };

// ((m0 a + m1 b) + m2 c) + m3 d: the row-times-vector order of the shader's mul()
BF_DEV float dot4(const float* m, float a, float b, float c, float d) { return ((m[0] * a + m[1] * b) + m[2] * c) + m[3] * d; }

BF_DEV bool depthOk(float d) { return d > Z_NEAR && d < BF_PINF; }      // false for <= 0.1, -inf, +inf and NaN

// getWorldSpacePosition / ComputeQuadVertex: pixel (x, y) at depth d -> 1/256-pixel position and depth in the colour camera
BF_DEV Vtx projectVertex(const CalibArgs& A, int x, int y, float d) {
    Vtx v; v.U = v.V = 0; v.z = 0.0f; v.ok = false;
    if (!depthOk(d)) return v;
    const float xd = (float)x * d, yd = (float)y * d;
    const float px = dot4(A.KdInv.e + 0, xd, yd, d, d), py = dot4(A.KdInv.e + 4, xd, yd, d, d), pz = dot4(A.KdInv.e + 12, xd, yd, d, d);
    const float ex = dot4(A.E.e + 0, px, py, pz, 1.0f), ey = dot4(A.E.e + 4, px, py, pz, 1.0f), ez = dot4(A.E.e + 8, px, py, pz, 1.0f), ew = dot4(A.E.e + 12, px, py, pz, 1.0f);
    const float wx = ex / ew, wy = ey / ew, wz = ez / ew;
    const float qx = dot4(A.Kc.e + 0, wx, wy, wz, 1.0f), qy = dot4(A.Kc.e + 4, wx, wy, wz, 1.0f), qz = dot4(A.Kc.e + 8, wx, wy, wz, 1.0f);
    const float u = qx / qz, vv = qy / qz;
    if (!(qz > Z_NEAR && qz < Z_FAR && fabsf(u) < UV_LIMIT && fabsf(vv) < UV_LIMIT)) return v;      // NaN fails every comparison
    v.U = (int)floorf(u * 256.0f + 0.5f);
    v.V = (int)floorf(vv * 256.0f + 0.5f);
    v.z = qz;
    v.ok = true;
    return v;
}

BF_DEV int64_t edgeFn(int aU, int aV, int bU, int bV, int pU, int pV) {
    return (int64_t)(bU - aU) * (int64_t)(pV - aV) - (int64_t)(bV - aV) * (int64_t)(pU - aU);
}
// an edge a -> b of a triangle of positive area (y down) owns the pixels exactly on it when it is a left edge (dV < 0) or a top edge (dV == 0, dU > 0)
BF_DEV bool topLeft(int aU, int aV, int bU, int bV) { const int dU = bU - aU, dV = bV - aV; return dV < 0 || (dV == 0 && dU > 0); }

BF_DEV int floorDiv256(int a) { return a >> 8; }                 // arithmetic shift: floor for negative values too
BF_DEV int ceilDiv256(int a) { return (a + 255) >> 8; }

BF_DEV void rasterTriangle(uint32_t* __restrict__ scratch, int w, int h, const Vtx& a, const Vtx& b, const Vtx& c) {
    if (!(a.ok && b.ok && c.ok)) return;
    const int64_t area2 = edgeFn(a.U, a.V, b.U, b.V, c.U, c.V);
    if (area2 <= 0) return;                                     // turned away from the camera (the source orientation is positive), or empty
    const int i0 = max(ceilDiv256(min(a.U, min(b.U, c.U))), 0), i1 = min(floorDiv256(max(a.U, max(b.U, c.U))), w - 1);
    const int j0 = max(ceilDiv256(min(a.V, min(b.V, c.V))), 0), j1 = min(floorDiv256(max(a.V, max(b.V, c.V))), h - 1);
    const bool tl0 = topLeft(b.U, b.V, c.U, c.V), tl1 = topLeft(c.U, c.V, a.U, a.V), tl2 = topLeft(a.U, a.V, b.U, b.V);
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) {                        // i, j inside the image: the only addresses written
            const int pU = i * 256, pV = j * 256;
            const int64_t e0 = edgeFn(b.U, b.V, c.U, c.V, pU, pV), e1 = edgeFn(c.U, c.V, a.U, a.V, pU, pV), e2 = edgeFn(a.U, a.V, b.U, b.V, pU, pV);
            if ((e0 > 0 || (e0 == 0 && tl0)) && (e1 > 0 || (e1 == 0 && tl1)) && (e2 > 0 || (e2 == 0 && tl2))) {
                const float f0 = (float)e0, f1 = (float)e1, f2 = (float)e2;
                const float val = ((f0 * a.z + f1 * b.z) + f2 * c.z) / ((f0 + f1) + f2);
                atomicMin(scratch + (size_t)j * w + i, __float_as_uint(val));
            }
        }
}

__global__ __launch_bounds__(256) void k_calib_raster(uint32_t* __restrict__ scratch, const float* __restrict__ depth, CalibArgs A) {
    __shared__ float sD[VH * VW];
    __shared__ float sZ[VH * VW];
    __shared__ int sU[VH * VW], sV[VH * VW];                    // sU == INT_MIN: the vertex is not drawn
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    for (int t = threadIdx.y * TW + threadIdx.x; t < VH * VW; t += TW * TH) {
        const int ly = t / VW, lx = t - ly * VW, x = x0 + lx, y = y0 + ly;
        const float d = (x < A.w && y < A.h) ? depth[(size_t)y * A.w + x] : 0.0f;       // a corner outside the image reads 0
        const Vtx v = projectVertex(A, x, y, d);
        sD[t] = d; sZ[t] = v.z; sU[t] = v.ok ? v.U : INT_MIN; sV[t] = v.V;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    const int t00 = threadIdx.y * VW + threadIdx.x, t01 = t00 + VW, t10 = t00 + 1, t11 = t01 + 1;     // t<dx><dy>
    const float d0 = sD[t00], d1 = sD[t01], d2 = sD[t10], d3 = sD[t11];
    if (!(depthOk(d0) && depthOk(d1) && depthOk(d2) && depthOk(d3))) return;
    const float dmax = fmaxf(fmaxf(d0, d1), fmaxf(d2, d3)), dmin = fminf(fminf(d0, d1), fminf(d2, d3));
    if (dmax - dmin > A.threshOffset + A.threshLin * (0.5f * (dmax + dmin))) return;
    Vtx v00, v01, v10, v11;
    v00.U = sU[t00]; v00.V = sV[t00]; v00.z = sZ[t00]; v00.ok = v00.U != INT_MIN;
    v01.U = sU[t01]; v01.V = sV[t01]; v01.z = sZ[t01]; v01.ok = v01.U != INT_MIN;
    v10.U = sU[t10]; v10.V = sV[t10]; v10.z = sZ[t10]; v10.ok = v10.U != INT_MIN;
    v11.U = sU[t11]; v11.V = sV[t11]; v11.z = sZ[t11]; v11.ok = v11.U != INT_MIN;
    rasterTriangle(scratch, A.w, A.h, v01, v00, v11);           // (x, y+1) (x, y) (x+1, y+1)
    rasterTriangle(scratch, A.w, A.h, v11, v00, v10);           // (x+1, y+1) (x, y) (x+1, y)
}

__global__ __launch_bounds__(256) void k_calib_resolve(float* __restrict__ depth, uint32_t* __restrict__ scratch, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = scratch[i];
    depth[i] = b == PINF_BITS ? BF_MINF : __uint_as_float(b);
    scratch[i] = PINF_BITS;
}

__global__ __launch_bounds__(256) void k_calib_arm(uint32_t* __restrict__ scratch, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) scratch[i] = PINF_BITS;
}

}  // namespace

extern "C" {

// CUDAImageCalibrator::OnD3D11CreateDevice(device, width, height)  .cpp:16-37: the render target becomes the scratch plane
int bf_image_calibrator_create(uint32_t width, uint32_t height, bf_image_calibrator** out) {
    BF_REQUIRE(out && width > 0 && height > 0 && width < 32768 && height < 32768, "bad image size");
    bf_image_calibrator* c = new bf_image_calibrator;
    bf::CreateGuard<bf_image_calibrator> guard(c, bf_image_calibrator_destroy);
    c->width = width; c->height = height;
    const uint32_t n = width * height;
    BF_TRY(c->res.device(&c->d_scratch, n));
    k_calib_arm<<<div_up(n, 256), 256, 0, nullptr>>>(c->d_scratch, n);
    BF_HIP_TRY(hipStreamSynchronize(nullptr));          // armed before any stream of the caller's can use it
    *out = guard.dismiss();
    return BF_OK;
}

// OnD3D11DestroyDevice()  .cpp:8-14
int bf_image_calibrator_destroy(bf_image_calibrator* c) {
    if (!c) return BF_OK;
    (void)hipStreamSynchronize(c->stream);
    delete c;
    return BF_OK;
}

int bf_image_calibrator_set_stream(bf_image_calibrator* c, void* s) { BF_REQUIRE(c, "null calibrator"); c->stream = (hipStream_t)s; return BF_OK; }

// process(context, d_depth, colorIntrinsics, depthIntrinsicsInv, depthExtrinsics)  .cpp:39-64, the two thresholds as arguments (the reference reads them
// from GlobalAppState inside, :56)
int bf_image_calibrator_process(bf_image_calibrator* c, float* d_depth, const float colorIntrinsics[16], const float depthIntrinsicsInv[16], const float depthExtrinsics[16],
                                float threshOffset, float threshLin) {
    BF_REQUIRE(c && d_depth && colorIntrinsics && depthIntrinsicsInv && depthExtrinsics, "null argument");
    CalibArgs A;
    memcpy(A.Kc.e, colorIntrinsics, 64); memcpy(A.KdInv.e, depthIntrinsicsInv, 64); memcpy(A.E.e, depthExtrinsics, 64);
    A.threshOffset = threshOffset; A.threshLin = threshLin; A.w = (int)c->width; A.h = (int)c->height;
    k_calib_raster<<<dim3(div_up(c->width, TW), div_up(c->height, TH)), dim3(TW, TH), 0, c->stream>>>(c->d_scratch, d_depth, A);
    BF_HIP_TRY(hipGetLastError());
    const uint32_t n = c->width * c->height;
    k_calib_resolve<<<div_up(n, 256), 256, 0, c->stream>>>(d_depth, c->d_scratch, n);
    BF_HIP_TRY(hipGetLastError());
    return BF_OK;
}

}  // extern "C"
