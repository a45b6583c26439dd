// The colours of a mesh's vertices taken from the key frames on the device, for gfx950, without the mesh leaving HBM (DESIGN.md "Mesh colour from the key frames:
// the definition"; include/bf_hip.h states it next to bf_marching_cubes_recolour).  The reference has no counterpart (mLib is absent); bf_mesh_recolour_host below
// is the definition as one sequential loop, tests/mesh_recolour_ref.py restates it in numpy, and the kernel is held to both as bits.
//
// Nothing here depends on the order in which threads run: a vertex belongs to one thread, which walks the frames in the order given, so the one float sum of the
// definition (mode 0) has the stated order; there are no atomics on floats.  The two counters of the stats are integer atomics (a sum and a maximum).
//
// Shape: one thread per vertex (grid-stride beyond MAX_GRID workgroups), ALL frames in one launch - the accumulators (three sums, the weight, the view count; mode
// 1: the best weight and its sample) live in registers from the first frame to the last and never round-trip through HBM, so there is no batch size.  The frame
// table (mesh to camera, camera centre, the two image pointers: 80 bytes per frame) sits in a device buffer and is indexed by the loop counter alone: every lane
// reads the same address, so the compiler fetches it through the scalar path (s_load) into SGPRs, and a frame costs no vector register.  Marching cubes emits
// vertices block by block and the clean keeps that order, so the lanes of a wave project to neighbouring pixels: the four depth gathers and four colour gathers of a
// pair touch a few cache lines per wave.  The gates are ordered cheapest first, and the depth gathers come before the colour gathers, which only lanes with an
// unoccluded pair issue.
// Every device loop is bounded (the vertex loop by numVertices, the frame loop by numFrames); no kernel waits for another workgroup and nothing spins.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bf_device.h"
#include "bf_resources.h"
#include "bf_meshrecolour.h"
#include "bf_meshview.h"

using namespace bf;

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t MAX_GRID = 8192;          // one step of the vertex loop is MAX_GRID * WG vertices

// the control words (uint32, zeroed before the launch)
enum : uint32_t { W_RECOLOURED = 0, W_MAX_VIEWS = 1, NUM_WORDS = 4 };

// ---- the arithmetic of the definition, shared by the kernel and bf_mesh_recolour_host (the library is built without contraction: one rounding per operation);
// rules 2 - 6 of a pair (pairOf) and the frame table are bf_meshview.h's, which the texture atlas shares
BF_HD bool vertexOk(f3 P, f3 N) {                                            // rule 1
    return finiteF(P.x) && finiteF(P.y) && finiteF(P.z) && finiteF(N.x) && finiteF(N.y) && finiteF(N.z) && (N.x * N.x + N.y * N.y) + N.z * N.z > 0.0f;
}
// the vertex's state over the frames in the order given; mode 0: acc = S, w = SW; mode 1: acc = the best view's sample, w = its weight
struct RcState { float acc[3], w; uint32_t views; };
BF_HD void stateInit(RcState& s) { s.acc[0] = s.acc[1] = s.acc[2] = 0.0f; s.w = 0.0f; s.views = 0u; }
BF_HD void stateAdd(RcState& s, const RcView& v, int mode) {
    if (mode == 0) {
        s.acc[0] = s.acc[0] + v.wgt * v.val[0]; s.acc[1] = s.acc[1] + v.wgt * v.val[1]; s.acc[2] = s.acc[2] + v.wgt * v.val[2];
        s.w = s.w + v.wgt;
    } else if (s.views == 0u || v.wgt > s.w) {
        s.acc[0] = v.val[0]; s.acc[1] = v.val[1]; s.acc[2] = v.val[2]; s.w = v.wgt;
    }
    ++s.views;
}
// the vertex's colour: false where it keeps its input colour
BF_HD bool stateColour(const RcState& s, int mode, float out[3]) {
    if (s.views == 0u) return false;
    if (mode == 0) {
        if (!(s.w > 0.0f && s.w < BF_PINF)) return false;
        out[0] = (s.acc[0] / s.w) / 255.0f; out[1] = (s.acc[1] / s.w) / 255.0f; out[2] = (s.acc[2] / s.w) / 255.0f;
    } else {
        out[0] = s.acc[0] / 255.0f; out[1] = s.acc[1] / 255.0f; out[2] = s.acc[2] / 255.0f;
    }
    return true;
}

// ---------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_recolour_zero(uint32_t* __restrict__ words) { if (threadIdx.x < NUM_WORDS) words[threadIdx.x] = 0u; }

// thread = vertex, all frames; colOut and views get every vertex (an unseen one its input colour bit for bit)
__global__ __launch_bounds__(256) void k_recolour(const float* __restrict__ pos, const float* __restrict__ nrm, const float* colIn, uint32_t nv, const RcFrame* __restrict__ frames,
                                                  uint32_t numFrames, RcCamera cam, bf_mesh_recolour_params p, float* colOut, uint32_t* __restrict__ views, uint32_t* __restrict__ words) {
    uint32_t recoloured = 0u, most = 0u;
    for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < nv; i += (size_t)gridDim.x * WG) {
        const f3 P = mk3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), N = mk3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
        RcState s; stateInit(s);
        if (vertexOk(P, N))
            for (uint32_t k = 0; k < numFrames; ++k) {
                RcView view;
                if (pairOf(P, N, frames[k], cam, p, view) == BF_RECOLOUR_VIEW) stateAdd(s, view, p.mode);
            }
        float c[3] = {colIn[3 * i], colIn[3 * i + 1], colIn[3 * i + 2]};
        if (stateColour(s, p.mode, c)) ++recoloured;
        colOut[3 * i] = c[0]; colOut[3 * i + 1] = c[1]; colOut[3 * i + 2] = c[2];
        views[i] = s.views;
        most = s.views > most ? s.views : most;
    }
    recoloured = (uint32_t)wave_sum_i((int)recoloured);
    most = wave_max_u(most);
    if ((threadIdx.x & 63u) == 0u) {
        if (recoloured) atomicAdd(words + W_RECOLOURED, recoloured);
        if (most) atomicMax(words + W_MAX_VIEWS, most);
    }
}

uint32_t gridFor(size_t n) { return (uint32_t)std::max<size_t>(1, std::min<size_t>((n + WG - 1) / WG, MAX_GRID)); }

template <typename T>
int grow(Resources& res, T** p, size_t count) { return res.regrow(p, std::max<size_t>(count, 1)); }

// the refusals of the definition, shared by both routes; null on success
const char* refusal(const float* normals, uint32_t nv, const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t w, uint32_t h, const float* intrinsics,
                    const bf_mesh_recolour_params* p) {
    if (!p || !intrinsics) return "null argument";
    if (nv && !normals) return "the mesh has no normals (clean or simplify it with computeNormals)";
    if (w < 2 || h < 2 || w > 32768 || h > 32768) return "the frames must be at least 2 x 2 (and at most 32768 x 32768)";
    if (!finiteF(p->depthMin) || !finiteF(p->depthMax) || !finiteF(p->depthTolerance) || !finiteF(p->depthToleranceLin) || !finiteF(p->minCos)) return "a parameter is not finite";
    if (!(p->depthMin > 0.0f) || p->depthMax < p->depthMin) return "depthMin must be above 0 and depthMax not below depthMin";
    if (p->depthTolerance < 0.0f || p->depthToleranceLin < 0.0f) return "a depth tolerance is negative";
    if (!(p->minCos > 0.0f && p->minCos <= 1.0f)) return "minCos is not in (0, 1]";
    if (p->mode != 0 && p->mode != 1) return "mode is neither 0 (blend) nor 1 (best view)";
    if (numFrames && !frames) return "null frames";
    for (uint32_t k = 0; k < numFrames; ++k)
        if (!frames[k].skipped && (!frames[k].d_depth || !frames[k].d_colorRGBX)) return "a frame that is not skipped has a null image";
    return nullptr;
}

void fillStats(bf_mesh_recolour_stats* s, uint32_t nv, uint32_t recoloured, uint32_t used, uint32_t numFrames, uint32_t maxViews) {
    if (!s) return;
    s->numVertices = nv; s->numRecoloured = recoloured; s->numUnseen = nv - recoloured; s->numFramesUsed = used; s->numFramesSkipped = numFrames - used; s->maxViews = maxViews;
}

}  // namespace

namespace bf {

int meshrecolour_run(MeshRecolour& r, Resources& res, hipStream_t st, const bf_clean_mesh& in, const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t w, uint32_t h,
                     const float* intrinsics, const bf_mesh_recolour_params& params, bf_mesh_recolour_stats* stats) {
    const uint32_t nv = in.numVertices;
    // ---- the refusals, before any buffer of the last result is touched
    if (const char* why = refusal(in.d_normals, nv, frames, numFrames, w, h, intrinsics, &params)) { set_error("bf_marching_cubes_recolour: %s", why); return BF_ERR_INVALID_ARG; }
    BF_REQUIRE(nv == 0 || (in.d_positions && in.d_colors), "null mesh array");
    std::vector<RcFrame> table;
    for (uint32_t k = 0; k < numFrames; ++k) if (!frames[k].skipped) table.push_back(frameOf(frames[k]));
    const uint32_t used = (uint32_t)table.size();

    if (!r.d_words) BF_TRY(res.device(&r.d_words, NUM_WORDS));
    if (used > r.capFrames || !r.d_frames) { r.capFrames = 0; BF_TRY(grow(res, (RcFrame**)&r.d_frames, used)); r.capFrames = used; }
    if (nv > r.capVertices || !r.d_colors) {
        r.capVertices = 0; r.numVertices = r.numFaces = 0;
        BF_TRY(grow(res, &r.d_colors, 3 * (size_t)nv)); BF_TRY(grow(res, &r.d_views, nv));
        r.capVertices = nv;
    }
    if (used) BF_HIP_TRY(hipMemcpyAsync(r.d_frames, table.data(), sizeof(RcFrame) * (size_t)used, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_recolour_zero, dim3(1), dim3(WG), 0, st, r.d_words);
    if (nv) hipLaunchKernelGGL(k_recolour, dim3(gridFor(nv)), dim3(WG), 0, st, in.d_positions, in.d_normals, in.d_colors, nv, (const RcFrame*)r.d_frames, used, cameraOf(intrinsics, w, h), params,
                               r.d_colors, r.d_views, r.d_words);
    BF_HIP_TRY(hipGetLastError());
    uint32_t words[NUM_WORDS] = {0};
    BF_HIP_TRY(hipMemcpyAsync(words, r.d_words, sizeof words, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));          // (the frame table on the host outlives its copy)
    r.d_positions = in.d_positions; r.d_normals = in.d_normals; r.d_faces = in.d_faces; r.numVertices = nv; r.numFaces = in.numFaces;
    fillStats(stats, nv, std::min(words[W_RECOLOURED], nv), used, numFrames, words[W_MAX_VIEWS]);
    return BF_OK;
}

}  // namespace bf

extern "C" int bf_mesh_recolour_frame_from_pose(const float* cameraToMesh, bf_mesh_recolour_frame* frame) {
    BF_REQUIRE(cameraToMesh && frame, "null argument");
    m44 M; memcpy(M.e, cameraToMesh, 64);
    const m44 W = inverse44(M);
    memcpy(frame->meshToCamera, W.e, 64);
    frame->cameraCentre[0] = M.e[3]; frame->cameraCentre[1] = M.e[7]; frame->cameraCentre[2] = M.e[11];
    bool ok = !(M.e[0] != M.e[0] || M.e[0] == BF_MINF);
    for (int i = 0; i < 16; ++i) ok = ok && finiteF(W.e[i]);
    for (int i = 0; i < 3; ++i) ok = ok && finiteF(frame->cameraCentre[i]);
    frame->skipped = ok ? 0 : 1;
    return BF_OK;
}

// The definition on one core: per vertex in increasing id, per frame in the order given.
extern "C" int bf_mesh_recolour_host(const float* pos, const float* nrm, const float* col, uint32_t nv, const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t w, uint32_t h,
                                     const float* intrinsics, const bf_mesh_recolour_params* params, float* colOut, uint32_t* viewsOut, uint8_t* codesOut, bf_mesh_recolour_stats* stats) {
    if (const char* why = refusal(nrm, nv, frames, numFrames, w, h, intrinsics, params)) { set_error("bf_mesh_recolour_host: %s", why); return BF_ERR_INVALID_ARG; }
    BF_REQUIRE(nv == 0 || (pos && col), "null mesh array");
    const RcCamera cam = cameraOf(intrinsics, w, h);
    std::vector<RcFrame> table(numFrames);
    uint32_t used = 0;
    for (uint32_t k = 0; k < numFrames; ++k) { table[k] = frameOf(frames[k]); used += frames[k].skipped ? 0u : 1u; }
    uint32_t recoloured = 0, most = 0;
    for (uint32_t i = 0; i < nv; ++i) {
        const size_t b = 3 * (size_t)i;
        const f3 P = mk3(pos[b], pos[b + 1], pos[b + 2]), N = mk3(nrm[b], nrm[b + 1], nrm[b + 2]);
        const bool ok = vertexOk(P, N);
        RcState s; stateInit(s);
        for (uint32_t k = 0; k < numFrames; ++k) {
            if (frames[k].skipped) continue;
            RcView view;
            const uint32_t code = ok ? pairOf(P, N, table[k], cam, *params, view) : (uint32_t)BF_RECOLOUR_NORMAL;
            if (code == BF_RECOLOUR_VIEW) stateAdd(s, view, params->mode);
            if (codesOut) codesOut[(size_t)i * numFrames + k] = (uint8_t)code;
        }
        float c[3] = {col[b], col[b + 1], col[b + 2]};
        if (stateColour(s, params->mode, c)) ++recoloured;
        if (colOut) { colOut[b] = c[0]; colOut[b + 1] = c[1]; colOut[b + 2] = c[2]; }
        if (viewsOut) viewsOut[i] = s.views;
        most = std::max(most, s.views);
    }
    fillStats(stats, nv, recoloured, used, numFrames, most);
    return BF_OK;
}
