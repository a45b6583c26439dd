// A texture atlas for a mesh taken from the key frames on the device, for gfx950, without the mesh leaving HBM (DESIGN.md "Mesh texture: the definition";
// include/bf_hip.h states it next to bf_marching_cubes_texture).  The reference has no counterpart (mLib is absent); bf_mesh_texture_host below is the definition as
// one sequential loop, tests/mesh_texture_ref.py restates it in numpy, and the kernels are held to both as bytes and bits.
//
// Two passes.  k_texture_select, one thread per face: the face's normal, then the frames in the order given - a frame views the face where all three corners pass
// rules 2 - 6 of the recolouring (bf_meshview.h's pairOf, the same copy), and the face takes the viewing frame of greatest weight (the least of its corners'; a later
// frame only where strictly greater).  The frame table holds ALL the frames given, a skipped one with a null image, and is indexed by the loop counter alone: the
// compiler fetches it through the scalar path, and a face's frame index is the caller's.  The same thread writes the face's six texture coordinates, which are pure
// layout.  k_texture_fill, one thread per texel: the layout (integers only, layoutOf / fillTexel below, the same functions on the host) names the texel's face and
// its barycentric weights; the point is projected into the face's frame and the colour gathered bilinearly, or interpolated from the vertex colours where the face
// has no frame or the texel leaves the image.  There is no depth test per texel: the three corners passed it.
//
// Nothing depends on the order in which threads run: a face and a texel each belong to one thread, there are no atomics on floats, the counters of the stats are
// integer atomics behind a wave reduction.  Every device loop is bounded (the frame loop by numFrames, the texel loop by the texel count); no kernel waits for
// another workgroup and nothing spins.  A thread of the fill takes texel index, index + FILL_GRID * 256, ...: the counters then cost one atomic per wave of the
// grid, not per wave of texels.  Texel indices fit 32 bits: the atlas is at most 16384 x 32768.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bf_device.h"
#include "bf_resources.h"
#include "bf_meshtexture.h"
#include "bf_meshview.h"

using namespace bf;

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t FILL_GRID = 4096;          // one step of the texel loop is FILL_GRID * WG texels
constexpr uint32_t MAX_HEIGHT = 32768;

// the control words (uint64, zeroed before the launches)
enum : uint32_t { W_TEXTURED = 0, W_FROM_FRAMES = 1, W_FROM_VERTICES = 2, W_UNUSED = 3, NUM_WORDS = 4 };
enum : int { TX_UNUSED = 0, TX_FRAME = 1, TX_VERTEX = 2 };

// ---- the layout: integers only, the same on host and device.  Face f lives in cell f >> 1, half f & 1; cells are S x S texels, cellsPerRow of them per atlas row
struct TxLayout { uint32_t S, m, A, cellsPerRow, H, nf; };

// false: the atlas would be higher than MAX_HEIGHT
bool layoutOf(uint32_t nf, const bf_mesh_texture_params& p, TxLayout& L) {
    L.S = p.patchSize; L.m = p.patchSize - 3u; L.A = p.atlasWidth; L.cellsPerRow = p.atlasWidth / p.patchSize; L.nf = nf;
    const uint64_t cells = ((uint64_t)nf + 1u) / 2u, rows = (cells + L.cellsPerRow - 1u) / L.cellsPerRow, H = rows * L.S;
    L.H = (uint32_t)std::min<uint64_t>(H, 0xFFFFFFFFull);
    return H <= MAX_HEIGHT;
}
// the texel of corner 0 (a), 1 (b) or 2 (c) of face f: half 1 is half 0 turned by 180 degrees, so no patch is mirrored
BF_HD void cornerOf(const TxLayout& L, uint32_t f, uint32_t corner, uint32_t& x, uint32_t& y) {
    const uint32_t q = f >> 1, t = f & 1u;
    uint32_t ci = corner == 1u ? L.m : 0u, cj = corner == 2u ? L.m : 0u;
    if (t) { ci = L.S - 1u - ci; cj = L.S - 1u - cj; }
    x = (q % L.cellsPerRow) * L.S + ci; y = (q / L.cellsPerRow) * L.S + cj;
}
BF_HD void faceUVOf(const TxLayout& L, uint32_t f, float* uv) {
    for (uint32_t corner = 0; corner < 3u; ++corner) {
        uint32_t x, y;
        cornerOf(L, f, corner, x, y);
        uv[2 * corner] = ((float)x + 0.5f) / (float)L.A;
        uv[2 * corner + 1] = 1.0f - ((float)y + 0.5f) / (float)L.H;
    }
}

// ---- the arithmetic of the definition, shared by the kernels and bf_mesh_texture_host (the library is built without contraction: one rounding per operation)
BF_HD f3 load3(const float* p, uint32_t i) { return mk3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]); }
BF_HD bool finite3(f3 P) { return finiteF(P.x) && finiteF(P.y) && finiteF(P.z); }

// the face's frame: its index in the table, -1 for a degenerate face or one no frame views
BF_HD int32_t selectFace(uint32_t f, const float* pos, const uint32_t* faces, uint32_t nv, const RcFrame* frames, uint32_t numFrames, const RcCamera& cam, const bf_mesh_texture_params& p) {
    const uint32_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if (a >= nv || b >= nv || c >= nv) return -1;
    const f3 Pa = load3(pos, a), Pb = load3(pos, b), Pc = load3(pos, c);
    if (!(finite3(Pa) && finite3(Pb) && finite3(Pc))) return -1;
    const f3 n = cross3(Pb - Pa, Pc - Pa);
    const float len = __builtin_sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z);
    if (!(len > 0.0f && len < BF_PINF)) return -1;
    const f3 N = n / len;
    int32_t best = -1;
    float bestWgt = 0.0f;
    for (uint32_t k = 0; k < numFrames; ++k) {
        if (!frames[k].depth) continue;          // skipped
        RcView va, vb, vc;
        if (pairOf(Pa, N, frames[k], cam, p, va) != BF_RECOLOUR_VIEW) continue;
        if (pairOf(Pb, N, frames[k], cam, p, vb) != BF_RECOLOUR_VIEW) continue;
        if (pairOf(Pc, N, frames[k], cam, p, vc) != BF_RECOLOUR_VIEW) continue;
        const float wgt = fminf(fminf(va.wgt, vb.wgt), vc.wgt);
        if (best < 0 || wgt > bestWgt) { best = (int32_t)k; bestWgt = wgt; }
    }
    return best;
}

BF_HD uint32_t byteOf(float v) { return (uint32_t)(uint8_t)(int)(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f); }          // (fmaxf of a NaN and 0 is 0)
BF_HD uint32_t rgbaOf(float r, float g, float b) { return byteOf(r) | (byteOf(g) << 8) | (byteOf(b) << 16) | 0xFF000000u; }

// texel (x, y) of the atlas as r | g << 8 | b << 16 | a << 24 and where it came from
BF_HD uint32_t fillTexel(uint32_t x, uint32_t y, const TxLayout& L, const float* pos, const float* col, const uint32_t* faces, uint32_t nv, const int32_t* faceFrame,
                         const RcFrame* frames, const RcCamera& cam, int& kind) {
    kind = TX_UNUSED;
    if (x >= L.cellsPerRow * L.S) return 0u;
    const uint32_t cellX = x / L.S, i = x - cellX * L.S, cellY = y / L.S, j = y - cellY * L.S;
    const uint32_t t = i + j <= L.S - 1u ? 0u : 1u;
    const uint32_t f = 2u * (cellY * L.cellsPerRow + cellX) + t;
    if (f >= L.nf) return 0u;
    kind = TX_VERTEX;
    const uint32_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    if (a >= nv || b >= nv || c >= nv) return 0xFF000000u;
    const float s = (float)(t ? L.S - 1u - i : i) / (float)L.m, r = (float)(t ? L.S - 1u - j : j) / (float)L.m;
    const float wb = s, wc = r, wa = (1.0f - s) - r;
    const int32_t k = faceFrame[f];
    if (k >= 0) {
        const f3 Pa = load3(pos, a), Pb = load3(pos, b), Pc = load3(pos, c);
        const f3 P = mk3((wa * Pa.x + wb * Pb.x) + wc * Pc.x, (wa * Pa.y + wb * Pb.y) + wc * Pc.y, (wa * Pa.z + wb * Pb.z) + wc * Pc.z);
        const RcFrame& fr = frames[k];
        const float p0 = ((fr.W[0] * P.x + fr.W[1] * P.y) + fr.W[2] * P.z) + fr.W[3] * 1.0f;
        const float p1 = ((fr.W[4] * P.x + fr.W[5] * P.y) + fr.W[6] * P.z) + fr.W[7] * 1.0f;
        const float z = ((fr.W[8] * P.x + fr.W[9] * P.y) + fr.W[10] * P.z) + fr.W[11] * 1.0f;
        if (z > 0.0f && z < BF_PINF) {
            const float u = (p0 * cam.fx) / z + cam.cx, v = (p1 * cam.fy) / z + cam.cy;
            if (u >= 0.0f && u < (float)(cam.w - 1) && v >= 0.0f && v < (float)(cam.h - 1)) {
                const int x0 = (int)u, y0 = (int)v;
                const float fa = u - (float)x0, fb = v - (float)y0;
                const size_t i00 = (size_t)y0 * (size_t)cam.w + (size_t)x0, i01 = i00 + (size_t)cam.w;          // x0 + 1 <= w - 1 and y0 + 1 <= h - 1
                const uint32_t* px = reinterpret_cast<const uint32_t*>(fr.color);
                const uint32_t c00 = px[i00], c10 = px[i00 + 1], c01 = px[i01], c11 = px[i01 + 1];
                if ((c00 & 0xFFFFFFu) && (c10 & 0xFFFFFFu) && (c01 & 0xFFFFFFu) && (c11 & 0xFFFFFFu)) {
                    kind = TX_FRAME;
                    return rgbaOf(bilinear(c00, c10, c01, c11, 0, fa, fb), bilinear(c00, c10, c01, c11, 8, fa, fb), bilinear(c00, c10, c01, c11, 16, fa, fb));
                }
            }
        }
    }
    const f3 Ca = load3(col, a), Cb = load3(col, b), Cc = load3(col, c);
    return rgbaOf(((wa * Ca.x + wb * Cb.x) + wc * Cc.x) * 255.0f, ((wa * Ca.y + wb * Cb.y) + wc * Cc.y) * 255.0f, ((wa * Ca.z + wb * Cb.z) + wc * Cc.z) * 255.0f);
}

// ---------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------
// thread = face, all frames; every face gets its frame and its texture coordinates
__global__ __launch_bounds__(256) void k_texture_select(const float* __restrict__ pos, const uint32_t* __restrict__ faces, uint32_t nv, const RcFrame* __restrict__ frames, uint32_t numFrames,
                                                        RcCamera cam, bf_mesh_texture_params p, TxLayout L, int32_t* __restrict__ faceFrame, float* __restrict__ faceUV,
                                                        unsigned long long* __restrict__ words) {
    const uint32_t f = blockIdx.x * WG + threadIdx.x;
    int textured = 0;
    if (f < L.nf) {
        const int32_t k = selectFace(f, pos, faces, nv, frames, numFrames, cam, p);
        faceFrame[f] = k;
        float uv[6];
        faceUVOf(L, f, uv);
        for (int e = 0; e < 6; ++e) faceUV[6 * (size_t)f + e] = uv[e];
        textured = k >= 0 ? 1 : 0;
    }
    textured = wave_sum_i(textured);
    if ((threadIdx.x & 63u) == 0u && textured) atomicAdd(words + W_TEXTURED, (unsigned long long)textured);
}

// thread = texel, `total` = A * H of them, cell-major: consecutive threads walk one cell's S * S texels, then the next cell's; the margin right of the last cell
// column comes behind all cells.  At S = 8 a wave is one cell: its two faces' data is the same on every lane and its gathers land on neighbouring pixels, at the
// price of stores in segments of S texels.  Measured against atlas-row-major threads (coalesced stores, 64 / S faces per wave) on 12.7 M texels: 0.37 ms against
// 0.43 ms (profiles/mesh_texture.md); the output does not depend on the mapping.
__global__ __launch_bounds__(256) void k_texture_fill(const float* __restrict__ pos, const float* __restrict__ col, const uint32_t* __restrict__ faces, uint32_t nv,
                                                      const int32_t* __restrict__ faceFrame, const RcFrame* __restrict__ frames, RcCamera cam, TxLayout L, uint32_t total,
                                                      uint32_t* __restrict__ atlas, unsigned long long* __restrict__ words) {
    int fromFrames = 0, fromVertices = 0, unused = 0;
    const uint32_t SS = L.S * L.S, cellTexels = L.cellsPerRow * (L.H / L.S) * SS, margin = L.A - L.cellsPerRow * L.S;
    for (uint32_t idx = blockIdx.x * WG + threadIdx.x; idx < total; idx += gridDim.x * WG) {
        uint32_t x, y;
        if (idx < cellTexels) {
            const uint32_t cell = idx / SS, l = idx - cell * SS, j = l / L.S, cellY = cell / L.cellsPerRow;
            x = (cell - cellY * L.cellsPerRow) * L.S + (l - j * L.S); y = cellY * L.S + j;
        } else {          // (margin > 0 here: without a margin the cells are all the texels)
            y = (idx - cellTexels) / margin; x = L.cellsPerRow * L.S + ((idx - cellTexels) - y * margin);
        }
        int kind;
        atlas[(size_t)y * L.A + x] = fillTexel(x, y, L, pos, col, faces, nv, faceFrame, frames, cam, kind);
        fromFrames += kind == TX_FRAME; fromVertices += kind == TX_VERTEX; unused += kind == TX_UNUSED;
    }
    fromFrames = wave_sum_i(fromFrames); fromVertices = wave_sum_i(fromVertices); unused = wave_sum_i(unused);          // (a thread takes at most 2^29 / 2^20 texels: the sums fit)
    if ((threadIdx.x & 63u) == 0u) {
        if (fromFrames) atomicAdd(words + W_FROM_FRAMES, (unsigned long long)fromFrames);
        if (fromVertices) atomicAdd(words + W_FROM_VERTICES, (unsigned long long)fromVertices);
        if (unused) atomicAdd(words + W_UNUSED, (unsigned long long)unused);
    }
}

template <typename T>
int grow(Resources& res, T** p, size_t count) { return res.regrow(p, std::max<size_t>(count, 1)); }

// the refusals of the definition, shared by both routes; null on success
const char* refusal(const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t w, uint32_t h, const float* intrinsics, const bf_mesh_texture_params* p) {
    if (!p || !intrinsics) return "null argument";
    if (w < 2 || h < 2 || w > 32768 || h > 32768) return "the frames must be at least 2 x 2 (and at most 32768 x 32768)";
    if (!finiteF(p->depthMin) || !finiteF(p->depthMax) || !finiteF(p->depthTolerance) || !finiteF(p->depthToleranceLin) || !finiteF(p->minCos)) return "a parameter is not finite";
    if (!(p->depthMin > 0.0f) || p->depthMax < p->depthMin) return "depthMin must be above 0 and depthMax not below depthMin";
    if (p->depthTolerance < 0.0f || p->depthToleranceLin < 0.0f) return "a depth tolerance is negative";
    if (!(p->minCos > 0.0f && p->minCos <= 1.0f)) return "minCos is not in (0, 1]";
    if (p->patchSize < 4u || p->patchSize > 64u) return "patchSize is not in 4 .. 64";
    if (p->atlasWidth < p->patchSize || p->atlasWidth > 16384u) return "atlasWidth is not in patchSize .. 16384";
    if (numFrames && !frames) return "null frames";
    for (uint32_t k = 0; k < numFrames; ++k)
        if (!frames[k].skipped && (!frames[k].d_depth || !frames[k].d_colorRGBX)) return "a frame that is not skipped has a null image";
    return nullptr;
}

// all the frames given, a skipped one with null images; the number that are not skipped
uint32_t tableOf(const bf_mesh_recolour_frame* frames, uint32_t numFrames, std::vector<RcFrame>& table) {
    uint32_t used = 0;
    table.resize(numFrames);
    for (uint32_t k = 0; k < numFrames; ++k) {
        table[k] = frameOf(frames[k]);
        if (frames[k].skipped) { table[k].depth = nullptr; table[k].color = nullptr; } else ++used;
    }
    return used;
}

void fillStats(bf_mesh_texture_stats* s, const TxLayout& L, uint32_t textured, uint32_t used, uint32_t numFrames, uint64_t fromFrames, uint64_t fromVertices, uint64_t unused) {
    if (!s) return;
    s->numFaces = L.nf; s->numFacesTextured = textured; s->numFacesUntextured = L.nf - textured; s->numFramesUsed = used; s->numFramesSkipped = numFrames - used;
    s->atlasWidth = L.A; s->atlasHeight = L.H; s->numTexelsFromFrames = fromFrames; s->numTexelsFromVertices = fromVertices; s->numTexelsUnused = unused;
}

}  // namespace

namespace bf {

int meshtexture_run(MeshTexture& t, Resources& res, hipStream_t st, const bf_clean_mesh& in, const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t w, uint32_t h,
                    const float* intrinsics, const bf_mesh_texture_params& params, bf_mesh_texture_stats* stats) {
    const uint32_t nv = in.numVertices, nf = in.numFaces;
    // ---- the refusals, before any buffer of the last result is touched
    if (const char* why = refusal(frames, numFrames, w, h, intrinsics, &params)) { set_error("bf_marching_cubes_texture: %s", why); return BF_ERR_INVALID_ARG; }
    BF_REQUIRE((nv == 0 || (in.d_positions && in.d_colors)) && (nf == 0 || in.d_faces), "null mesh array");
    TxLayout L;
    if (!layoutOf(nf, params, L)) {
        set_error("bf_marching_cubes_texture: %u faces in patches of %u need an atlas higher than %u at width %u", nf, L.S, MAX_HEIGHT, L.A);
        return BF_ERR_CAPACITY;
    }
    std::vector<RcFrame> table;
    const uint32_t used = tableOf(frames, numFrames, table);
    const size_t total = (size_t)L.A * L.H;

    if (!t.d_words) BF_TRY(res.device(&t.d_words, NUM_WORDS));
    if (numFrames > t.capFrames || !t.d_frames) { t.capFrames = 0; BF_TRY(grow(res, (RcFrame**)&t.d_frames, numFrames)); t.capFrames = numFrames; }
    if (nf > t.capFaces || !t.d_faceFrame) {
        t.capFaces = 0; t.numFaces = t.atlasWidth = t.atlasHeight = 0;
        BF_TRY(grow(res, &t.d_faceFrame, nf)); BF_TRY(grow(res, &t.d_faceUV, 6 * (size_t)nf));
        t.capFaces = nf;
    }
    if (total > t.capTexels || !t.d_atlas) {
        t.capTexels = 0; t.numFaces = t.atlasWidth = t.atlasHeight = 0;
        BF_TRY(grow(res, &t.d_atlas, total));
        t.capTexels = total;
    }
    if (numFrames) BF_HIP_TRY(hipMemcpyAsync(t.d_frames, table.data(), sizeof(RcFrame) * (size_t)numFrames, hipMemcpyHostToDevice, st));
    BF_HIP_TRY(hipMemsetAsync(t.d_words, 0, sizeof(unsigned long long) * NUM_WORDS, st));
    if (nf) {
        const RcCamera cam = cameraOf(intrinsics, w, h);
        hipLaunchKernelGGL(k_texture_select, dim3((nf + WG - 1) / WG), dim3(WG), 0, st, in.d_positions, in.d_faces, nv, (const RcFrame*)t.d_frames, numFrames, cam, params, L, t.d_faceFrame,
                           t.d_faceUV, t.d_words);
        const dim3 grid((uint32_t)std::min<size_t>((total + WG - 1) / WG, FILL_GRID));
        hipLaunchKernelGGL(k_texture_fill, grid, dim3(WG), 0, st, in.d_positions, in.d_colors, in.d_faces, nv, (const int32_t*)t.d_faceFrame, (const RcFrame*)t.d_frames, cam, L,
                           (uint32_t)total, t.d_atlas, t.d_words);
    }
    BF_HIP_TRY(hipGetLastError());
    unsigned long long words[NUM_WORDS] = {0};
    BF_HIP_TRY(hipMemcpyAsync(words, t.d_words, sizeof words, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));          // (the frame table on the host outlives its copy)
    t.numFaces = nf; t.atlasWidth = L.A; t.atlasHeight = L.H;
    fillStats(stats, L, (uint32_t)std::min<unsigned long long>(words[W_TEXTURED], nf), used, numFrames, words[W_FROM_FRAMES], words[W_FROM_VERTICES], words[W_UNUSED]);
    return BF_OK;
}

}  // namespace bf

extern "C" int bf_mesh_texture_atlas_height(uint32_t numFaces, const bf_mesh_texture_params* p, uint32_t* atlasHeight) {
    BF_REQUIRE(p && atlasHeight, "null argument");
    BF_REQUIRE(p->patchSize >= 4u && p->patchSize <= 64u && p->atlasWidth >= p->patchSize && p->atlasWidth <= 16384u, "patchSize is not in 4 .. 64 or atlasWidth not in patchSize .. 16384");
    TxLayout L;
    if (!layoutOf(numFaces, *p, L)) { set_error("bf_mesh_texture_atlas_height: %u faces in patches of %u need an atlas higher than %u at width %u", numFaces, L.S, MAX_HEIGHT, L.A); return BF_ERR_CAPACITY; }
    *atlasHeight = L.H;
    return BF_OK;
}

// The definition on one core: per face in increasing id, per frame in the order given; then per texel, row by row.
extern "C" int bf_mesh_texture_host(const float* pos, const float* col, const uint32_t* faces, uint32_t nv, uint32_t nf, const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t w,
                                    uint32_t h, const float* intrinsics, const bf_mesh_texture_params* params, uint8_t* atlasOut, int32_t* faceFrameOut, float* faceUVOut,
                                    bf_mesh_texture_stats* stats) {
    if (const char* why = refusal(frames, numFrames, w, h, intrinsics, params)) { set_error("bf_mesh_texture_host: %s", why); return BF_ERR_INVALID_ARG; }
    BF_REQUIRE((nv == 0 || (pos && col)) && (nf == 0 || faces), "null mesh array");
    TxLayout L;
    if (!layoutOf(nf, *params, L)) { set_error("bf_mesh_texture_host: %u faces in patches of %u need an atlas higher than %u at width %u", nf, L.S, MAX_HEIGHT, L.A); return BF_ERR_CAPACITY; }
    const RcCamera cam = cameraOf(intrinsics, w, h);
    std::vector<RcFrame> table;
    const uint32_t used = tableOf(frames, numFrames, table);
    std::vector<int32_t> faceFrame(nf);
    uint32_t textured = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        faceFrame[f] = selectFace(f, pos, faces, nv, table.data(), numFrames, cam, *params);
        textured += faceFrame[f] >= 0 ? 1u : 0u;
        if (faceUVOut) faceUVOf(L, f, faceUVOut + 6 * (size_t)f);
    }
    uint64_t count[3] = {0, 0, 0};
    for (uint32_t y = 0; y < L.H; ++y)
        for (uint32_t x = 0; x < L.A; ++x) {
            int kind;
            const uint32_t rgba = fillTexel(x, y, L, pos, col, faces, nv, faceFrame.data(), table.data(), cam, kind);
            ++count[kind];
            if (atlasOut) memcpy(atlasOut + 4 * ((size_t)y * L.A + x), &rgba, 4);
        }
    if (faceFrameOut && nf) memcpy(faceFrameOut, faceFrame.data(), 4 * (size_t)nf);
    fillStats(stats, L, textured, used, numFrames, count[TX_FRAME], count[TX_VERTEX], count[TX_UNUSED]);
    return BF_OK;
}

// The PLY of a textured mesh (host only): bf_write_ply_indexed[_normals]' header with the texture's file name in a comment and a texcoord list per face; the
// vertex records are those writers', a face record is theirs followed by the byte 6 and u_a v_a u_b v_b u_c v_c.
extern "C" int bf_write_ply_textured(const char* filename, const char* textureFileName, const float* h_positions, const float* h_normals, const float* h_colors, const uint32_t* h_faces,
                                     const float* h_faceUV, uint32_t numVertices, uint32_t numFaces) {
    BF_REQUIRE(filename && textureFileName, "null argument");
    BF_REQUIRE((numVertices == 0 || (h_positions && h_colors)) && (numFaces == 0 || (h_faces && h_faceUV)), "null array");
    BF_REQUIRE(!strchr(textureFileName, '\n') && !strchr(textureFileName, '\r'), "the texture's file name has a line break");
    FILE* f = fopen(filename, "wb");
    if (!f) { set_error("cannot open %s", filename); return BF_ERR_INVALID_ARG; }
    fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment bundlefusion_amd marching cubes\ncomment TextureFile %s\nelement vertex %u\nproperty float x\nproperty float y\nproperty float z\n"
               "%sproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face %u\nproperty list uchar int vertex_indices\n"
               "property list uchar float texcoord\nend_header\n", textureFileName, numVertices, h_normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "", numFaces);
    const size_t CH = 65536;            // records per write
    const size_t vsize = h_normals ? 28 : 16;
    std::vector<uint8_t> buf(CH * 38);
    for (size_t base = 0; base < numVertices; base += CH) {
        const size_t m = std::min(CH, (size_t)numVertices - base);
        for (size_t j = 0; j < m; ++j) {
            const size_t i = base + j;
            uint8_t* r = buf.data() + vsize * j;
            memcpy(r, h_positions + 3 * i, 12);
            if (h_normals) memcpy(r + 12, h_normals + 3 * i, 12);
            for (int k = 0; k < 3; ++k) r[vsize - 4 + k] = (uint8_t)std::max(0.0f, std::min(255.0f, h_colors[3 * i + k] * 255.0f + 0.5f));
            r[vsize - 1] = 255;
        }
        fwrite(buf.data(), vsize, m, f);
    }
    for (size_t base = 0; base < numFaces; base += CH) {
        const size_t m = std::min(CH, (size_t)numFaces - base);
        for (size_t j = 0; j < m; ++j) {
            uint8_t* r = buf.data() + 38 * j;
            r[0] = 3;
            memcpy(r + 1, h_faces + 3 * (base + j), 12);          // int32 in the file: the same bits
            r[13] = 6;
            memcpy(r + 14, h_faceUV + 6 * (base + j), 24);
        }
        fwrite(buf.data(), 38, m, f);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) { set_error("cannot write %s", filename); return BF_ERR_INVALID_ARG; }
    return BF_OK;
}
