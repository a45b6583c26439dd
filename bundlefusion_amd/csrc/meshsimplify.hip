// Simplification of an indexed mesh on the device by vertex clustering on a uniform grid (Rossignac-Borrel), for gfx950, without the mesh leaving HBM
// (DESIGN.md "Mesh simplification: the definition"; include/bf_hip.h states it next to bf_marching_cubes_simplify).  The reference has no counterpart (mLib is
// absent); bf_mesh_simplify_host below is the definition as one sequential loop, tests/mesh_simplify_ref.py restates it in numpy, and the kernels are held to both
// as bits.
//
// Nothing here depends on the order in which threads run: a cluster's leader is a minimum over vertex ids, its representative comes from int64 sums of quantised
// coordinates (no float sums, no float atomics), a kept face is a minimum over face numbers, and ids count leaders / kept elements in increasing number.
//
// Tables: the weld's protocol (meshweld.hip:13-18).  An open-addressing table of uint32 NUMBERS (capacity: a power of two >= 2 * max(nv, nf), linear probing) -
// vertex numbers keyed on the cell of the vertex, then, refilled, face numbers keyed on the sorted triple of cluster numbers.  Insert of number i at slot h:
// prev = atomicCAS(slot, EMPTY, i); EMPTY: done; key(prev) == key(i): atomicMin(slot, i), done; otherwise the next slot.  Inside an insert kernel a slot is read
// through the CAS result only; the kernels after it start behind the kernel boundary and read slots with plain loads.
// Counting and compaction: the weld's scheme - tiles of 1024 elements, count per tile, one scan of the tile counts by one workgroup, scatter.
// Accumulation (the hot path, 7 integer adds per vertex): marching cubes emits vertices block by block, so the lanes of a wave mostly share a handful of clusters.
// A wave walks its distinct cluster numbers (readfirstlane of the lowest pending lane, a ballot of the lanes that hold the same number), sums the seven values
// over those lanes, and one lane issues one set of seven 64-bit integer atomics per (wave, cluster) - k_clean_count's scheme.
// Every device loop is bounded: probe sequences by the table size, the wave loop by 64.  Exhaustion sets a bit of the error word, which the host turns into
// BF_ERR_INTERNAL; no kernel waits for another workgroup and nothing spins.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "bf_device.h"
#include "bf_resources.h"
#include "bf_meshsimplify.h"

using namespace bf;

namespace {

typedef unsigned long long u64;

constexpr uint32_t WG = 256;
constexpr uint32_t TILE = 1024;                 // 4 consecutive elements per thread
constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint32_t MAX_GRID = 8192;
constexpr uint32_t MAX_FACES = 300000000u;      // 3 * numFaces stays below 2^32
constexpr uint32_t MAX_VERTICES = 900000000u;   // as many as MAX_FACES faces have corners; 2 * numVertices rounded up to a power of two stays below 2^32

// the control words (uint32, zeroed before the validation)
enum : uint32_t { W_ERR = 0, W_CLUSTERS = 1, W_NV_OUT = 2, W_NF_OUT = 3, W_COLLAPSED = 4, W_LARGEST = 5, NUM_WORDS = 8 };
constexpr uint32_t ERR_FACE_ID = 1u, ERR_VALUE = 2u, ERR_CELL = 4u, ERR_LOOP = 8u;

// ---- the arithmetic of the definition, shared by the kernels and bf_mesh_simplify_host (the library is built without contraction: one rounding per operation)
BF_HD bool valueOk(float x) { return x > -1024.0f && x < 1024.0f; }          // finite and |x| < 1024 (a NaN fails both comparisons)
// the 63-bit key of the cell of p: per axis floor((double)p * inv), inv = 1.0 / (double)cellSize, biased by 2^20; false where an index is not in (-2^20, 2^20)
BF_HD bool cellKey(const float* __restrict__ p, double inv, u64& key) {
    key = 0ull;
    for (int d = 0; d < 3; ++d) {
        const double t = __builtin_floor((double)p[d] * inv);
        if (!(t > -1048576.0 && t < 1048576.0)) return false;
        key |= (u64)((long long)t + 1048576ll) << (21 * d);
    }
    return true;
}
BF_HD long long quant(float x) { return (long long)__builtin_floor((double)x * 1048576.0 + 0.5); }
BF_HD float meanOf(long long S, u64 n) { return (float)((double)S / ((double)n * 1048576.0)); }

BF_DEV uint32_t mix(u64 a, u64 b, u64 c) {          // the weld's hash
    u64 h = a * 0x9E3779B97F4A7C15ull;
    h = (h ^ (h >> 31) ^ b) * 0xC2B2AE3D27D4EB4Full;
    h = (h ^ (h >> 29) ^ c) * 0x165667B19E3779F9ull;
    return (uint32_t)(h >> 32) ^ (uint32_t)h;
}

// the two key sources: a vertex of the position array, a face of the cluster-number array
struct CellSrc { const float* pos; double inv; };
struct TriSrc { const uint32_t* ids; };
struct Tri3 { uint32_t a, b, c; };          // sorted
BF_DEV u64 keyAt(const CellSrc& s, uint32_t v) { u64 k; cellKey(s.pos + 3 * (size_t)v, s.inv, k); return k; }
BF_DEV Tri3 keyAt(const TriSrc& s, uint32_t f) {
    uint32_t a = s.ids[3 * (size_t)f], b = s.ids[3 * (size_t)f + 1], c = s.ids[3 * (size_t)f + 2], x;
    if (a > b) { x = a; a = b; b = x; }
    if (b > c) { x = b; b = c; c = x; }
    if (a > b) { x = a; a = b; b = x; }
    Tri3 r; r.a = a; r.b = b; r.c = c;
    return r;
}
BF_DEV bool same(u64 p, u64 q) { return p == q; }
BF_DEV bool same(const Tri3& p, const Tri3& q) { return p.a == q.a && p.b == q.b && p.c == q.c; }
BF_DEV uint32_t hashKey(u64 k) { return mix(k & 0x1FFFFFull, (k >> 21) & 0x1FFFFFull, k >> 42); }
BF_DEV uint32_t hashKey(const Tri3& k) { return mix(k.a, k.b, k.c); }

// the insert of the protocol above over the numbers below n; slot values only ever decrease.  false: the probe sequence ran out, or a slot held no number
template <typename K, typename S>
BF_DEV bool tableInsert(uint32_t* table, uint32_t mask, uint32_t i, uint32_t n, const K& key, const S& src) {
    uint32_t h = hashKey(key) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes, h = (h + 1u) & mask) {
        const uint32_t prev = atomicCAS(&table[h], EMPTY, i);
        if (prev == EMPTY) return true;
        if (prev >= n) return false;
        if (same(keyAt(src, prev), key)) { if (i < prev) atomicMin(&table[h], i); return true; }
    }
    return false;
}
// after the insert kernel: the slot of the key holds its lowest number
template <typename K, typename S>
BF_DEV uint32_t tableFind(const uint32_t* __restrict__ table, uint32_t mask, uint32_t i, uint32_t n, const K& key, const S& src, bool& ok) {
    uint32_t h = hashKey(key) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes, h = (h + 1u) & mask) {
        const uint32_t s = table[h];
        if (s == i) return i;
        if (s >= n) break;          // EMPTY included
        if (same(keyAt(src, s), key)) return s;
    }
    ok = false;                     // (not reached: every number was inserted)
    return i;
}

__global__ __launch_bounds__(256) void k_simp_fill(uint32_t* __restrict__ a, size_t n, uint32_t v) {
    for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) a[i] = v;
}
// the refusals: a component that is not finite or not below 1024, a cell index beyond 2^20, a face id beyond the vertices
__global__ __launch_bounds__(256) void k_simp_validate(const float* __restrict__ pos, const float* __restrict__ col, uint32_t nv, const uint32_t* __restrict__ faces, uint32_t n, double inv,
                                                       uint32_t* words) {
    uint32_t bad = 0;
    for (uint32_t v = blockIdx.x * WG + threadIdx.x; v < nv; v += gridDim.x * WG) {
        bool ok = true;
        for (uint32_t d = 0; d < 3; ++d) ok = ok && valueOk(pos[3 * (size_t)v + d]) && valueOk(col[3 * (size_t)v + d]);
        u64 k;
        if (!ok) bad |= ERR_VALUE;
        else if (!cellKey(pos + 3 * (size_t)v, inv, k)) bad |= ERR_CELL;
    }
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) if (faces[i] >= nv) bad |= ERR_FACE_ID;
    if (bad) atomicOr(&words[W_ERR], bad);
}
__global__ __launch_bounds__(256) void k_simp_vertex_insert(CellSrc src, uint32_t nv, uint32_t* table, uint32_t mask, uint32_t* words) {
    for (uint32_t v = blockIdx.x * WG + threadIdx.x; v < nv; v += gridDim.x * WG)
        if (!tableInsert(table, mask, v, nv, keyAt(src, v), src)) atomicOr(&words[W_ERR], ERR_LOOP);
}
__global__ __launch_bounds__(256) void k_simp_vertex_find(CellSrc src, uint32_t nv, const uint32_t* __restrict__ table, uint32_t mask, uint32_t* __restrict__ leader, uint32_t* words) {
    for (uint32_t v = blockIdx.x * WG + threadIdx.x; v < nv; v += gridDim.x * WG) {
        bool ok = true;
        leader[v] = tableFind(table, mask, v, nv, keyAt(src, v), src, ok);
        if (!ok) atomicOr(&words[W_ERR], ERR_LOOP);
    }
}
// the cluster number of every vertex: its leader's
__global__ __launch_bounds__(256) void k_simp_cluster_of(const uint32_t* __restrict__ leader, const uint32_t* __restrict__ cnum, uint32_t nv, uint32_t numClusters, uint32_t* __restrict__ cid,
                                                         uint32_t* words) {
    for (uint32_t v = blockIdx.x * WG + threadIdx.x; v < nv; v += gridDim.x * WG) {
        const uint32_t l = leader[v];
        uint32_t c = l < nv ? cnum[l] : EMPTY;
        if (c >= numClusters) { atomicOr(&words[W_ERR], ERR_LOOP); c = 0u; }          // (not reached; numClusters >= 1 wherever a vertex exists)
        cid[v] = c;
    }
}

BF_DEV long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// acc[7 * c ...] += (1, q(position), q(colour)) of every vertex of cluster c.  The lanes of a wave that hold the same cluster number add their values with one
// set of atomics; a lane alone with its number adds its own.
__global__ __launch_bounds__(256) void k_simp_accumulate(const float* __restrict__ pos, const float* __restrict__ col, uint32_t nv, const uint32_t* __restrict__ cid, u64* acc, uint32_t* words) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * WG; base < nv; base += gridDim.x * WG) {
        const uint32_t v = base + threadIdx.x;
        bool pending = v < nv;
        const uint32_t c = pending ? cid[v] : 0u;
        long long q[6];
        for (uint32_t d = 0; d < 3; ++d) { q[d] = pending ? quant(pos[3 * (size_t)v + d]) : 0ll; q[3 + d] = pending ? quant(col[3 * (size_t)v + d]) : 0ll; }
        u64 todo = __ballot(pending);
        uint32_t turns = 0;
        for (; todo && turns < 64u; ++turns) {                          // every turn retires its first lane
            const uint32_t first = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t key = __shfl(c, (int)first, 64);
            const bool mine = pending && c == key;
            const u64 group = __ballot(mine);
            const uint32_t members = (uint32_t)__popcll(group);
            long long s[6];
            if (members == 1u) { for (uint32_t j = 0; j < 6; ++j) s[j] = q[j]; }          // (wave-uniform: `group` is a ballot)
            else { for (uint32_t j = 0; j < 6; ++j) s[j] = wave_sum_ll(mine ? q[j] : 0ll); }
            if (lane == first) {
                u64* a = acc + 7 * (size_t)key;
                atomicAdd(a, (u64)members);
                for (uint32_t j = 0; j < 6; ++j) atomicAdd(a + 1 + j, (u64)s[j]);
            }
            if (mine) pending = false;
            todo &= ~group;
        }
        if (todo) atomicOr(&words[W_ERR], ERR_LOOP);
    }
}
// the representative of every cluster: the member itself where it is alone, the mean of the quantised members otherwise
__global__ __launch_bounds__(256) void k_simp_finalise(const u64* __restrict__ acc, const uint32_t* __restrict__ clusterLeader, const float* __restrict__ pos, const float* __restrict__ col,
                                                       uint32_t nv, uint32_t numClusters, float* __restrict__ repPos, float* __restrict__ repCol, uint32_t* words) {
    for (uint32_t base = blockIdx.x * WG; base < numClusters; base += gridDim.x * WG) {
        const uint32_t c = base + threadIdx.x;
        u64 n = 0ull;
        if (c < numClusters) {
            const u64* a = acc + 7 * (size_t)c;
            n = a[0];
            const uint32_t l = clusterLeader[c];
            if (n == 0ull || n > (u64)nv || l >= nv) { atomicOr(&words[W_ERR], ERR_LOOP); n = 0ull; }          // (not reached)
            else if (n == 1ull) {
                for (uint32_t d = 0; d < 3; ++d) { repPos[3 * (size_t)c + d] = pos[3 * (size_t)l + d]; repCol[3 * (size_t)c + d] = col[3 * (size_t)l + d]; }
            } else {
                for (uint32_t d = 0; d < 3; ++d) { repPos[3 * (size_t)c + d] = meanOf((long long)a[1 + d], n); repCol[3 * (size_t)c + d] = meanOf((long long)a[4 + d], n); }
            }
        }
        const uint32_t m = wave_max_u((uint32_t)n);
        if ((threadIdx.x & 63) == 0 && m) atomicMax(&words[W_LARGEST], m);
    }
}
// faces: a face whose three clusters are not pairwise different is collapsed; ids to cluster numbers
BF_DEV bool collapsed(const uint32_t* __restrict__ fids, uint32_t f) {
    const uint32_t a = fids[3 * (size_t)f], b = fids[3 * (size_t)f + 1], c = fids[3 * (size_t)f + 2];
    return a == b || b == c || a == c;
}
__global__ __launch_bounds__(256) void k_simp_face_ids(const uint32_t* __restrict__ faces, uint32_t n, uint32_t nv, const uint32_t* __restrict__ cid, uint32_t* __restrict__ fids) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) { const uint32_t v = faces[i]; fids[i] = v < nv ? cid[v] : 0u; }          // (v < nv: refused otherwise)
}
__global__ __launch_bounds__(256) void k_simp_face_insert(TriSrc src, uint32_t nf, uint32_t* table, uint32_t mask, uint32_t* words) {
    for (uint32_t f = blockIdx.x * WG + threadIdx.x; f < nf; f += gridDim.x * WG)
        if (!collapsed(src.ids, f) && !tableInsert(table, mask, f, nf, keyAt(src, f), src)) atomicOr(&words[W_ERR], ERR_LOOP);
}
// the lowest face of every sorted triple stays; it marks its three clusters as used
__global__ __launch_bounds__(256) void k_simp_face_find(TriSrc src, uint32_t nf, const uint32_t* __restrict__ table, uint32_t mask, uint32_t numClusters, uint32_t* __restrict__ faceRep,
                                                        uint32_t* __restrict__ used, uint32_t* words) {
    for (uint32_t f = blockIdx.x * WG + threadIdx.x; f < nf; f += gridDim.x * WG) {
        if (collapsed(src.ids, f)) { faceRep[f] = EMPTY; continue; }
        bool ok = true;
        const uint32_t r = tableFind(table, mask, f, nf, keyAt(src, f), src, ok);
        if (!ok) atomicOr(&words[W_ERR], ERR_LOOP);
        faceRep[f] = r;
        if (r == f) for (uint32_t d = 0; d < 3; ++d) { const uint32_t c = src.ids[3 * (size_t)f + d]; if (c < numClusters) used[c] = 1u; }          // every writer writes 1
    }
}

// ---- count / scan / scatter over a predicate: a[i] == i (leaders, kept faces), a[i] != 0 (used clusters) or a[i] == EMPTY (collapsed faces: counted only - one
// atomicAdd per wave on one counter had made the id kernel 0.64 ms for 3.6 M faces, twice the accumulation)
enum { NONZERO = 0, SELF = 1, IS_EMPTY = 2 };
struct Pred {
    const uint32_t* a; int mode;
    BF_DEV bool at(uint32_t i) const { return mode == SELF ? a[i] == i : mode == NONZERO ? a[i] != 0u : a[i] == EMPTY; }
};
__global__ __launch_bounds__(256) void k_simp_tile_count(Pred pred, uint32_t n, uint32_t numTiles, uint32_t* __restrict__ tileCounts) {
    __shared__ uint32_t ws[4];
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; if (i < n && pred.at(i)) ++c; }
        c = (uint32_t)wave_sum_i((int)c);
        if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) tileCounts[tile] = ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}
// exclusive scan of the tile counts in place by one workgroup; the total -> *total
__global__ __launch_bounds__(256) void k_simp_tile_scan(uint32_t* a, uint32_t n, uint32_t* total) {
    __shared__ uint32_t wtot[4];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < n; base += WG) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < n ? a[i] : 0u;
        uint32_t incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += y; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (uint32_t w = 0; w < wave; ++w) woff += wtot[w];
        const uint32_t c0 = carry;
        if (i < n) a[i] = c0 + woff + incl - x;
        __syncthreads();
        if (threadIdx.x == WG - 1) carry = c0 + woff + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
// what a kept element writes at its rank: LEADERS: the cluster number on the leader and the leader of the cluster; VERTS: the output id of the cluster and its
// representative; FACES: the face's output ids
enum { LEADERS = 0, VERTS = 1, FACES = 2 };
struct Scatter {
    uint32_t *cnum, *clusterLeader;                                        // LEADERS
    uint32_t* newId; const float *repPos, *repCol; float *positions, *colors;      // VERTS (newId: FACES too)
    const uint32_t* fids; uint32_t* faces;                                 // FACES
};
template <int MODE>
__global__ __launch_bounds__(256) void k_simp_tile_scatter(Pred pred, uint32_t n, uint32_t numTiles, const uint32_t* __restrict__ tileOffsets, uint32_t capacity, Scatter s) {
    __shared__ uint32_t wscan[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        bool own[4]; uint32_t c = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; own[k] = i < n && pred.at(i); c += own[k] ? 1u : 0u; }
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += y; }
        if (lane == 63) wscan[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (uint32_t w = 0; w < wave; ++w) woff += wscan[w];
        uint32_t at = tileOffsets[tile] + woff + incl - c;
        for (uint32_t k = 0; k < 4; ++k) {
            if (!own[k]) continue;
            const uint32_t i = tile * TILE + threadIdx.x * 4 + k;
            const uint32_t id = at++;
            if (id >= capacity) continue;
            if (MODE == LEADERS) { s.cnum[i] = id; s.clusterLeader[id] = i; }
            else if (MODE == VERTS) {
                s.newId[i] = id;
                for (uint32_t d = 0; d < 3; ++d) { s.positions[3 * (size_t)id + d] = s.repPos[3 * (size_t)i + d]; s.colors[3 * (size_t)id + d] = s.repCol[3 * (size_t)i + d]; }
            } else {
                for (uint32_t d = 0; d < 3; ++d) s.faces[3 * (size_t)id + d] = s.newId[s.fids[3 * (size_t)i + d]];          // a kept face's clusters are used: they have an id
            }
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_simp_map(const uint32_t* __restrict__ cid, const uint32_t* __restrict__ used, const uint32_t* __restrict__ newId, uint32_t nv, uint32_t* __restrict__ map) {
    for (uint32_t v = blockIdx.x * WG + threadIdx.x; v < nv; v += gridDim.x * WG) { const uint32_t c = cid[v]; map[v] = used[c] ? newId[c] : EMPTY; }
}

uint32_t gridFor(size_t n) { return (uint32_t)std::max<size_t>(1, std::min<size_t>((n + WG - 1) / WG, MAX_GRID)); }
uint32_t gridForTiles(uint32_t tiles) { return std::max(1u, std::min(tiles, MAX_GRID)); }

template <typename T>
int grow(Resources& res, T** p, size_t count) { return res.regrow(p, std::max<size_t>(count, 1)); }

bool cellSizeOk(float cellSize) { return cellSize > 0.0f && cellSize < BF_PINF; }          // finite and > 0 (a NaN fails)

void fillStats(bf_mesh_simplify_stats* s, uint32_t nv, uint32_t nf, uint32_t clusters, uint32_t nvOut, uint32_t nfOut, uint32_t gone, uint32_t largest) {
    if (!s) return;
    s->numVerticesIn = nv; s->numFacesIn = nf; s->numClusters = clusters; s->numVerticesOut = nvOut; s->numFacesOut = nfOut;
    s->numFacesCollapsed = gone; s->numFacesDuplicate = nf - nfOut - gone; s->largestCluster = largest;
}

int internalError(MeshSimplify& s, const char* what) {
    s.numVertices = s.numFaces = s.numVerticesIn = 0; s.hasNormals = false;
    set_error("bf_marching_cubes_simplify: %s", what);
    return BF_ERR_INTERNAL;
}

}  // namespace

namespace bf {

int meshsimplify_run(MeshSimplify& s, Resources& res, hipStream_t st, const bf_indexed_mesh& in, const bf_mesh_simplify_params& params, bf_mesh_simplify_stats* stats) {
    const uint32_t nv = in.numVertices, nf = in.numFaces;
    BF_REQUIRE(cellSizeOk(params.cellSize), "cellSize is not a finite number above 0");
    BF_REQUIRE(nf <= MAX_FACES && nv <= MAX_VERTICES, "too many faces or vertices for one simplification");
    BF_REQUIRE((nv == 0 || (in.d_positions && in.d_colors)) && (nf == 0 || in.d_faces), "null mesh array");
    const double inv = 1.0 / (double)params.cellSize;
    if (!s.d_words) BF_TRY(res.device(&s.d_words, NUM_WORDS));

    // ---- the refusals, before any buffer of the last result is touched
    hipLaunchKernelGGL(k_simp_fill, dim3(1), dim3(WG), 0, st, s.d_words, (size_t)NUM_WORDS, 0u);
    hipLaunchKernelGGL(k_simp_validate, dim3(gridFor(std::max<size_t>(nv, 3 * (size_t)nf))), dim3(WG), 0, st, in.d_positions, in.d_colors, nv, in.d_faces, 3u * nf, inv, s.d_words);
    BF_HIP_TRY(hipGetLastError());
    uint32_t words[NUM_WORDS] = {0};
    BF_HIP_TRY(hipMemcpyAsync(words, s.d_words, 4, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));
    BF_REQUIRE(!(words[W_ERR] & ERR_FACE_ID), "a face id is not below numVertices");
    BF_REQUIRE(!(words[W_ERR] & ERR_VALUE), "a position or colour component is not finite or not below 1024 in magnitude");
    BF_REQUIRE(!(words[W_ERR] & ERR_CELL), "a cell index is not below 2^20 in magnitude: cellSize is too small for the mesh");

    s.numVertices = s.numFaces = s.numVerticesIn = 0; s.hasNormals = false;
    uint32_t cap = 1024;
    while (cap < 2u * std::max(nv, nf)) cap <<= 1;
    const uint32_t mask = cap - 1u;
    const uint32_t tilesV = div_up(nv, TILE), tilesF = div_up(nf, TILE);
    if (cap > s.capTable || !s.d_table) { s.capTable = 0; BF_TRY(grow(res, &s.d_table, cap)); s.capTable = cap; }
    if (nv > s.capVerticesIn || !s.d_leader) {
        s.capVerticesIn = 0;
        BF_TRY(grow(res, &s.d_leader, nv)); BF_TRY(grow(res, &s.d_cnum, nv)); BF_TRY(grow(res, &s.d_cid, nv)); BF_TRY(grow(res, &s.d_map, nv)); BF_TRY(grow(res, &s.d_tilesV, tilesV));
        s.capVerticesIn = nv;
    }
    if (nf > s.capFacesIn || !s.d_fids) {
        s.capFacesIn = 0;
        BF_TRY(grow(res, &s.d_fids, 3 * (size_t)nf)); BF_TRY(grow(res, &s.d_faceRep, nf)); BF_TRY(grow(res, &s.d_tilesF, tilesF));
        s.capFacesIn = nf;
    }

    // ---- keys and leaders, the cluster count
    CellSrc cells; cells.pos = in.d_positions; cells.inv = inv;
    Pred leaders; leaders.a = s.d_leader; leaders.mode = SELF;
    hipLaunchKernelGGL(k_simp_fill, dim3(gridFor(cap)), dim3(WG), 0, st, s.d_table, (size_t)cap, EMPTY);
    hipLaunchKernelGGL(k_simp_vertex_insert, dim3(gridFor(nv)), dim3(WG), 0, st, cells, nv, s.d_table, mask, s.d_words);
    hipLaunchKernelGGL(k_simp_vertex_find, dim3(gridFor(nv)), dim3(WG), 0, st, cells, nv, (const uint32_t*)s.d_table, mask, s.d_leader, s.d_words);
    hipLaunchKernelGGL(k_simp_tile_count, dim3(gridForTiles(tilesV)), dim3(WG), 0, st, leaders, nv, tilesV, s.d_tilesV);
    hipLaunchKernelGGL(k_simp_tile_scan, dim3(1), dim3(WG), 0, st, s.d_tilesV, tilesV, s.d_words + W_CLUSTERS);
    BF_HIP_TRY(hipGetLastError());
    BF_HIP_TRY(hipMemcpyAsync(words, s.d_words, sizeof words, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));
    if (words[W_ERR] & ERR_LOOP) return internalError(s, "a probe sequence of the vertex table ran out of slots");
    const uint32_t nc = words[W_CLUSTERS];
    if (nc > nv || (nv && !nc)) return internalError(s, "cluster count out of range");

    // ---- accumulate, finalise
    const uint32_t tilesC = div_up(nc, TILE);
    if (nc > s.capClusters || !s.d_acc) {
        s.capClusters = 0;
        BF_TRY(grow(res, &s.d_acc, 7 * (size_t)nc)); BF_TRY(grow(res, &s.d_clusterLeader, nc)); BF_TRY(grow(res, &s.d_used, nc)); BF_TRY(grow(res, &s.d_newId, nc));
        BF_TRY(grow(res, &s.d_tilesC, tilesC)); BF_TRY(grow(res, &s.d_repPos, 3 * (size_t)nc)); BF_TRY(grow(res, &s.d_repCol, 3 * (size_t)nc));
        s.capClusters = nc;
    }
    Scatter sc; memset(&sc, 0, sizeof sc);
    sc.cnum = s.d_cnum; sc.clusterLeader = s.d_clusterLeader;
    hipLaunchKernelGGL(k_simp_tile_scatter<LEADERS>, dim3(gridForTiles(tilesV)), dim3(WG), 0, st, leaders, nv, tilesV, (const uint32_t*)s.d_tilesV, nc, sc);
    hipLaunchKernelGGL(k_simp_cluster_of, dim3(gridFor(nv)), dim3(WG), 0, st, (const uint32_t*)s.d_leader, (const uint32_t*)s.d_cnum, nv, nc, s.d_cid, s.d_words);
    hipLaunchKernelGGL(k_simp_fill, dim3(gridFor(14 * (size_t)nc)), dim3(WG), 0, st, (uint32_t*)s.d_acc, 14 * (size_t)nc, 0u);
    hipLaunchKernelGGL(k_simp_fill, dim3(gridFor(nc)), dim3(WG), 0, st, s.d_used, (size_t)nc, 0u);
    hipLaunchKernelGGL(k_simp_accumulate, dim3(gridFor(nv)), dim3(WG), 0, st, in.d_positions, in.d_colors, nv, (const uint32_t*)s.d_cid, s.d_acc, s.d_words);
    hipLaunchKernelGGL(k_simp_finalise, dim3(gridFor(nc)), dim3(WG), 0, st, (const u64*)s.d_acc, (const uint32_t*)s.d_clusterLeader, in.d_positions, in.d_colors, nv, nc, s.d_repPos,
                       s.d_repCol, s.d_words);

    // ---- faces: cluster numbers, the lowest face of every sorted triple, the used clusters, the counts
    TriSrc tris; tris.ids = s.d_fids;
    Pred keptFaces; keptFaces.a = s.d_faceRep; keptFaces.mode = SELF;
    Pred goneFaces; goneFaces.a = s.d_faceRep; goneFaces.mode = IS_EMPTY;
    Pred usedClusters; usedClusters.a = s.d_used; usedClusters.mode = NONZERO;
    hipLaunchKernelGGL(k_simp_face_ids, dim3(gridFor(3 * (size_t)nf)), dim3(WG), 0, st, in.d_faces, 3u * nf, nv, (const uint32_t*)s.d_cid, s.d_fids);
    hipLaunchKernelGGL(k_simp_fill, dim3(gridFor(cap)), dim3(WG), 0, st, s.d_table, (size_t)cap, EMPTY);
    hipLaunchKernelGGL(k_simp_face_insert, dim3(gridFor(nf)), dim3(WG), 0, st, tris, nf, s.d_table, mask, s.d_words);
    hipLaunchKernelGGL(k_simp_face_find, dim3(gridFor(nf)), dim3(WG), 0, st, tris, nf, (const uint32_t*)s.d_table, mask, nc, s.d_faceRep, s.d_used, s.d_words);
    hipLaunchKernelGGL(k_simp_tile_count, dim3(gridForTiles(tilesC)), dim3(WG), 0, st, usedClusters, nc, tilesC, s.d_tilesC);
    hipLaunchKernelGGL(k_simp_tile_scan, dim3(1), dim3(WG), 0, st, s.d_tilesC, tilesC, s.d_words + W_NV_OUT);
    hipLaunchKernelGGL(k_simp_tile_count, dim3(gridForTiles(tilesF)), dim3(WG), 0, st, goneFaces, nf, tilesF, s.d_tilesF);
    hipLaunchKernelGGL(k_simp_tile_scan, dim3(1), dim3(WG), 0, st, s.d_tilesF, tilesF, s.d_words + W_COLLAPSED);
    hipLaunchKernelGGL(k_simp_tile_count, dim3(gridForTiles(tilesF)), dim3(WG), 0, st, keptFaces, nf, tilesF, s.d_tilesF);
    hipLaunchKernelGGL(k_simp_tile_scan, dim3(1), dim3(WG), 0, st, s.d_tilesF, tilesF, s.d_words + W_NF_OUT);
    BF_HIP_TRY(hipGetLastError());
    BF_HIP_TRY(hipMemcpyAsync(words, s.d_words, sizeof words, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));
    if (words[W_ERR] & ERR_LOOP) return internalError(s, "a bounded loop ran out of steps");
    const uint32_t nvOut = words[W_NV_OUT], nfOut = words[W_NF_OUT], gone = words[W_COLLAPSED];
    if (nvOut > nc || nfOut > nf || gone > nf - nfOut) return internalError(s, "counts out of range");
    fillStats(stats, nv, nf, nc, nvOut, nfOut, gone, words[W_LARGEST]);

    // ---- compaction, the map
    if (nvOut > s.capVertices || !s.d_positions) {
        s.capVertices = 0;
        BF_TRY(grow(res, &s.d_positions, 3 * (size_t)nvOut)); BF_TRY(grow(res, &s.d_colors, 3 * (size_t)nvOut));
        s.capVertices = nvOut;
    }
    if (nfOut > s.capFaces || !s.d_faces) { s.capFaces = 0; BF_TRY(grow(res, &s.d_faces, 3 * (size_t)nfOut)); s.capFaces = nfOut; }
    sc.newId = s.d_newId; sc.repPos = s.d_repPos; sc.repCol = s.d_repCol; sc.positions = s.d_positions; sc.colors = s.d_colors; sc.fids = s.d_fids; sc.faces = s.d_faces;
    hipLaunchKernelGGL(k_simp_tile_scatter<VERTS>, dim3(gridForTiles(tilesC)), dim3(WG), 0, st, usedClusters, nc, tilesC, (const uint32_t*)s.d_tilesC, nvOut, sc);
    hipLaunchKernelGGL(k_simp_tile_scatter<FACES>, dim3(gridForTiles(tilesF)), dim3(WG), 0, st, keptFaces, nf, tilesF, (const uint32_t*)s.d_tilesF, nfOut, sc);
    hipLaunchKernelGGL(k_simp_map, dim3(gridFor(nv)), dim3(WG), 0, st, (const uint32_t*)s.d_cid, (const uint32_t*)s.d_used, (const uint32_t*)s.d_newId, nv, s.d_map);
    BF_HIP_TRY(hipGetLastError());
    s.numVertices = nvOut; s.numFaces = nfOut; s.numVerticesIn = nv;
    if (!params.computeNormals) return BF_OK;
    BF_TRY(meshnormals_run(s.normals, res, st, s.d_positions, s.d_faces, nvOut, nfOut));
    s.hasNormals = true;
    return BF_OK;
}

}  // namespace bf

namespace {
struct TriHash {
    size_t operator()(const Tri3& t) const { u64 h = t.a * 0x9E3779B97F4A7C15ull; h = (h ^ (h >> 31) ^ t.b) * 0xC2B2AE3D27D4EB4Full; h = (h ^ (h >> 29) ^ t.c) * 0x165667B19E3779F9ull; return (size_t)h; }
};
struct TriEq { bool operator()(const Tri3& p, const Tri3& q) const { return p.a == q.a && p.b == q.b && p.c == q.c; } };
}  // namespace

// The definition on one core: one pass over the vertices in increasing id (a cluster is numbered when its first member, its leader, arrives), one over the faces.
extern "C" int bf_mesh_simplify_host(const float* pos, const float* col, const uint32_t* faces, uint32_t nv, uint32_t nf, const bf_mesh_simplify_params* params, float* posOut, float* colOut,
                                     float* nrmOut, uint32_t* facesOut, uint32_t* mapOut, uint32_t vertexCapacity, uint32_t faceCapacity, bf_mesh_simplify_stats* stats) {
    BF_REQUIRE(params, "null argument");
    BF_REQUIRE(cellSizeOk(params->cellSize), "cellSize is not a finite number above 0");
    BF_REQUIRE(nf <= MAX_FACES && nv <= MAX_VERTICES, "too many faces or vertices for one simplification");
    BF_REQUIRE((nv == 0 || (pos && col)) && (nf == 0 || faces), "null mesh array");
    const double inv = 1.0 / (double)params->cellSize;
    for (size_t i = 0; i < 3 * (size_t)nf; ++i) BF_REQUIRE(faces[i] < nv, "a face id is not below numVertices");
    for (size_t i = 0; i < 3 * (size_t)nv; ++i) BF_REQUIRE(valueOk(pos[i]) && valueOk(col[i]), "a position or colour component is not finite or not below 1024 in magnitude");
    std::vector<uint32_t> cid(nv);
    {
        u64 k;
        for (uint32_t v = 0; v < nv; ++v) BF_REQUIRE(cellKey(pos + 3 * (size_t)v, inv, k), "a cell index is not below 2^20 in magnitude: cellSize is too small for the mesh");
    }
    // clusters
    std::unordered_map<u64, uint32_t> cellOf;
    cellOf.reserve(nv);
    std::vector<uint32_t> leader;
    std::vector<long long> acc;          // 7 per cluster: n, SP, SC
    for (uint32_t v = 0; v < nv; ++v) {
        u64 k; cellKey(pos + 3 * (size_t)v, inv, k);
        const auto at = cellOf.emplace(k, (uint32_t)leader.size());
        if (at.second) { leader.push_back(v); acc.insert(acc.end(), 7, 0ll); }
        const uint32_t c = at.first->second;
        cid[v] = c;
        long long* a = acc.data() + 7 * (size_t)c;
        a[0] += 1;
        for (int d = 0; d < 3; ++d) { a[1 + d] += quant(pos[3 * (size_t)v + d]); a[4 + d] += quant(col[3 * (size_t)v + d]); }
    }
    const uint32_t nc = (uint32_t)leader.size();
    uint32_t largest = 0;
    for (uint32_t c = 0; c < nc; ++c) largest = std::max(largest, (uint32_t)acc[7 * (size_t)c]);
    // faces
    std::unordered_map<Tri3, uint32_t, TriHash, TriEq> seen;
    seen.reserve(nf);
    std::vector<uint32_t> kept;          // face numbers
    std::vector<uint32_t> newId(nc, EMPTY);
    uint32_t gone = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        uint32_t a = cid[faces[3 * (size_t)f]], b = cid[faces[3 * (size_t)f + 1]], c = cid[faces[3 * (size_t)f + 2]], x;
        if (a == b || b == c || a == c) { ++gone; continue; }
        if (a > b) { x = a; a = b; b = x; }
        if (b > c) { x = b; b = c; c = x; }
        if (a > b) { x = a; a = b; b = x; }
        Tri3 t; t.a = a; t.b = b; t.c = c;
        if (!seen.emplace(t, f).second) continue;          // a duplicate of a lower face
        kept.push_back(f);
        newId[a] = newId[b] = newId[c] = 0u;               // used
    }
    uint32_t nvOut = 0;
    for (uint32_t c = 0; c < nc; ++c) if (newId[c] != EMPTY) newId[c] = nvOut++;
    const uint32_t nfOut = (uint32_t)kept.size();
    fillStats(stats, nv, nf, nc, nvOut, nfOut, gone, largest);
    const bool wantsV = posOut || colOut || (nrmOut && params->computeNormals);
    if ((wantsV && nvOut > vertexCapacity) || (facesOut && nfOut > faceCapacity)) { set_error("bf_mesh_simplify_host: the result (%u vertices, %u faces) exceeds the capacity", nvOut, nfOut); return BF_ERR_CAPACITY; }
    // the output mesh, then what the caller asked for of it
    std::vector<float> P(3 * (size_t)nvOut);
    std::vector<uint32_t> F(3 * (size_t)nfOut);
    for (uint32_t c = 0; c < nc; ++c) {
        if (newId[c] == EMPTY) continue;
        const long long* a = acc.data() + 7 * (size_t)c;
        const uint32_t id = newId[c], l = leader[c];
        for (int d = 0; d < 3; ++d) {
            P[3 * (size_t)id + d] = a[0] == 1 ? pos[3 * (size_t)l + d] : meanOf(a[1 + d], (u64)a[0]);
            if (colOut) colOut[3 * (size_t)id + d] = a[0] == 1 ? col[3 * (size_t)l + d] : meanOf(a[4 + d], (u64)a[0]);
        }
    }
    for (uint32_t k = 0; k < nfOut; ++k) for (int d = 0; d < 3; ++d) F[3 * (size_t)k + d] = newId[cid[faces[3 * (size_t)kept[k] + d]]];
    if (posOut && nvOut) memcpy(posOut, P.data(), 12 * (size_t)nvOut);
    if (facesOut && nfOut) memcpy(facesOut, F.data(), 12 * (size_t)nfOut);
    if (mapOut) for (uint32_t v = 0; v < nv; ++v) mapOut[v] = newId[cid[v]];
    if (nrmOut && params->computeNormals) meshnormals_host(P.data(), F.data(), nvOut, nfOut, nrmOut);
    return BF_OK;
}
