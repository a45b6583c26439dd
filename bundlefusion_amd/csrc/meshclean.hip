// Cleaning of an indexed mesh on the device, for gfx950: connected components, the keep rule, compaction and per-vertex normals without the mesh leaving HBM
// (DESIGN.md "Mesh cleaning: the definition"; include/bf_hip.h states it next to bf_marching_cubes_clean).  The reference has no counterpart (mLib is absent);
// bf_mesh_clean_host below is the definition as one sequential loop, tests/mesh_clean_ref.py restates it in numpy, and the kernels are held to both as bits.
//
// Nothing here depends on the order in which threads run: labels are minima over vertex ids, sizes are integer sums, "the largest" is one 64-bit maximum over
// (size << 32) | ~label, and the one float sum (a vertex's normal) runs in increasing corner number.  No float atomics anywhere.
//
// Labelling: parent[v] = v, then k_clean_hook unites (a, b) and (b, c) of every face, lock-free.  unite() finds the two roots and hangs the LARGER root under the
// smaller one with atomicCAS(&parent[hi], hi, lo); a CAS that fails returns hi's new parent, from which the search goes on.  find() shortens the path it walks with
// atomicMin(&parent[x], grandparent).  So parent[v] <= v throughout, a value only ever decreases and only ever to a vertex of the same component, a root is its
// tree's lowest id, and the final root of a component is its lowest id whatever the interleaving.  Coherence (meshweld.hip:16-17 has the same rule for its table):
// inside k_clean_hook parent[] is read through an atomic's return value or an agent-scope relaxed atomic load, never a plain load, which this CU's L1 or another
// XCD's L2 may serve stale (a stale parent is still an ancestor in the same component: it would cost trips, not correctness).  k_clean_flatten starts after the
// hook kernel has ended and reads parent[] with plain loads.
// Every device loop is bounded: a walk towards a root strictly decreases the id (at most numVertices steps), and a unite retries only after another thread's
// successful hook, of which there are fewer than numVertices.  Exhaustion sets a bit of the error word, which the host turns into BF_ERR_INTERNAL; no kernel waits
// for another workgroup and nothing spins.
//
// Counting and compaction: the weld's scheme (meshweld.hip:20) driven by a predicate - tiles of 1024 elements, count per tile, one scan of the tile counts by one
// workgroup, scatter.  The normals' vertex-to-corner incidence is in CSR form: integer degree count, an exclusive scan of the degrees (tile sums, the same scan of
// the tile sums, a scan inside every tile), an atomic-cursor fill in whatever order, and the defined order restored per segment: a segment of at most 64 corners is
// walked by one thread that picks the next higher corner number each time; a longer one is rank-sorted and then summed by one wave, 64 face normals at a time.
// The normal pass is a function of its own (meshnormals_run, and meshnormals_host for the one-core route): the simplification (meshsimplify.hip) calls it too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bf_device.h"
#include "bf_resources.h"
#include "bf_meshclean.h"

using namespace bf;

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t TILE = 1024;                 // 4 consecutive elements per thread
constexpr uint32_t MAX_GRID = 8192;
constexpr uint32_t MAX_FACES = 300000000u;      // 3 * numFaces corner numbers stay below 2^32
constexpr uint32_t SHORT_SEGMENT = 64;          // corners of a vertex one thread orders by itself
constexpr uint32_t NO_CORNER = 0xFFFFFFFFu;

// the control words (uint32, zeroed by k_clean_init)
enum : uint32_t { W_ERR = 0, W_NV_OUT = 1, W_NF_OUT = 2, W_COMPONENTS = 3, W_PASSING = 4, W_ISOLATED = 5, W_LARGEST = 6, W_BEST = 8 /* 64 bits */, NUM_WORDS = 16 };
constexpr uint32_t ERR_FACE_ID = 1u, ERR_LOOP = 2u;

// ---- the arithmetic of the normals, shared by the kernels and bf_mesh_clean_host (the library is built without contraction: one rounding per operation)
BF_HD f3 faceNormal(const float* __restrict__ P, const uint32_t* __restrict__ faces, uint32_t f) {
    const uint32_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    const f3 pa = mk3(P[3 * (size_t)a], P[3 * (size_t)a + 1], P[3 * (size_t)a + 2]);
    const f3 e1 = mk3(P[3 * (size_t)b], P[3 * (size_t)b + 1], P[3 * (size_t)b + 2]) - pa;
    const f3 e2 = mk3(P[3 * (size_t)c], P[3 * (size_t)c + 1], P[3 * (size_t)c + 2]) - pa;
    return cross3(e1, e2);
}
BF_HD f3 unitOrZero(f3 s) {
    const float l = __builtin_sqrtf((s.x * s.x + s.y * s.y) + s.z * s.z);
    if (!(l > 0.0f && l < BF_PINF)) return mk3(0.0f, 0.0f, 0.0f);
    return mk3(s.x / l, s.y / l, s.z / l);
}

// the kernels' form: a corner slot or a face id that is out of range (a bug upstream, never the input: that is refused) contributes nothing and reads nothing
BF_DEV f3 faceNormalAt(const float* __restrict__ P, const uint32_t* __restrict__ faces, uint32_t corner, uint32_t nf, uint32_t nv) {
    const uint32_t f = corner / 3u;
    if (f >= nf || faces[3 * (size_t)f] >= nv || faces[3 * (size_t)f + 1] >= nv || faces[3 * (size_t)f + 2] >= nv) return mk3(0.0f, 0.0f, 0.0f);
    return faceNormal(P, faces, f);
}

// ---- labelling
BF_DEV uint32_t loadAgent(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x at some moment of the walk; every step goes to a lower id
BF_DEV uint32_t findRoot(uint32_t* parent, uint32_t x, uint32_t nv, bool& ok) {
    for (uint32_t steps = 0; steps <= nv; ++steps) {
        const uint32_t p = loadAgent(&parent[x]);
        if (p == x) return x;
        const uint32_t g = loadAgent(&parent[p]);
        if (g == p) return p;
        atomicMin(&parent[x], g);
        x = g;
    }
    ok = false;
    return x;
}
BF_DEV bool unite(uint32_t* parent, uint32_t u, uint32_t v, uint32_t nv) {
    bool ok = true;
    for (uint32_t tries = 0; tries <= nv; ++tries) {
        u = findRoot(parent, u, nv, ok);
        v = findRoot(parent, v, nv, ok);
        if (!ok) return false;
        if (u == v) return true;
        if (u < v) { const uint32_t x = u; u = v; v = x; }
        const uint32_t old = atomicCAS(&parent[u], u, v);          // u > v: the larger root goes under the smaller
        if (old == u) return true;
        u = old;                                                    // somebody hung u under `old` first
    }
    return false;
}

__global__ __launch_bounds__(256) void k_clean_fill(uint32_t* __restrict__ a, uint32_t n, uint32_t v) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) a[i] = v;
}
__global__ __launch_bounds__(256) void k_clean_init(uint32_t* __restrict__ parent, uint32_t* __restrict__ count, uint32_t nv, uint32_t* __restrict__ words) {
    if (blockIdx.x == 0 && threadIdx.x < NUM_WORDS) words[threadIdx.x] = 0u;
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < nv; i += gridDim.x * WG) { parent[i] = i; count[i] = 0u; }
}
__global__ __launch_bounds__(256) void k_clean_validate(const uint32_t* __restrict__ faces, uint32_t n, uint32_t nv, uint32_t* words) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) bad = bad || faces[i] >= nv;
    if (bad) atomicOr(&words[W_ERR], ERR_FACE_ID);
}
__global__ __launch_bounds__(256) void k_clean_hook(const uint32_t* __restrict__ faces, uint32_t nf, uint32_t nv, uint32_t* parent, uint32_t* words) {
    for (uint32_t f = blockIdx.x * WG + threadIdx.x; f < nf; f += gridDim.x * WG) {
        const uint32_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        if (a >= nv || b >= nv || c >= nv) { atomicOr(&words[W_ERR], ERR_FACE_ID); continue; }          // (refused before this kernel is launched)
        const bool ok1 = unite(parent, a, b, nv);
        const bool ok2 = unite(parent, b, c, nv);          // the third edge adds nothing
        if (!ok1 || !ok2) atomicOr(&words[W_ERR], ERR_LOOP);
    }
}
__global__ __launch_bounds__(256) void k_clean_flatten(const uint32_t* __restrict__ parent, uint32_t nv, uint32_t* __restrict__ label, uint32_t* words) {
    for (uint32_t v = blockIdx.x * WG + threadIdx.x; v < nv; v += gridDim.x * WG) {
        uint32_t r = v; bool done = false;
        for (uint32_t steps = 0; steps <= nv; ++steps) {
            const uint32_t p = parent[r];
            if (p == r || p >= nv) { done = p == r; break; }
            r = p;
        }
        if (!done) atomicOr(&words[W_ERR], ERR_LOOP);
        label[v] = r;
    }
}
// a face belongs to the component of its vertices: of its first one.  Neighbouring faces mostly share a component, and a scan is mostly one component: the lanes
// of a wave that hold the same label add their number with one atomic (one atomic per face was 19 ms for 3.6 M faces, nearly all of them on one counter).
__global__ __launch_bounds__(256) void k_clean_count(const uint32_t* __restrict__ faces, uint32_t nf, const uint32_t* __restrict__ label, uint32_t* count) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * WG; base < nf; base += gridDim.x * WG) {
        const uint32_t f = base + threadIdx.x;
        bool pending = f < nf;
        const uint32_t l = pending ? label[faces[3 * (size_t)f]] : 0u;
        unsigned long long todo = __ballot(pending);
        while (todo) {                                                  // at most 64 turns: every turn retires its leader
            const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t key = __shfl(l, (int)leader, 64);
            const bool mine = pending && l == key;
            const unsigned long long same = __ballot(mine);
            if (lane == leader) atomicAdd(&count[key], (uint32_t)__popcll(same));
            if (mine) pending = false;
            todo &= ~same;
        }
    }
}
// per root: the statistics and the greatest passing component.  A root without faces is an isolated vertex (a vertex of any face has a face in its component).
__global__ __launch_bounds__(256) void k_clean_decide(const uint32_t* __restrict__ label, const uint32_t* __restrict__ count, uint32_t nv, uint32_t threshold, uint32_t* words) {
    for (uint32_t base = blockIdx.x * WG; base < nv; base += gridDim.x * WG) {
        const uint32_t v = base + threadIdx.x;
        const bool root = v < nv && label[v] == v;
        const uint32_t size = root ? count[v] : 0u;
        const bool comp = root && size >= 1u, pass = comp && size >= threshold;
        const int nc = wave_sum_i(comp ? 1 : 0), np = wave_sum_i(pass ? 1 : 0), ni = wave_sum_i(root && size == 0u ? 1 : 0);
        if ((threadIdx.x & 63) == 0) {
            if (nc) atomicAdd(&words[W_COMPONENTS], (uint32_t)nc);
            if (np) atomicAdd(&words[W_PASSING], (uint32_t)np);
            if (ni) atomicAdd(&words[W_ISOLATED], (uint32_t)ni);
        }
        if (comp) atomicMax(&words[W_LARGEST], size);
        if (pass) atomicMax(reinterpret_cast<unsigned long long*>(words + W_BEST), ((unsigned long long)size << 32) | (unsigned long long)(~v));          // equal sizes: the lowest label
    }
}

// ---- the keep rule as a predicate over vertices (FACES: over faces, through the first vertex), read after k_clean_decide has ended
struct Keep {
    const uint32_t *label, *count, *faces, *words;
    uint32_t threshold; int largest;
    template <bool FACES>
    BF_DEV bool at(uint32_t i) const {
        const uint32_t l = label[FACES ? faces[3 * (size_t)i] : i];
        if (count[l] < threshold) return false;
        if (!largest) return true;
        const unsigned long long best = *reinterpret_cast<const unsigned long long*>(words + W_BEST);
        return best != 0ull && l == ~(uint32_t)best;
    }
};

template <bool FACES>
__global__ __launch_bounds__(256) void k_clean_tile_count(Keep keep, uint32_t n, uint32_t numTiles, uint32_t* __restrict__ tileCounts) {
    __shared__ uint32_t ws[4];
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; if (i < n && keep.at<FACES>(i)) ++c; }
        c = (uint32_t)wave_sum_i((int)c);
        if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) tileCounts[tile] = ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}
// sums of tiles of 1024 values (the general scan's first step)
__global__ __launch_bounds__(256) void k_clean_tile_sum(const uint32_t* __restrict__ in, uint32_t n, uint32_t numTiles, uint32_t* __restrict__ tileSums) {
    __shared__ uint32_t ws[4];
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; if (i < n) c += in[i]; }
        c = (uint32_t)wave_sum_i((int)c);
        if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) tileSums[tile] = ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}
// exclusive scan of n values in place by one workgroup (one value per tile, not per element); the total -> *total
__global__ __launch_bounds__(256) void k_clean_tile_scan(uint32_t* a, uint32_t n, uint32_t* total) {
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
// the general scan's last step: out[i] = tile offset + the sum of the tile's values before i
__global__ __launch_bounds__(256) void k_clean_tile_exscan(const uint32_t* __restrict__ in, uint32_t n, uint32_t numTiles, const uint32_t* __restrict__ tileOffsets, uint32_t* __restrict__ out) {
    __shared__ uint32_t wscan[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        uint32_t x[4], c = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; x[k] = i < n ? in[i] : 0u; c += x[k]; }
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += y; }
        if (lane == 63) wscan[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (uint32_t w = 0; w < wave; ++w) woff += wscan[w];
        uint32_t pos = tileOffsets[tile] + woff + incl - c;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; if (i < n) out[i] = pos; pos += x[k]; }
        __syncthreads();
    }
}
// rank of the tile's kept elements behind the tile's offset; vertices: write the new id, position and colour; faces: write the remapped ids
template <bool FACES>
__global__ __launch_bounds__(256) void k_clean_tile_scatter(Keep keep, uint32_t n, uint32_t numTiles, const uint32_t* __restrict__ tileOffsets, uint32_t capacity,
                                                            const float* __restrict__ inPos, const float* __restrict__ inCol, uint32_t* __restrict__ newId,
                                                            float* __restrict__ positions, float* __restrict__ colors, uint32_t* __restrict__ faces) {
    __shared__ uint32_t wscan[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < numTiles; tile += gridDim.x) {
        bool own[4]; uint32_t c = 0;
        for (uint32_t k = 0; k < 4; ++k) { const uint32_t i = tile * TILE + threadIdx.x * 4 + k; own[k] = i < n && keep.at<FACES>(i); c += own[k] ? 1u : 0u; }
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += y; }
        if (lane == 63) wscan[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
        for (uint32_t w = 0; w < wave; ++w) woff += wscan[w];
        uint32_t pos = tileOffsets[tile] + woff + incl - c;
        for (uint32_t k = 0; k < 4; ++k) {
            if (!own[k]) continue;
            const uint32_t i = tile * TILE + threadIdx.x * 4 + k;
            const uint32_t id = pos++;
            if (id >= capacity) continue;
            if (!FACES) {
                newId[i] = id;
                for (uint32_t d = 0; d < 3; ++d) { positions[3 * (size_t)id + d] = inPos[3 * (size_t)i + d]; colors[3 * (size_t)id + d] = inCol[3 * (size_t)i + d]; }
            } else {
                for (uint32_t d = 0; d < 3; ++d) faces[3 * (size_t)id + d] = newId[keep.faces[3 * (size_t)i + d]];
            }
        }
        __syncthreads();
    }
}

// ---- normals, over the OUTPUT mesh (n = 3 * numFaces corners)
__global__ __launch_bounds__(256) void k_clean_degree(const uint32_t* __restrict__ faces, uint32_t n, uint32_t nv, uint32_t* degree) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) if (faces[i] < nv) atomicAdd(&degree[faces[i]], 1u);
}
// the cursor counts the degree down to zero: every corner of a vertex gets a slot of its own in the vertex's segment, in whatever order
__global__ __launch_bounds__(256) void k_clean_corner_fill(const uint32_t* __restrict__ faces, uint32_t n, uint32_t nv, uint32_t* degree, const uint32_t* __restrict__ offset, uint32_t* __restrict__ corners) {
    for (uint32_t i = blockIdx.x * WG + threadIdx.x; i < n; i += gridDim.x * WG) {
        const uint32_t v = faces[i];
        if (v >= nv) continue;
        const uint32_t slot = atomicSub(&degree[v], 1u) - 1u;
        if (slot < offset[v + 1] - offset[v]) corners[offset[v] + slot] = i;
    }
}
// one thread per vertex: a short segment is summed in increasing corner number by picking the lowest corner above the last one each time; a long one is listed
__global__ __launch_bounds__(256) void k_clean_normals_short(const float* __restrict__ P, const uint32_t* __restrict__ faces, uint32_t nf, uint32_t nv, const uint32_t* __restrict__ offset,
                                                             const uint32_t* __restrict__ corners, float* __restrict__ normals, uint32_t* __restrict__ longList, uint32_t longCapacity,
                                                             uint32_t* numLongWord) {
    for (uint32_t v = blockIdx.x * WG + threadIdx.x; v < nv; v += gridDim.x * WG) {
        const uint32_t s = offset[v], d = offset[v + 1] - s;
        if (d > SHORT_SEGMENT) {
            const uint32_t at = atomicAdd(numLongWord, 1u);
            if (at < longCapacity) longList[at] = v;
            continue;
        }
        f3 S = mk3(0.0f, 0.0f, 0.0f);
        uint32_t lower = 0;
        for (uint32_t k = 0; k < d; ++k) {
            uint32_t next = NO_CORNER;
            for (uint32_t j = 0; j < d; ++j) { const uint32_t c = corners[s + j]; if (c >= lower && c < next) next = c; }
            if (next == NO_CORNER) break;
            S = S + faceNormalAt(P, faces, next, nf, nv);
            lower = next + 1u;
        }
        const f3 nrm = unitOrZero(S);
        normals[3 * (size_t)v] = nrm.x; normals[3 * (size_t)v + 1] = nrm.y; normals[3 * (size_t)v + 2] = nrm.z;
    }
}
// one wave per long segment: the rank of a corner number is the count of lower ones in its segment (corner numbers are all different)
__global__ __launch_bounds__(256) void k_clean_sort_long(const uint32_t* __restrict__ longList, const uint32_t* __restrict__ numLongWord, uint32_t longCapacity, uint32_t nv, const uint32_t* __restrict__ offset,
                                                         const uint32_t* __restrict__ corners, uint32_t* __restrict__ sorted) {
    const uint32_t numLong = min(*numLongWord, longCapacity);
    const uint32_t lane = threadIdx.x & 63, wave = blockIdx.x * (WG / 64) + (threadIdx.x >> 6), numWaves = gridDim.x * (WG / 64);
    for (uint32_t li = wave; li < numLong; li += numWaves) {
        const uint32_t v = longList[li];
        if (v >= nv) continue;
        const uint32_t s = offset[v], d = offset[v + 1] - s;
        for (uint32_t j = lane; j < d; j += 64) {
            const uint32_t c = corners[s + j];
            uint32_t rank = 0;
            for (uint32_t k = 0; k < d; ++k) rank += corners[s + k] < c ? 1u : 0u;
            sorted[s + rank] = c;
        }
    }
}
// after the sort kernel has ended: 64 face normals at a time, added lane by lane in every lane alike
__global__ __launch_bounds__(256) void k_clean_normals_long(const float* __restrict__ P, const uint32_t* __restrict__ faces, uint32_t nf, uint32_t nv, const uint32_t* __restrict__ longList,
                                                            const uint32_t* __restrict__ numLongWord, uint32_t longCapacity, const uint32_t* __restrict__ offset,
                                                            const uint32_t* __restrict__ sorted, float* __restrict__ normals) {
    const uint32_t numLong = min(*numLongWord, longCapacity);
    const uint32_t lane = threadIdx.x & 63, wave = blockIdx.x * (WG / 64) + (threadIdx.x >> 6), numWaves = gridDim.x * (WG / 64);
    for (uint32_t li = wave; li < numLong; li += numWaves) {
        const uint32_t v = longList[li];
        if (v >= nv) continue;
        const uint32_t s = offset[v], d = offset[v + 1] - s;
        f3 S = mk3(0.0f, 0.0f, 0.0f);
        for (uint32_t base = 0; base < d; base += 64) {
            const uint32_t j = base + lane, m = min(64u, d - base);
            const f3 N = j < d ? faceNormalAt(P, faces, sorted[s + j], nf, nv) : mk3(0.0f, 0.0f, 0.0f);
            for (uint32_t k = 0; k < m; ++k) S = S + mk3(__shfl(N.x, (int)k, 64), __shfl(N.y, (int)k, 64), __shfl(N.z, (int)k, 64));
        }
        const f3 nrm = unitOrZero(S);
        if (lane == 0) { normals[3 * (size_t)v] = nrm.x; normals[3 * (size_t)v + 1] = nrm.y; normals[3 * (size_t)v + 2] = nrm.z; }
    }
}

uint32_t gridFor(uint32_t n) { return std::max(1u, std::min(div_up(n, WG), MAX_GRID)); }
uint32_t gridForTiles(uint32_t tiles) { return std::max(1u, std::min(tiles, MAX_GRID)); }

template <typename T>
int grow(Resources& res, T** p, size_t count) { return res.regrow(p, std::max<size_t>(count, 1)); }

void fillStats(bf_mesh_clean_stats* s, uint32_t nv, uint32_t nf, uint32_t nvOut, uint32_t nfOut, uint32_t comps, uint32_t kept, uint32_t isolated, uint32_t largest) {
    if (!s) return;
    s->numVerticesIn = nv; s->numFacesIn = nf; s->numVerticesOut = nvOut; s->numFacesOut = nfOut;
    s->numComponents = comps; s->numComponentsKept = kept; s->numIsolatedVertices = isolated; s->largestComponentFaces = largest;
}

}  // namespace

namespace bf {

int meshclean_run(MeshClean& c, Resources& res, hipStream_t st, const bf_indexed_mesh& in, const bf_mesh_clean_params& params, bf_mesh_clean_stats* stats) {
    const uint32_t nv = in.numVertices, nf = in.numFaces;
    BF_REQUIRE(nf <= MAX_FACES, "too many faces for one clean");
    BF_REQUIRE((nv == 0 || (in.d_positions && in.d_colors)) && (nf == 0 || in.d_faces), "null mesh array");
    const uint32_t threshold = std::max(1u, params.minComponentFaces);
    const int largest = params.keepLargestOnly ? 1 : 0;
    const uint32_t tilesV = div_up(nv, TILE), tilesF = div_up(nf, TILE);
    if (nv > c.capVerticesIn || !c.d_parent) {
        c.capVerticesIn = 0;
        BF_TRY(grow(res, &c.d_parent, nv)); BF_TRY(grow(res, &c.d_label, nv)); BF_TRY(grow(res, &c.d_count, nv)); BF_TRY(grow(res, &c.d_newId, nv));
        BF_TRY(grow(res, &c.d_tilesV, tilesV));
        c.capVerticesIn = nv;
    }
    if (nf > c.capFacesIn || !c.d_tilesF) { c.capFacesIn = 0; BF_TRY(grow(res, &c.d_tilesF, tilesF)); c.capFacesIn = nf; }
    if (!c.d_words) BF_TRY(res.device(&c.d_words, NUM_WORDS));

    // ---- refuse a face id beyond the vertices before anything else reads the faces
    hipLaunchKernelGGL(k_clean_init, dim3(gridFor(nv)), dim3(WG), 0, st, c.d_parent, c.d_count, nv, c.d_words);
    hipLaunchKernelGGL(k_clean_validate, dim3(gridFor(3u * nf)), dim3(WG), 0, st, in.d_faces, 3u * nf, nv, c.d_words);
    BF_HIP_TRY(hipGetLastError());
    uint32_t words[NUM_WORDS] = {0};
    BF_HIP_TRY(hipMemcpyAsync(words, c.d_words, 4, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));
    BF_REQUIRE(!(words[W_ERR] & ERR_FACE_ID), "a face id is not below numVertices");

    // ---- components, the keep rule, the counts
    Keep keep; keep.label = c.d_label; keep.count = c.d_count; keep.faces = in.d_faces; keep.words = c.d_words; keep.threshold = threshold; keep.largest = largest;
    hipLaunchKernelGGL(k_clean_hook, dim3(gridFor(nf)), dim3(WG), 0, st, in.d_faces, nf, nv, c.d_parent, c.d_words);
    hipLaunchKernelGGL(k_clean_flatten, dim3(gridFor(nv)), dim3(WG), 0, st, (const uint32_t*)c.d_parent, nv, c.d_label, c.d_words);
    c.numVerticesIn = nv;          // d_label is the new input's from here on
    hipLaunchKernelGGL(k_clean_count, dim3(gridFor(nf)), dim3(WG), 0, st, in.d_faces, nf, (const uint32_t*)c.d_label, c.d_count);
    hipLaunchKernelGGL(k_clean_decide, dim3(gridFor(nv)), dim3(WG), 0, st, (const uint32_t*)c.d_label, (const uint32_t*)c.d_count, nv, threshold, c.d_words);
    hipLaunchKernelGGL(k_clean_tile_count<false>, dim3(gridForTiles(tilesV)), dim3(WG), 0, st, keep, nv, tilesV, c.d_tilesV);
    hipLaunchKernelGGL(k_clean_tile_scan, dim3(1), dim3(WG), 0, st, c.d_tilesV, tilesV, c.d_words + W_NV_OUT);
    hipLaunchKernelGGL(k_clean_tile_count<true>, dim3(gridForTiles(tilesF)), dim3(WG), 0, st, keep, nf, tilesF, c.d_tilesF);
    hipLaunchKernelGGL(k_clean_tile_scan, dim3(1), dim3(WG), 0, st, c.d_tilesF, tilesF, c.d_words + W_NF_OUT);
    BF_HIP_TRY(hipGetLastError());
    BF_HIP_TRY(hipMemcpyAsync(words, c.d_words, sizeof words, hipMemcpyDeviceToHost, st));
    BF_HIP_TRY(hipStreamSynchronize(st));
    c.numVertices = c.numFaces = 0; c.hasNormals = false; c.hasResult = false;
    if (words[W_ERR] & ERR_LOOP) { set_error("bf_marching_cubes_clean: a bounded loop of the labelling ran out of steps"); return BF_ERR_INTERNAL; }
    const uint32_t nvOut = words[W_NV_OUT], nfOut = words[W_NF_OUT];
    if (nvOut > nv || nfOut > nf) { set_error("bf_marching_cubes_clean: counts out of range"); return BF_ERR_INTERNAL; }
    unsigned long long best; memcpy(&best, words + W_BEST, 8);
    fillStats(stats, nv, nf, nvOut, nfOut, words[W_COMPONENTS], largest ? (best != 0ull ? 1u : 0u) : words[W_PASSING], words[W_ISOLATED], words[W_LARGEST]);

    // ---- compaction
    if (nvOut > c.capVertices || !c.d_positions) {
        c.capVertices = 0;
        BF_TRY(grow(res, &c.d_positions, 3 * (size_t)nvOut)); BF_TRY(grow(res, &c.d_colors, 3 * (size_t)nvOut));
        c.capVertices = nvOut;
    }
    if (nfOut > c.capFaces || !c.d_faces) { c.capFaces = 0; BF_TRY(grow(res, &c.d_faces, 3 * (size_t)nfOut)); c.capFaces = nfOut; }
    hipLaunchKernelGGL(k_clean_tile_scatter<false>, dim3(gridForTiles(tilesV)), dim3(WG), 0, st, keep, nv, tilesV, (const uint32_t*)c.d_tilesV, nvOut, in.d_positions, in.d_colors,
                       c.d_newId, c.d_positions, c.d_colors, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_clean_tile_scatter<true>, dim3(gridForTiles(tilesF)), dim3(WG), 0, st, keep, nf, tilesF, (const uint32_t*)c.d_tilesF, nfOut, (const float*)nullptr,
                       (const float*)nullptr, c.d_newId, (float*)nullptr, (float*)nullptr, c.d_faces);
    BF_HIP_TRY(hipGetLastError());
    c.numVertices = nvOut; c.numFaces = nfOut;
    c.hasResult = true;
    if (!params.computeNormals) return BF_OK;
    BF_TRY(meshnormals_run(c.normals, res, st, c.d_positions, c.d_faces, nvOut, nfOut));
    c.hasNormals = true;
    return BF_OK;
}

int meshnormals_run(MeshNormals& c, Resources& res, hipStream_t st, const float* d_positions, const uint32_t* d_faces, uint32_t nvOut, uint32_t nfOut) {
    const uint32_t n = 3u * nfOut, tilesN = div_up(nvOut, TILE), longCap = n / (SHORT_SEGMENT + 1u) + 1u;
    if (!c.d_numLong) BF_TRY(res.device(&c.d_numLong, 1));
    if (nvOut > c.capNormalVertices || !c.d_degree) {
        c.capNormalVertices = 0;
        BF_TRY(grow(res, &c.d_degree, nvOut)); BF_TRY(grow(res, &c.d_offset, (size_t)nvOut + 1)); BF_TRY(grow(res, &c.d_tilesN, tilesN));
        c.capNormalVertices = nvOut;
    }
    if (nfOut > c.capNormalFaces || !c.d_corners) {
        c.capNormalFaces = 0;
        BF_TRY(grow(res, &c.d_corners, n)); BF_TRY(grow(res, &c.d_sorted, n)); BF_TRY(grow(res, &c.d_long, longCap));
        c.capNormalFaces = nfOut;
    }
    if (nvOut > c.capNormals || !c.d_normals) { c.capNormals = 0; BF_TRY(grow(res, &c.d_normals, 3 * (size_t)nvOut)); c.capNormals = nvOut; }
    hipLaunchKernelGGL(k_clean_fill, dim3(1), dim3(WG), 0, st, c.d_numLong, 1u, 0u);
    hipLaunchKernelGGL(k_clean_fill, dim3(gridFor(nvOut)), dim3(WG), 0, st, c.d_degree, nvOut, 0u);
    hipLaunchKernelGGL(k_clean_degree, dim3(gridFor(n)), dim3(WG), 0, st, d_faces, n, nvOut, c.d_degree);
    hipLaunchKernelGGL(k_clean_tile_sum, dim3(gridForTiles(tilesN)), dim3(WG), 0, st, (const uint32_t*)c.d_degree, nvOut, tilesN, c.d_tilesN);
    hipLaunchKernelGGL(k_clean_tile_scan, dim3(1), dim3(WG), 0, st, c.d_tilesN, tilesN, c.d_offset + nvOut);
    hipLaunchKernelGGL(k_clean_tile_exscan, dim3(gridForTiles(tilesN)), dim3(WG), 0, st, (const uint32_t*)c.d_degree, nvOut, tilesN, (const uint32_t*)c.d_tilesN, c.d_offset);
    hipLaunchKernelGGL(k_clean_corner_fill, dim3(gridFor(n)), dim3(WG), 0, st, d_faces, n, nvOut, c.d_degree, (const uint32_t*)c.d_offset, c.d_corners);
    hipLaunchKernelGGL(k_clean_normals_short, dim3(gridFor(nvOut)), dim3(WG), 0, st, d_positions, d_faces, nfOut, nvOut, (const uint32_t*)c.d_offset,
                       (const uint32_t*)c.d_corners, c.d_normals, c.d_long, longCap, c.d_numLong);
    const uint32_t longGrid = std::max(1u, std::min(div_up(longCap, WG / 64), 2048u));
    hipLaunchKernelGGL(k_clean_sort_long, dim3(longGrid), dim3(WG), 0, st, (const uint32_t*)c.d_long, (const uint32_t*)c.d_numLong, longCap, nvOut, (const uint32_t*)c.d_offset,
                       (const uint32_t*)c.d_corners, c.d_sorted);
    hipLaunchKernelGGL(k_clean_normals_long, dim3(longGrid), dim3(WG), 0, st, d_positions, d_faces, nfOut, nvOut, (const uint32_t*)c.d_long,
                       (const uint32_t*)c.d_numLong, longCap, (const uint32_t*)c.d_offset, (const uint32_t*)c.d_sorted, c.d_normals);
    BF_HIP_TRY(hipGetLastError());
    return BF_OK;
}

void meshnormals_host(const float* P, const uint32_t* F, uint32_t nvOut, uint32_t nfOut, float* nrmOut) {
    std::vector<f3> S(nvOut, mk3(0.0f, 0.0f, 0.0f));
    for (uint32_t f = 0; f < nfOut; ++f) {          // corners in increasing number 3f + c
        const f3 N = faceNormal(P, F, f);
        for (int d = 0; d < 3; ++d) { f3& s = S[F[3 * (size_t)f + d]]; s = s + N; }
    }
    for (uint32_t v = 0; v < nvOut; ++v) { const f3 nrm = unitOrZero(S[v]); nrmOut[3 * (size_t)v] = nrm.x; nrmOut[3 * (size_t)v + 1] = nrm.y; nrmOut[3 * (size_t)v + 2] = nrm.z; }
}

}  // namespace bf

// The definition on one core: a sequential union-find that always hangs the larger root under the smaller, then the rules in the order the header states them.
extern "C" int bf_mesh_clean_host(const float* pos, const float* col, const uint32_t* faces, uint32_t nv, uint32_t nf, const bf_mesh_clean_params* params, float* posOut, float* colOut,
                                  float* nrmOut, uint32_t* facesOut, uint32_t* labelsOut, uint32_t vertexCapacity, uint32_t faceCapacity, bf_mesh_clean_stats* stats) {
    BF_REQUIRE(params, "null argument");
    BF_REQUIRE(nf <= MAX_FACES, "too many faces for one clean");
    BF_REQUIRE((nv == 0 || (pos && col)) && (nf == 0 || faces), "null mesh array");
    for (size_t i = 0; i < 3 * (size_t)nf; ++i) BF_REQUIRE(faces[i] < nv, "a face id is not below numVertices");
    std::vector<uint32_t> parent(nv), count(nv, 0u), newId(nv, 0u);
    for (uint32_t v = 0; v < nv; ++v) parent[v] = v;
    auto find = [&](uint32_t x) {
        uint32_t r = x;
        while (parent[r] != r) r = parent[r];
        while (parent[x] != r) { const uint32_t p = parent[x]; parent[x] = r; x = p; }
        return r;
    };
    auto unite = [&](uint32_t u, uint32_t v) { u = find(u); v = find(v); if (u != v) parent[std::max(u, v)] = std::min(u, v); };
    for (uint32_t f = 0; f < nf; ++f) { unite(faces[3 * (size_t)f], faces[3 * (size_t)f + 1]); unite(faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]); }
    for (uint32_t v = 0; v < nv; ++v) parent[v] = find(v);          // parent[] is the label array from here on
    for (uint32_t f = 0; f < nf; ++f) ++count[parent[faces[3 * (size_t)f]]];
    const uint32_t threshold = std::max(1u, params->minComponentFaces);
    uint32_t comps = 0, passing = 0, isolated = 0, largestSize = 0, bestSize = 0, bestLabel = 0;
    for (uint32_t v = 0; v < nv; ++v) {
        if (parent[v] != v) continue;
        if (count[v] == 0) { ++isolated; continue; }
        ++comps; largestSize = std::max(largestSize, count[v]);
        if (count[v] >= threshold) { ++passing; if (count[v] > bestSize) { bestSize = count[v]; bestLabel = v; } }          // equal sizes: the first, the lowest label, stays
    }
    auto kept = [&](uint32_t l) { return count[l] >= threshold && (!params->keepLargestOnly || (bestSize != 0 && l == bestLabel)); };
    uint32_t nvOut = 0, nfOut = 0;
    for (uint32_t v = 0; v < nv; ++v) if (kept(parent[v])) newId[v] = nvOut++;
    for (uint32_t f = 0; f < nf; ++f) if (kept(parent[faces[3 * (size_t)f]])) ++nfOut;
    fillStats(stats, nv, nf, nvOut, nfOut, comps, params->keepLargestOnly ? (bestSize != 0 ? 1u : 0u) : passing, isolated, largestSize);
    const bool wantsV = posOut || colOut || (nrmOut && params->computeNormals);
    if ((wantsV && nvOut > vertexCapacity) || (facesOut && nfOut > faceCapacity)) { set_error("bf_mesh_clean_host: the result (%u vertices, %u faces) exceeds the capacity", nvOut, nfOut); return BF_ERR_CAPACITY; }
    if (labelsOut && nv) memcpy(labelsOut, parent.data(), 4 * (size_t)nv);
    // the output mesh, then what the caller asked for of it
    std::vector<float> P(3 * (size_t)nvOut);
    std::vector<uint32_t> F(3 * (size_t)nfOut);
    for (uint32_t v = 0; v < nv; ++v) {
        if (!kept(parent[v])) continue;
        memcpy(P.data() + 3 * (size_t)newId[v], pos + 3 * (size_t)v, 12);
        if (colOut) memcpy(colOut + 3 * (size_t)newId[v], col + 3 * (size_t)v, 12);
    }
    size_t k = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        if (!kept(parent[faces[3 * (size_t)f]])) continue;
        for (int d = 0; d < 3; ++d) F[k++] = newId[faces[3 * (size_t)f + d]];
    }
    if (posOut && nvOut) memcpy(posOut, P.data(), 12 * (size_t)nvOut);
    if (facesOut && nfOut) memcpy(facesOut, F.data(), 12 * (size_t)nfOut);
    if (nrmOut && params->computeNormals) meshnormals_host(P.data(), F.data(), nvOut, nfOut, nrmOut);
    return BF_OK;
}

// The PLY of a mesh with normals (host only): bf_write_ply_indexed's header and records with nx ny nz behind the position, as in bf_write_ply_points.
extern "C" int bf_write_ply_indexed_normals(const char* filename, const float* h_positions, const float* h_normals, const float* h_colors, const uint32_t* h_faces, uint32_t numVertices,
                                            uint32_t numFaces) {
    if (!h_normals) return bf_write_ply_indexed(filename, h_positions, h_colors, h_faces, numVertices, numFaces);
    BF_REQUIRE(filename, "null argument");
    BF_REQUIRE((numVertices == 0 || (h_positions && h_colors)) && (numFaces == 0 || h_faces), "null array");
    FILE* f = fopen(filename, "wb");
    if (!f) { set_error("cannot open %s", filename); return BF_ERR_INVALID_ARG; }
    fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment bundlefusion_amd marching cubes\nelement vertex %u\nproperty float x\nproperty float y\nproperty float z\n"
               "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
               "element face %u\nproperty list uchar int vertex_indices\nend_header\n", numVertices, numFaces);
    const size_t CH = 65536;            // records per write
    std::vector<uint8_t> buf(CH * 28);
    for (size_t base = 0; base < numVertices; base += CH) {
        const size_t m = std::min(CH, (size_t)numVertices - base);
        for (size_t j = 0; j < m; ++j) {
            const size_t i = base + j;
            uint8_t* r = buf.data() + 28 * j;
            memcpy(r, h_positions + 3 * i, 12); memcpy(r + 12, h_normals + 3 * i, 12);
            for (int k = 0; k < 3; ++k) r[24 + k] = (uint8_t)std::max(0.0f, std::min(255.0f, h_colors[3 * i + k] * 255.0f + 0.5f));
            r[27] = 255;
        }
        fwrite(buf.data(), 28, m, f);
    }
    for (size_t base = 0; base < numFaces; base += CH) {
        const size_t m = std::min(CH, (size_t)numFaces - base);
        for (size_t j = 0; j < m; ++j) {
            uint8_t* r = buf.data() + 13 * j;
            r[0] = 3;
            memcpy(r + 1, h_faces + 3 * (base + j), 12);          // int32 in the file: the same bits
        }
        fwrite(buf.data(), 13, m, f);
    }
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) { set_error("cannot write %s", filename); return BF_ERR_INVALID_ARG; }
    return BF_OK;
}
