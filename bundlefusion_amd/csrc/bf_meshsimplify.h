// The device simplification of an indexed mesh by vertex clustering (meshsimplify.hip): the buffers a bf_marching_cubes object owns for it and the entry point
// mesh.hip calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bf_hip.h"
#include "bf_resources.h"
#include "bf_meshclean.h"

namespace bf {

struct MeshSimplify {
    // the control words and the open-addressing table (vertex numbers keyed on the cell, then face numbers keyed on the sorted cluster triple)
    uint32_t *d_words = nullptr, *d_table = nullptr;
    uint32_t capTable = 0;
    // per input vertex, grown on demand: the leader of its cluster (the cluster's lowest vertex id), on a leader the cluster's number, the cluster number of every
    // vertex, the map of the result; per scan tile of vertices its count, then its offset
    uint32_t *d_leader = nullptr, *d_cnum = nullptr, *d_cid = nullptr, *d_map = nullptr, *d_tilesV = nullptr;
    uint32_t capVerticesIn = 0;
    // per input face: its three cluster numbers, the lowest face with the same sorted triple (EMPTY: collapsed); per scan tile of faces its count / offset
    uint32_t *d_fids = nullptr, *d_faceRep = nullptr, *d_tilesF = nullptr;
    uint32_t capFacesIn = 0;
    // per cluster, allocated after the cluster count is known: n, SP[3], SC[3] as 7 int64; the leader; the representative; used by a kept face; the output id
    unsigned long long* d_acc = nullptr;
    uint32_t *d_clusterLeader = nullptr, *d_used = nullptr, *d_newId = nullptr, *d_tilesC = nullptr;
    float *d_repPos = nullptr, *d_repCol = nullptr;
    uint32_t capClusters = 0;
    // the result, valid until the next simplify: nv x 3 float (normals.d_normals: only when the last run computed them), nf x 3 uint32, numVerticesIn map entries
    float *d_positions = nullptr, *d_colors = nullptr; uint32_t* d_faces = nullptr;
    MeshNormals normals;
    uint32_t capVertices = 0, capFaces = 0;
    uint32_t numVertices = 0, numFaces = 0, numVerticesIn = 0;
    bool hasNormals = false;
};

// Simplifies the mesh at the device arrays of `in` on `stream` (see meshsimplify.hip for the definition and the kernels); waits for the stream three times (the
// refusals, the cluster count, the output counts).  The buffers of `s` are taken from, and stay with, `res`.  A refusal leaves the last result as it was.
int meshsimplify_run(MeshSimplify& s, Resources& res, hipStream_t stream, const bf_indexed_mesh& in, const bf_mesh_simplify_params& params, bf_mesh_simplify_stats* stats);

}  // namespace bf
