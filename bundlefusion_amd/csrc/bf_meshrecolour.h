// The device recolouring of a mesh's vertices from the key frames (meshrecolour.hip): the buffers a bf_marching_cubes object owns for it and the entry point
// mesh.hip calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bf_hip.h"
#include "bf_resources.h"

namespace bf {

struct MeshRecolour {
    // the control words; the table of the frames that are not skipped (grown on demand)
    uint32_t* d_words = nullptr;
    void* d_frames = nullptr;
    uint32_t capFrames = 0;
    // the result, valid until the next recolour: nv x 3 float colours and nv view counts.  No other pass takes either as scratch.
    float* d_colors = nullptr; uint32_t* d_views = nullptr;
    uint32_t capVertices = 0;
    // the mesh of the last recolour: the input's own arrays (not owned) and counts
    const float *d_positions = nullptr, *d_normals = nullptr; const uint32_t* d_faces = nullptr;
    uint32_t numVertices = 0, numFaces = 0;
};

// Recolours the vertices of `in` (d_normals required) from `frames` on `stream` (see meshrecolour.hip for the definition and the kernel): all frames in one launch,
// one thread per vertex; waits for the stream once (the stats).  The buffers of `r` are taken from, and stay with, `res`.  A refusal leaves the last result as it was.
int meshrecolour_run(MeshRecolour& r, Resources& res, hipStream_t stream, const bf_clean_mesh& in, const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t width, uint32_t height,
                     const float intrinsics[16], const bf_mesh_recolour_params& params, bf_mesh_recolour_stats* stats);

}  // namespace bf
