// The device texture atlas of a mesh from the key frames (meshtexture.hip): the buffers a bf_marching_cubes object owns for it and the entry point mesh.hip calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bf_hip.h"
#include "bf_resources.h"

namespace bf {

struct MeshTexture {
    // the control words (uint64); the table of ALL the frames given, skipped ones included, so that a face's frame index is the caller's (grown on demand)
    unsigned long long* d_words = nullptr;
    void* d_frames = nullptr;
    uint32_t capFrames = 0;
    // the result, valid until the next texture: per face its frame (-1: none) and six texture coordinates, the atlas as RGBA8 texels, row 0 first
    int32_t* d_faceFrame = nullptr; float* d_faceUV = nullptr;
    uint32_t capFaces = 0;
    uint32_t* d_atlas = nullptr;
    size_t capTexels = 0;
    uint32_t numFaces = 0, atlasWidth = 0, atlasHeight = 0;
};

// Textures the faces of `in` from `frames` on `stream` (see meshtexture.hip for the definition and the kernels): the face choice, one thread per face over all
// frames, then the atlas fill, one thread per texel; waits for the stream once (the stats).  The buffers of `t` are taken from, and stay with, `res`.  A refusal
// leaves the last result as it was.
int meshtexture_run(MeshTexture& t, Resources& res, hipStream_t stream, const bf_clean_mesh& in, const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t width, uint32_t height,
                    const float intrinsics[16], const bf_mesh_texture_params& params, bf_mesh_texture_stats* stats);

}  // namespace bf
