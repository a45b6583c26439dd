/*
 * bf_hip.h — C ABI of libbf_hip.so, the MI355X (gfx950) implementation of the
 * BundleFusion pose-optimisation + volumetric (re-)integration hot path.
 *
 * Every entry point replaces one method of the reference's operator surface
 * (paths relative to /root/reference/FriedLiver/Source).  Plain pointers and
 * sizes only; all `d_*` pointers are DEVICE pointers on the current HIP device,
 * all `const float m[16]` matrices are row-major 4x4 (the reference's
 * float4x4 / mat4f layout) in HOST memory.
 *
 * Conventions
 *   - every function returns BF_OK (0) or a negative bf_status; the message of
 *     the last failure on the calling thread is available via bf_last_error().
 *     (the reference throws MLIB_EXCEPTION; a C ABI cannot.)
 *   - work is enqueued on the handle's HIP stream (bf_*_set_stream; default is
 *     the NULL stream like the reference).  Functions that return a host value
 *     (counts) synchronise that stream; everything else is asynchronous.
 */
#ifndef BF_HIP_H
#define BF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BF_API __attribute__((visibility("default")))

typedef enum bf_status {
    BF_OK = 0,
    BF_ERR_INVALID_ARG = -1,
    BF_ERR_HIP = -2,           /* a HIP runtime call failed                      */
    BF_ERR_NO_DEVICE = -3,     /* no gfx950 device / extension unusable          */
    BF_ERR_CAPACITY = -4,      /* a fixed-capacity buffer overflowed             */
    BF_ERR_STATE = -5,         /* call order violated (e.g. GC before compactify) */
    BF_ERR_NOT_ON_DEVICE = -6, /* a valid input that only the host path handles (bf_jpeg_*): decode on the host instead */
    BF_ERR_INTERNAL = -7       /* a bounded device loop ran out of steps (bf_marching_cubes_clean): a bug in the library, never a hung card */
} bf_status;

BF_API const char* bf_last_error(void);
BF_API const char* bf_version(void);
/* number of visible HIP devices, <0 on error (never falls back to a CPU path) */
BF_API int bf_device_count(void);
/* Plumbing for hosts that hold raw pointers only: copies / a device-wide fence issued by this library's own HIP
 * runtime (a process may hold more than one copy of libamdhip64; work is only ordered within one of them). */
/* Restrict every thread of the calling process to the CPUs of the NUMA node HIP device `device` is attached to (intersected with the
 * caller's current affinity); threads created later inherit it.  cpulist_out (optional) receives the node's CPU list ("0-63,128-191"),
 * empty if nothing was changed (unknown topology, BF_BIND_NUMA=0).  Launch latency from the remote socket costs ~20 % of the frame rate
 * (DESIGN.md 4.4); the library never changes affinities on its own. */
BF_API int bf_bind_host_threads_to_device(int device, char* cpulist_out, size_t cpulist_len);
BF_API int bf_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
BF_API int bf_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
BF_API int bf_device_synchronize(void);
/* one stream only / a blocking copy whose direction follows from the pointers (hipMemcpyDefault): for all-gather callbacks of a host language (bf_comm.h) */
BF_API int bf_stream_synchronize(void* hip_stream);
BF_API int bf_memcpy(void* dst, const void* src, size_t bytes);
/* Diagnostics of resource ownership.  Every handle keeps what it takes from the runtime (device memory, pinned host memory, events, streams) in one owner, counted
 * process-wide: out = { live owners (== live handles that own anything), live device allocations, live device bytes, live pinned allocations + events + streams,
 * acquisitions so far, release calls that returned an error }.
 * bf_debug_fail_acquire(nth): the nth acquisition from this call on, of any handle, fails as out-of-memory without reaching the runtime (bf_last_error says that it was
 * injected); it fires once and disarms itself, 0 switches it off.  A host-side error return: the create or grow path that meets it unwinds, no kernel sees it. */
BF_API int bf_debug_live_resources(uint64_t out[6]);
BF_API int bf_debug_fail_acquire(uint64_t nth);

/* ------------------------------------------------------------------------- */
/* Voxel-hash TSDF:  DepthSensing/CUDASceneRepHashSDF.h                       */
/* ------------------------------------------------------------------------- */

#define BF_SDF_BLOCK_SIZE 8          /* VoxelUtilHashSDF.h:40 */
#define BF_HASH_BUCKET_SIZE 4        /* VoxelUtilHashSDF.h:41 */
#define BF_LOCK_ENTRY (-1)           /* VoxelUtilHashSDF.h:52 */
#define BF_FREE_ENTRY (-2)           /* VoxelUtilHashSDF.h:53 */

/* HashEntry, VoxelUtilHashSDF.h:56-74: __align__(16), 20 B payload => 32 B stride */
typedef struct __attribute__((aligned(16))) bf_hash_entry {
    int32_t pos[3];      /* SDF-block coordinate                                  */
    int32_t ptr;         /* first voxel of the block in d_SDFBlocks, or FREE_ENTRY */
    uint32_t offset;     /* collision chain link, relative to bucket's last slot  */
    uint32_t _pad[3];
} bf_hash_entry;

/* Voxel, VoxelUtilHashSDF.h:77-98: 12 B, AoS */
typedef struct bf_voxel {
    float sdf;
    float weight;
    uint8_t color[4];
} bf_voxel;

/* HashParams, DepthSensing/CUDAHashParams.h:9-39 (same fields, same order) */
typedef struct bf_hash_params {
    float m_rigidTransform[16];
    float m_rigidTransformInverse[16];
    uint32_t m_hashNumBuckets;
    uint32_t m_hashBucketSize;
    uint32_t m_hashMaxCollisionLinkedListSize;
    uint32_t m_numSDFBlocks;
    int32_t m_SDFBlockSize;
    float m_virtualVoxelSize;
    uint32_t m_numOccupiedBlocks;
    float m_maxIntegrationDistance;
    float m_truncScale;
    float m_truncation;
    uint32_t m_integrationWeightSample;
    uint32_t m_integrationWeightMax;
    float m_streamingVoxelExtents[3];
    int32_t m_streamingGridDimensions[3];
    int32_t m_streamingMinGridPos[3];
    uint32_t m_streamingInitialChunkListSize;
    uint32_t m_dummy[2];
} bf_hash_params;

/* DepthCameraParams, DepthSensing/CUDADepthCameraParams.h:7-19 */
typedef struct bf_depth_camera_params {
    float fx, fy, mx, my;
    uint32_t m_imageWidth, m_imageHeight;
    float m_sensorDepthWorldMin, m_sensorDepthWorldMax;
} bf_depth_camera_params;

/* DepthCameraData, DepthSensing/DepthCameraUtil.h:17-29: borrowed device pointers
 * at integration resolution; depth in metres with -inf = invalid, colour RGBX8. */
typedef struct bf_depth_camera_data {
    const float* d_depthData;
    const uint8_t* d_colorData; /* uchar4 per pixel, may be NULL */
} bf_depth_camera_data;

/* HashDataStruct raw pointers, VoxelUtilHashSDF.h:830-838.  d_hashBucketMutex,
 * d_hashDecisionPrefix are NULL: the gfx950 allocator is lock-free.
 * d_hashCompactified holds m_numSDFBlocks entries (it can never need more). */
typedef struct bf_hash_data {
    uint32_t* d_heap;
    uint32_t* d_heapCounter;
    int32_t* d_hashDecision;
    int32_t* d_hashDecisionPrefix;
    bf_hash_entry* d_hash;
    bf_hash_entry* d_hashCompactified;
    int32_t* d_hashCompactifiedCounter;
    bf_voxel* d_SDFBlocks;
    int32_t* d_hashBucketMutex;
} bf_hash_data;

typedef struct bf_scene bf_scene; /* == class CUDASceneRepHashSDF */

/* CUDASceneRepHashSDF(const HashParams&)            CUDASceneRepHashSDF.h:32,317 */
BF_API int bf_scene_create(const bf_hash_params* params, bf_scene** out);
/* ~CUDASceneRepHashSDF                               CUDASceneRepHashSDF.h:35    */
BF_API int bf_scene_destroy(bf_scene* s);
BF_API int bf_scene_set_stream(bf_scene* s, void* hip_stream);
/* reset()                                            CUDASceneRepHashSDF.h:147   */
BF_API int bf_scene_reset(bf_scene* s);
/* integrate(lastRigidTransform, data, params, d_bitMask)   :65-83
 * d_bitMask (streaming) must be NULL: streaming is disabled for BundleFusion
 * (zParametersDefault.txt:100) and incompatible with de-integration (:89-91). */
BF_API int bf_scene_integrate(bf_scene* s, const float cam_to_world[16],
                              const bf_depth_camera_data* data,
                              const bf_depth_camera_params* cam, const uint32_t* d_bitMask);
/* deIntegrate(...)                                         :85-108               */
BF_API int bf_scene_deintegrate(bf_scene* s, const float cam_to_world[16],
                                const bf_depth_camera_data* data,
                                const bf_depth_camera_params* cam, const uint32_t* d_bitMask);
/* Software pipelining of consecutive operators: with overlap enabled, the preparation of operators n+1 .. n+3 (allocation: the ray march and the
 * placement, which also builds the operator's block list - two launches) runs on an internal stream while the voxel update of operator n runs on the
 * scene's stream (four list buffers; the update never reads the hash table, allocation never touches voxels).  Results are unchanged.  The ORDER of
 * d_hashCompactified is unspecified (as in the reference, whose compactify appends with atomicAdd, CUDASceneRepHashSDF.cu:324-366): compare it as a
 * set.  The caller then must
 * order its input frames against the scene with bf_scene_wait_event (or have them complete) instead of relying on stream
 * order: bf_scene_wait_event makes the next operator's first kernel wait for `hip_event`.                               */
BF_API int bf_scene_set_overlap(bf_scene* s, int enable);
BF_API int bf_scene_wait_event(bf_scene* s, void* hip_event);
/* Multi-GPU hash-bucket sharding (one process per GPU): the volume owns the home buckets
 * [rank*numBuckets/world, (rank+1)*numBuckets/world) and allocates / integrates / collects only blocks hashing there.
 * Call before the first integrate; every shard is fed every frame and pose, there is no exchange between shards. */
BF_API int bf_scene_set_shard(bf_scene* s, uint32_t rank, uint32_t world);
/* Multi-GPU allocation (with bf_scene_set_shard): the ray march of the allocation (CUDASceneRepHashSDF.cu:165-251) is the part of an operator
 * that does not shrink when the volume is sharded by home bucket - every shard would march every pixel to find its own blocks.  Instead:
 *   rank r:   bf_scene_alloc_collect(part = r, parts = world)  marches a band of the pixel tiles, writes the distinct in-frustum block keys
 *   all ranks exchange the key lists (one all-gather; the lists are opaque 64-bit keys + a count)
 *   every rank: bf_scene_alloc_ingest(list) for each rank's list (ownership, table lookup, de-dup), bf_scene_alloc_place() once,
 *               then bf_scene_integrate / _reintegrate with bf_scene_set_external_alloc(1) (they skip their own allocation).
 * The resulting table is identical to the one the operator's own allocation builds (tests/test_tsdf_gpu.py).  d_slots is scratch of
 * `capacity` words; everything runs on the scene's allocation stream, bf_scene_alloc_sync waits for it. */
BF_API int bf_scene_set_external_alloc(bf_scene* s, int enable);
BF_API int bf_scene_alloc_collect(bf_scene* s, const float cam_to_world[16], const bf_depth_camera_data* data, const bf_depth_camera_params* cam,
                                  uint32_t part, uint32_t parts, uint64_t* d_keys, uint32_t* d_slots, uint32_t* d_count, uint32_t capacity);
BF_API int bf_scene_alloc_ingest(bf_scene* s, const uint64_t* d_keys, const uint32_t* d_count, uint32_t capacity);
BF_API int bf_scene_alloc_place(bf_scene* s);
BF_API int bf_scene_alloc_sync(bf_scene* s);
/* Arithmetic contract of the voxel update, CUDASceneRepHashSDF.cu:425-516 (integrateDepthMapKernel / deIntegrateDepthMapKernel):
 *   BF_TSDF_ARITH_FAST (default)   the contract of the reference's own Release GPU build (FriedLiver.vcxproj:124 <FastMath>true</FastMath>):
 *                                  approximate division (v_rcp_f32), FMA contraction.  Block set, bucket occupancy, heap and voxel
 *                                  weights are the same as in exact mode; sdf within 1e-5 x truncation, colour within 1 LSB, except
 *                                  voxels projecting within 2e-4 pixel (640x480; 6e-4 at 1280x960; measured 1.1e-4 / 4.8e-4) of a pixel
 *                                  boundary (they may sample the neighbouring pixel) - held against the oracle, tests/test_tsdf_fast_gpu.py.
 *                                  This is the path bench.py measures.
 *   BF_TSDF_ARITH_EXACT            every operation as written, IEEE binary32, no contraction - bit-comparable with a host build of the
 *                                  reference (and with oracle/): the mode of every bit-for-bit test.
 * Environment: BF_TSDF_ARITH=fast|exact selects the mode of every scene created afterwards.  May be switched at any time.
 * (Until round 3 exact was the default and the benchmark measured fast; since round 4 the library default is what is measured.) */
#define BF_TSDF_ARITH_EXACT 0
#define BF_TSDF_ARITH_FAST 1
BF_API int bf_scene_set_arith(bf_scene* s, int mode);
/* MI355X addition (fast contract): a sample's depth and colour are gathered as ONE 8-byte texel {depth f32, colour RGBX8}.  Without _set_frame_texels an
 * operator's own ray march writes the texels of its frame on the way (a de-integration, or an operator behind an external / exchanged allocation,
 * interleaves the frame in a launch of its own).  A caller that keeps its frames can interleave each frame once
 * (bf_image_interleave_texels: numPixels x 8 bytes) and hand that image to the NEXT operator on the frame with _set_frame_texels (consumed by one operator). */
BF_API int bf_scene_set_frame_texels(bf_scene* s, const void* d_texels);
BF_API int bf_image_interleave_texels(void* d_texels, const float* d_depth, const uint8_t* d_colorRGBX, uint32_t numPixels, void* hip_stream);
BF_API int bf_scene_get_arith(bf_scene* s, int* mode);
/* MI355X addition: deIntegrate(oldT) + integrate(newT) of the same frame (DepthSensing.cpp:882-889) as ONE pass over
 * the union of the two frustum lists — each touched voxel is read and written once.  Bit-identical to the two calls. */
BF_API int bf_scene_reintegrate(bf_scene* s, const float old_cam_to_world[16], const float new_cam_to_world[16],
                                const bf_depth_camera_data* data, const bf_depth_camera_params* cam);
/* garbageCollect()                                         :110-126              */
/* A batch of operators (MI355X addition).  DepthSensing.cpp:854-902 issues the up to s_maxFrameFixes re-integrations of a frame one after the other, each
 * with its own allocation, compactify and passes over the volume; bf_scene_run_batch takes them together - kind 0: integrate(T0), 1: deIntegrate(T0),
 * 2: deIntegrate(T0) + integrate(T1) of the same frame - and leaves the hash table, the heap and every voxel exactly as the same calls issued in that order
 * would (CUDASceneRepHashSDF.h:65-155), with one ray march over all frames, one placement, one union block list and ONE pass of the voxel update in which
 * every touched block is loaded once, updated by the batch's operators in order and stored once.  `wait_event` (optional hipEvent_t): the operator's frame is
 * complete when the event is; `d_texels` (optional): the frame as interleaved texels (bf_image_interleave_texels).  cam as in bf_scene_integrate. */
#define BF_SCENE_BATCH_MAX 12
#define BF_SCENE_OP_INTEGRATE 0        /* integrate(T0)                                   */
#define BF_SCENE_OP_DEINTEGRATE 1      /* deIntegrate(T0)                                 */
#define BF_SCENE_OP_REINTEGRATE 2      /* deIntegrate(T0) + integrate(T1), the same frame */
typedef struct bf_scene_batch_op {
    int32_t kind;                      /* BF_SCENE_OP_*                                   */
    int32_t reserved;
    float T0[16], T1[16];
    bf_depth_camera_data data;
    const void* d_texels;
    void* wait_event;
} bf_scene_batch_op;
BF_API int bf_scene_run_batch(bf_scene* s, const bf_scene_batch_op* ops, uint32_t n, const bf_depth_camera_params* cam);
BF_API int bf_scene_garbage_collect(bf_scene* s);
/* setLastRigidTransformAndCompactify(T)                    :136-139
 * (needs the camera of the following ray cast / GC for the frustum test)         */
BF_API int bf_scene_set_last_rigid_transform_and_compactify(
    bf_scene* s, const float cam_to_world[16], const bf_depth_camera_params* cam);
/* setLastRigidTransform(T)                                 :128-134 (host state only: m_rigidTransform and its inverse) */
BF_API int bf_scene_set_last_rigid_transform(bf_scene* s, const float cam_to_world[16]);
/* A frustum list for a view that is not the reconstruction's (the frame renderer, bf_render.h): setLastRigidTransformAndCompactify(T) + getHashData() +
 * getHashParams() into a list buffer of its own.  The scene's last rigid transform, its block list and whatever a later operator or garbage collection reads
 * stay as they are.  *hashData / *hashParams (m_rigidTransform = T, m_numOccupiedBlocks read back: the call waits for the stream) are valid until
 * bf_scene_end_view, which the caller issues after its last launch that reads them, on the scene's stream; no other scene call in between. */
BF_API int bf_scene_begin_view(bf_scene* s, const float cam_to_world[16], const bf_depth_camera_params* cam, bf_hash_data* hashData, bf_hash_params* hashParams);
BF_API int bf_scene_end_view(bf_scene* s);
/* getHashData() / getHashParams()                          :158-164
 * get_hash_params synchronises and refreshes m_numOccupiedBlocks.               */
BF_API int bf_scene_get_hash_data(bf_scene* s, bf_hash_data* out);
BF_API int bf_scene_get_hash_params(bf_scene* s, bf_hash_params* out);
/* getHeapFreeCount()                                       :168-172 (syncs)      */
BF_API int bf_scene_get_heap_free_count(bf_scene* s, uint32_t* out);
/* getNumIntegratedFrames()                                 :174                  */
BF_API int bf_scene_get_num_integrated_frames(bf_scene* s, uint32_t* out);
/* debugHash() invariants                                   :179-314 (syncs).
 * out[0]=#occupied entries out[1]=#free heap out[2]=#duplicate keys
 * out[3]=#entries whose ptr is also on the free heap out[4]=#leaked blocks
 * out[5]=#blocks dropped by the allocator so far (chain window / heap exhausted) */
BF_API int bf_scene_debug_hash(bf_scene* s, uint32_t out[6]);
/* test / tooling aid: d_ptr_out[i] = ptr of block d_pos[3 i .. 3 i + 2] (device arrays) or FREE_ENTRY, behind everything issued so far (synchronises) */
BF_API int bf_scene_debug_find_blocks(bf_scene* s, const int32_t* d_pos, uint32_t n, int32_t* d_ptr_out);
/* number of allocated SDF blocks (= occupied hash entries), syncs */
BF_API int bf_scene_get_num_allocated_blocks(bf_scene* s, uint32_t* out);
/* Opt-in HIP-event timing of the voxel-update kernel (integrateDepthMapKernel<>'s
 * replacement) on the scene's stream: enable, run ops, then read {#launches, total ms}
 * (read synchronises the stream and clears the accumulator).                       */
BF_API int bf_scene_kernel_timing(bf_scene* s, int enable);
BF_API int bf_scene_kernel_timing_read(bf_scene* s, uint32_t* count, float* total_ms);
/* over the launches timed since bf_scene_kernel_timing(s, 1) (call before _read): the sum of the frustum-list lengths
 * (m_numOccupiedBlocks) of the integrate / de-integrate operations they performed, and the number of those operations
 * (a fused re-integration launch performs two).                                                                     */
BF_API int bf_scene_kernel_timing_occupied(bf_scene* s, uint64_t* sumOccupiedBlocks, uint32_t* numOps);
/* the same plus the sum of the list lengths per LAUNCH, separately for the plain (integrate / de-integrate) and the fused
 * re-integration kernel: a fused launch visits the union of its two frustum lists once (each voxel read and written once), so its
 * algorithmic traffic is unionBlocks * (512*24 + 32) B, not 2 B                                                              */
/* frames (depth + colour images) the timed launches sampled: one per operator, n per batch of n */
BF_API int bf_scene_kernel_timing_images(bf_scene* s, uint32_t* numImages);
BF_API int bf_scene_kernel_timing_blocks(bf_scene* s, uint64_t* sumOperatorBlocks, uint64_t* visitedPlain, uint64_t* visitedFused, uint32_t* numOps);


/* ------------------------------------------------------------------------- */
/* Dense frame cache:  CUDACache.h / CUDACacheUtil.h                          */
/* ------------------------------------------------------------------------- */

/* CUDACachedFrame, CUDACacheUtil.h:10-53 (CUDACACHE_UCHAR_NORMALS and _FLOAT_NORMALS both on) */
typedef struct bf_cached_frame {
    float* d_depthDownsampled;            /* W*H                                  */
    float* d_cameraposDownsampled;        /* float4 per pixel (x,y,z,1) or -inf   */
    float* d_intensityDownsampled;        /* W*H                                  */
    float* d_intensityDerivsDownsampled;  /* float2 per pixel                     */
    uint8_t* d_normalsDownsampledUCHAR4;  /* uchar4 per pixel                     */
    float* d_normalsDownsampled;          /* float4 per pixel (nx,ny,nz,0) or -inf */
} bf_cached_frame;

typedef struct bf_cache bf_cache; /* == class CUDACache */

/* CUDACache(widthDepthInput, heightDepthInput, widthDownSampled, heightDownSampled, maxNumImages,
 *           inputIntrinsics)  CUDACache.cpp:14-43; the three filter sigmas are
 * GlobalBundlingState s_colorDownSigma / s_depthDownSigmaD / s_depthDownSigmaR.               */
BF_API int bf_cache_create(uint32_t widthDepthInput, uint32_t heightDepthInput, uint32_t widthDownSampled,
                           uint32_t heightDownSampled, uint32_t maxNumImages, const float inputIntrinsics[16],
                           float colorDownSigma, float depthDownSigmaD, float depthDownSigmaR, bf_cache** out);
BF_API int bf_cache_destroy(bf_cache* c);
BF_API int bf_cache_set_stream(bf_cache* c, void* hip_stream);
/* storeFrame(d_depth, w, h, d_color, cw, ch)                  CUDACache.cpp:45-86 */
BF_API int bf_cache_store_frame(bf_cache* c, const float* d_depth, uint32_t inputDepthWidth, uint32_t inputDepthHeight,
                                const uint8_t* d_color, uint32_t inputColorWidth, uint32_t inputColorHeight);
BF_API int bf_cache_reset(bf_cache* c);                                   /* CUDACache.h:17 */
BF_API int bf_cache_copy_cache_frame_from(bf_cache* c, bf_cache* other, uint32_t frameFrom); /* :24 */
BF_API int bf_cache_increment(bf_cache* c);                               /* incrementCache :43 */
BF_API int bf_cache_get_num_frames(bf_cache* c, uint32_t* out);
BF_API int bf_cache_set_current_frame(bf_cache* c, uint32_t n);           /* setCurrentFrame (debug) */
/* getCacheFramesGPU(): device array of maxNumImages bf_cached_frame   CUDACache.h:22 */
BF_API int bf_cache_get_frames_gpu(bf_cache* c, const bf_cached_frame** d_frames);
/* host copy of one frame's pointer struct (getCacheFrames()[i]) */
BF_API int bf_cache_get_frame(bf_cache* c, uint32_t i, bf_cached_frame* out);
/* getWidth/getHeight/getIntrinsics: out = {fx, fy, cx, cy} of the down-sampled camera */
BF_API int bf_cache_get_geometry(bf_cache* c, uint32_t* width, uint32_t* height, float intrinsics4[4]);

/* ------------------------------------------------------------------------- */
/* Bundling solver:  Solver/CUDASolverBundling.h, SBA.cu                      */
/* ------------------------------------------------------------------------- */

/* EntryJ, SiftGPU/SIFTImageManager.h:45-60 (32 B) */
typedef struct bf_entry_j {
    uint32_t imgIdx_i, imgIdx_j;   /* 0xFFFFFFFF in imgIdx_i == invalid */
    float pos_i[3];
    float pos_j[3];
} bf_entry_j;

/* thresholds CUDASolverBundling reads from GlobalBundlingState (.cpp:35-36, :93-100) */
typedef struct bf_solver_config {
    float optMaxResThresh;          /* s_optMaxResThresh              */
    float denseDistThresh;          /* s_denseDistThresh              */
    float denseNormalThresh;        /* s_denseNormalThresh            */
    float denseColorThresh;         /* s_denseColorThresh             */
    float denseColorGradientMin;    /* s_denseColorGradientMin        */
    float denseDepthMin;            /* s_denseDepthMin                */
    float denseDepthMax;            /* s_denseDepthMax                */
    uint32_t denseOverlapCheckSubsampleFactor;
    float verifyOptDistThresh;      /* 0.02 (.cpp:35)                 */
    float verifyOptPercentThresh;   /* 0.05 (.cpp:36)                 */
    int32_t recordConvergence;      /* s_recordSolverConvergence      */
} bf_solver_config;

typedef struct bf_solver bf_solver; /* == class CUDASolverBundling */

/* CUDASolverBundling(maxNumberOfImages, maxNumResiduals)      CUDASolverBundling.cpp:24 */
BF_API int bf_solver_create(uint32_t maxNumberOfImages, uint32_t maxNumResiduals, const bf_solver_config* cfg,
                            bf_solver** out);
BF_API int bf_solver_destroy(bf_solver* s);
BF_API int bf_solver_set_stream(bf_solver* s, void* hip_stream);
/* solve(...)                                                   CUDASolverBundling.cpp:187-284
 * d_rot / d_trans: float3 per image (se(3) unknowns), updated in place.  d_cacheFrames may be
 * NULL (dense term off).  weights*: numWeights host floats, one per non-linear iteration.
 * Asynchronous unless findMaxResidual/recordConvergence need host values (one sync at the end). */
BF_API int bf_solver_solve(bf_solver* s, bf_entry_j* d_correspondences, uint32_t numberOfCorrespondences,
                           const int32_t* d_validImages, uint32_t numberOfImages, uint32_t nNonLinearIterations,
                           uint32_t nLinearIterations, const bf_cached_frame* d_cacheFrames, uint32_t cacheWidth,
                           uint32_t cacheHeight, const float cacheIntrinsics4[4], const float* weightsSparse,
                           const float* weightsDenseDepth, const float* weightsDenseColor, uint32_t numWeights,
                           int usePairwiseDense, float* d_rot, float* d_trans, int rebuildJT, int findMaxResidual,
                           uint32_t revalidateIdx);
/* getVarToCorrNumEntriesPerRow(): device int[numberOfImages], #valid correspondences touching each image at the
 * last solve                                                    CUDASolverBundling.h:48 */
BF_API int bf_solver_get_var_to_corr_num_entries_per_row(bf_solver* s, const int32_t** d_out);
/* m_maxCorrPerImage (CUDASolverBundling.cpp:39): the reference invalidates correspondences beyond this many per image in atomic arrival
 * order (.cpp:195-199); this solver uses all of them.  *numImagesOverLimit = images of the last solve whose count exceeds the limit. */
BF_API int bf_solver_get_corr_overflow(bf_solver* s, uint32_t* numImagesOverLimit, uint32_t* limit);
/* getMaxResidual(max, index)                                   CUDASolverBundling.h:37-40 */
BF_API int bf_solver_get_max_residual(bf_solver* s, float* max, int32_t* index);
/* getMaxResidual(curFrame, d_corr, imageIndices, maxRes) -> remove?   .cpp:429-452 */
BF_API int bf_solver_get_max_residual_pair(bf_solver* s, uint32_t curFrame, const bf_entry_j* d_correspondences,
                                           uint32_t imageIndices[2], float* maxRes, int* remove);
/* useVerification(d_corr, n)                                   .cpp:454-476 (syncs) */
BF_API int bf_solver_use_verification(bf_solver* s, const bf_entry_j* d_correspondences, uint32_t numberOfCorrespondences,
                                      int* out);
/* getConvergenceAnalysis(): energies per GN iteration of the last solve (needs recordConvergence) */
BF_API int bf_solver_get_convergence(bf_solver* s, float* out, uint32_t capacity, uint32_t* count);
/* diagnostics of the last solve (syncs): out[0]=#GN iterations run, out[1..]=#PCG iterations of each */
BF_API int bf_solver_get_iteration_counts(bf_solver* s, int32_t* out, uint32_t capacity);
/* dump of the last dense system in the reference's layout (6N x 6N row-major JtJ, 6N Jtr);
 * test hook, syncs.  numPairs = #overlapping image pairs found.                              */
BF_API int bf_solver_debug_dense_system(bf_solver* s, float* h_JtJ, float* h_Jtr, uint32_t numImages, int32_t* numPairs);
/* dump of the last Gauss-Newton iteration's whole system in the reference's layout: A (6N x 6N row-major, sparse + dense),
 * b = -J^T F (6N) and the Jacobi preconditioner M^-1 (6N); test hook, syncs.  Image 0 is not a variable. */
BF_API int bf_solver_debug_system(bf_solver* s, float* h_A, float* h_b, float* h_prec, uint32_t numImages);
/* directed image pairs of the last solve that did not fit the solver's block capacity (min(N^2, 2C + 4N) for N > 64 images):
 * their blocks are left out of the system.  0 when everything fit.  Syncs. */
BF_API int bf_solver_get_slot_overflow(bf_solver* s, uint32_t* numSlotsDropped);

/* convertMatricesToPosesCU / convertPosesToMatricesCU          SBA.cu:75-108 (Lie space) */
BF_API int bf_convert_matrices_to_poses(const float* d_transforms, uint32_t numTransforms, float* d_rot, float* d_trans,
                                        const int32_t* d_validImages, void* hip_stream);
BF_API int bf_convert_poses_to_matrices(const float* d_rot, const float* d_trans, uint32_t numImages, float* d_transforms,
                                        const int32_t* d_validImages, void* hip_stream);

/* ------------------------------------------------------------------------- */
/* SIFT detection:  SiftGPU/SiftGPU.h (detection half of the fork)            */
/* ------------------------------------------------------------------------- */

/* SIFTKeyPoint, SiftGPU/SIFTImageManager.h:20-24 (16 B); SIFTKeyPointDesc :26-28 (128 B) */
typedef struct bf_sift_keypoint { float pos[2]; float scale; float depth; } bf_sift_keypoint;
typedef struct bf_sift_keypoint_desc { uint8_t feature[128]; } bf_sift_keypoint_desc;

typedef struct bf_sift bf_sift; /* == class SiftGPU (+ SiftPyramid) */

/* SiftGPU::SetParams(siftWidth, siftHeight, enableTiming, featureCountThreshold, siftDepthMin, siftDepthMax)
 * + InitSiftGPU  (SiftGPU.cpp:224-253; Bundler.cpp:57-62 passes threshold 150 and the sensor depth range);
 * depthWidth/Height and minKeyScale are the SiftCameraParams fields the kernels read
 * (SiftCameraParams.h, OnlineBundler.cpp:46-56).                                                      */
BF_API int bf_sift_create(uint32_t siftWidth, uint32_t siftHeight, uint32_t depthWidth, uint32_t depthHeight,
                          uint32_t featureCountThreshold, float siftDepthMin, float siftDepthMax, float minKeyScale,
                          uint32_t maxNumKeysPerImage, bf_sift** out);
BF_API int bf_sift_destroy(bf_sift* s);
BF_API int bf_sift_set_stream(bf_sift* s, void* hip_stream);
/* RunSIFT(d_intensity, d_depth) + GetKeyPointsAndDescriptorsCUDA(image, d_depth, max)  SiftGPU.cpp:72-101,267-272.
 * Asynchronous; *d_numKeys (device int) receives the feature count, or -1 for "too many keypoints".  */
BF_API int bf_sift_run(bf_sift* s, const float* d_intensity, const float* d_depth, float* d_keyPoints, uint8_t* d_descs,
                       int32_t* d_numKeys);
BF_API int bf_sift_debug_level(bf_sift* s, uint32_t octave, uint32_t index, float* h_out);
BF_API int bf_sift_debug_counts(bf_sift* s, int32_t out[26]);


/* ------------------------------------------------------------------------- */
/* Keypoint / match store, matcher, match filters:                            */
/*   SiftGPU/SIFTImageManager.h, SiftGPU/SiftMatch.h                          */
/* ------------------------------------------------------------------------- */

/* SIFTImageGPU, SIFTImageManager.h:32-36.  d_numKeyPoints is this library's addition: the key count of an
 * image stays on the device (bf_sift_run writes it) so detection -> matching needs no host read-back.
 * Keys of image i start at element i * maxKeyPointsPerImage (fixed stride instead of the reference's packed
 * prefix-sum layout); key indices in matches / correspondences are indices into that array.            */
typedef struct bf_sift_image_gpu {
    bf_sift_keypoint* d_keyPoints;
    bf_sift_keypoint_desc* d_keyPointDescs;
    int32_t* d_numKeyPoints;
} bf_sift_image_gpu;

typedef struct bf_siftmgr bf_siftmgr; /* == class SIFTImageManager (+ the SiftMatchGPU it feeds) */

/* SIFTImageManager(maxImages, maxKeyPointsPerImage)            SIFTImageManager.cpp:7-15, alloc :274-313 */
BF_API int bf_siftmgr_create(uint32_t maxImages, uint32_t maxKeyPointsPerImage, bf_siftmgr** out);
BF_API int bf_siftmgr_destroy(bf_siftmgr* m);
BF_API int bf_siftmgr_set_stream(bf_siftmgr* m, void* hip_stream);
BF_API int bf_siftmgr_reset(bf_siftmgr* m);                                      /* reset()  .h:112-124 */
/* createSIFTImageGPU / finalizeSIFTImageGPU(numKeyPoints)     .cpp:44-75.  numKeyPoints < 0: keep the count the
 * detector wrote to d_numKeyPoints.                                                                   */
BF_API int bf_siftmgr_create_image(bf_siftmgr* m, bf_sift_image_gpu* out);
BF_API int bf_siftmgr_finalize_image(bf_siftmgr* m, int32_t numKeyPoints);
BF_API int bf_siftmgr_get_image(bf_siftmgr* m, uint32_t imageIdx, bf_sift_image_gpu* out);          /* getImageGPU */
BF_API int bf_siftmgr_get_num_images(bf_siftmgr* m, uint32_t* out);
BF_API int bf_siftmgr_get_max_num_keypoints_per_image(bf_siftmgr* m, uint32_t* out);
BF_API int bf_siftmgr_get_current_frame(bf_siftmgr* m, uint32_t* out);
BF_API int bf_siftmgr_set_current_frame(bf_siftmgr* m, uint32_t idx);
/* getNumKeyPointsPerImage for images [first, first+count) — D2H + sync */
BF_API int bf_siftmgr_get_num_keypoints(bf_siftmgr* m, uint32_t first, uint32_t count, int32_t* h_out);

/* The per-pair loop of Bundler::matchAndFilter (Bundler.cpp:117-136): SiftMatchGPU::GetSiftMatch
 * (SiftMatch.cpp:160-196, ProgramCU.cu:1634-1936) of image curFrame against every image in
 * [startFrame, numFrames) \ {curFrame}, followed by SortKeyPointMatchesCU (SIFTImageManager.cu:59-143).
 * Pairs whose previous image is invalid or has no keys get 0 matches.  One launch, asynchronous.        */
BF_API int bf_siftmgr_match(bf_siftmgr* m, uint32_t curFrame, uint32_t startFrame, uint32_t numFrames, float distMax,
                            float ratioMax);
/* FilterKeyPointMatchesCU                                      SIFTImageManager.cu:186-316 */
BF_API int bf_siftmgr_filter_keypoint_matches(bf_siftmgr* m, uint32_t curFrame, uint32_t startFrame, uint32_t numFrames,
                                              const float siftIntrinsicsInv[16], uint32_t minNumMatches,
                                              float maxKabschRes2);
/* FilterMatchesBySurfaceAreaCU                                 :318-416 */
BF_API int bf_siftmgr_filter_matches_by_surface_area(bf_siftmgr* m, uint32_t curFrame, uint32_t startFrame,
                                                     uint32_t numFrames, const float colorIntrinsicsInv[16],
                                                     float areaThresh);
/* FilterMatchesByDenseVerifyCU                                 :418-608 */
BF_API int bf_siftmgr_filter_matches_by_dense_verify(bf_siftmgr* m, uint32_t curFrame, uint32_t startFrame,
                                                     uint32_t numFrames, uint32_t imageWidth, uint32_t imageHeight,
                                                     const float intrinsics[16], const bf_cached_frame* d_cachedFrames,
                                                     float distThresh, float normalThresh, float colorThresh,
                                                     float errThresh, float corrThresh, float sensorDepthMin,
                                                     float sensorDepthMax);
/* MI355X addition: the per-pair result arrays (d_currNumMatchesPerImagePair ... d_currFilteredTransformsInv, SIFTImageManager.h:262-276) exist twice.
 * _set_pair_stage selects the set (0 / 1) and the stream (null: the manager's) the pair kernels above are issued on from now on, so that the pair
 * kernels of frame k + 1 can run beside those of frame k; speculative != 0: match does not consult the valid flags of the previous images (they may
 * still be in the making on the manager's stream) and _commit_pairs - on the manager's stream, once those flags are final - clears the pairs
 * Bundler::matchAndFilter would not have matched (Bundler.cpp:126-129).  Ordering between the streams is the caller's.  The accessors of the per-pair
 * arrays name the selected set.  Default (0, null, 0): the reference's behaviour. */
BF_API int bf_siftmgr_set_pair_stage(bf_siftmgr* m, uint32_t set, void* hip_stream, int speculative);
BF_API int bf_siftmgr_commit_pairs(bf_siftmgr* m, uint32_t curFrame, uint32_t startFrame, uint32_t numFrames);
/* filterFrames                                                 SIFTImageManager.cpp:551-575 (syncs, returns the
 * last matched frame or 0xFFFFFFFF).  The _async form only enqueues the decision; it is read back together with
 * the residual count by bf_siftmgr_sync_frame_result (one D2H per frame).                              */
BF_API int bf_siftmgr_filter_frames(bf_siftmgr* m, uint32_t curFrame, uint32_t startFrame, uint32_t numFrames,
                                    uint32_t* lastMatchedFrame);
BF_API int bf_siftmgr_filter_frames_async(bf_siftmgr* m, uint32_t curFrame, uint32_t startFrame, uint32_t numFrames);
/* AddCurrToResidualsCU                                         SIFTImageManager.cu:610-690.  Skipped on the device
 * when curFrame was not connected (Bundler.cpp:218-219); pairs are appended in ascending previous-image order. */
BF_API int bf_siftmgr_add_curr_to_residuals(bf_siftmgr* m, uint32_t curFrame, uint32_t startFrame, uint32_t numFrames,
                                            const float colorIntrinsicsInv[16]);
/* MI355X addition: _filter_frames_async and _add_curr_to_residuals in ONE launch - same flags, frame result, rows and counts */
BF_API int bf_siftmgr_commit_frame(bf_siftmgr* m, uint32_t curFrame, uint32_t startFrame, uint32_t numFrames,
                                   const float colorIntrinsicsInv[16]);
BF_API int bf_siftmgr_sync_frame_result(bf_siftmgr* m, uint32_t curFrame, uint32_t* lastMatchedFrame,
                                        int32_t* numKeyPointsCur);
/* optional: enqueue that read-back now (after filter_frames_async / add_curr_to_residuals); sync_frame_result then only waits - for an
 * event behind the copy, not for the stream: up to two read-backs may be in flight, so the next frame's chain can be enqueued on the same
 * stream before the previous frame's result is consumed (results are consumed oldest first). */
BF_API int bf_siftmgr_prefetch_frame_result(bf_siftmgr* m);
/* the device record behind the read-back, for kernels that act on a frame's result without a host round trip:
 * 4 x int32 {lastMatched (-1: none), valid, numResiduals, numKeysCur}, rewritten by every filter_frames_async / add_curr_to_residuals */
BF_API int bf_siftmgr_get_frame_result_gpu(bf_siftmgr* m, const int32_t** d_frameResult);
/* InvalidateImageToImageCU / CheckForInvalidFrames[Simple]CU   :692-795 */
BF_API int bf_siftmgr_invalidate_image_to_image(bf_siftmgr* m, uint32_t imageIdx_i, uint32_t imageIdx_j);
BF_API int bf_siftmgr_check_for_invalid_frames_simple(bf_siftmgr* m, const int32_t* d_varToCorrNumEntriesPerRow,
                                                      uint32_t numVars);
BF_API int bf_siftmgr_check_for_invalid_frames(bf_siftmgr* m, const int32_t* d_varToCorrNumEntriesPerRow,
                                               uint32_t numVars);
/* VerifyTrajectoryCU                                           :1036-1159 */
BF_API int bf_siftmgr_verify_trajectory(bf_siftmgr* m, uint32_t numImages, const float* d_trajectory, uint32_t imageWidth,
                                        uint32_t imageHeight, const float intrinsics[16],
                                        const bf_cached_frame* d_cachedFrames, float distThresh, float normalThresh,
                                        float colorThresh, float errThresh, float corrThresh, float sensorDepthMin,
                                        float sensorDepthMax, int32_t* valid);
/* getValidImages / invalidateFrame / updateGPUValidImages / getValidImagesGPU   .h:157-163 */
BF_API int bf_siftmgr_get_valid_images(bf_siftmgr* m, int32_t* h_out, uint32_t count);
BF_API int bf_siftmgr_set_valid_image(bf_siftmgr* m, uint32_t frame, int32_t valid);
BF_API int bf_siftmgr_update_gpu_valid_images(bf_siftmgr* m);
BF_API int bf_siftmgr_get_valid_images_gpu(bf_siftmgr* m, const int32_t** d_out);
/* getGlobalCorrespondencesGPU / getNumGlobalCorrespondences / setGlobalCorrespondencesDEBUG   .h:182-188,251-253 */
BF_API int bf_siftmgr_get_global_correspondences_gpu(bf_siftmgr* m, bf_entry_j** d_out);
BF_API int bf_siftmgr_get_global_correspondence_keys_gpu(bf_siftmgr* m, const uint32_t** d_out /* uint2 per entry */);
BF_API int bf_siftmgr_get_num_global_correspondences(bf_siftmgr* m, uint32_t* out);
BF_API int bf_siftmgr_set_global_correspondences(bf_siftmgr* m, const bf_entry_j* h_corr, uint32_t n);
/* getFiltTransformsToWorldGPU (= d_currFilteredTransformsInv) / getNumFiltMatchesGPU   .h:254-255 */
BF_API int bf_siftmgr_get_filt_transforms_gpu(bf_siftmgr* m, const float** d_transforms, const float** d_transformsInv);
BF_API int bf_siftmgr_get_num_filt_matches_gpu(bf_siftmgr* m, const int32_t** d_out);
BF_API int bf_siftmgr_get_keys_gpu(bf_siftmgr* m, const bf_sift_keypoint** d_keys, const bf_sift_keypoint_desc** d_descs,
                                   const int32_t** d_numKeys);
#define BF_MAX_MATCHES_PER_IMAGE_PAIR_RAW 128u        /* GlobalDefines.h:8 */
#define BF_MAX_MATCHES_PER_IMAGE_PAIR_FILTERED 25u    /* GlobalDefines.h:9 */
/* getCurrMatchKeyPointIndicesDEBUG without the copy (SIFTImageManager.h:236-243): device views of the current frame's match lists -
 * uint2 key indices [maxImages][128] (raw) or [maxImages][25] (filtered) and the match count per previous image.  A key index is
 * image * maxNumKeyPointsPerImage + key (fixed stride; the reference packs the key points of all images). */
BF_API int bf_siftmgr_get_curr_matches_gpu(bf_siftmgr* m, int filtered, const uint32_t** d_keyPointIndices, const int32_t** d_numMatches);
/* get{Raw,Filt}KeyPointIndicesAndMatchDistancesDEBUG           .h:212-235 (128 / 25 slots are copied) */
BF_API int bf_siftmgr_get_raw_matches(bf_siftmgr* m, uint32_t imagePairIndex, int32_t* numMatches,
                                      uint32_t* h_keyPointIndices, float* h_distances);
BF_API int bf_siftmgr_get_filt_matches(bf_siftmgr* m, uint32_t imagePairIndex, int32_t* numMatches,
                                       uint32_t* h_keyPointIndices, float* h_distances, float* h_transform,
                                       float* h_transformInv);
/* The inverse of the two getters, for tests that hand the filters a match list of their own: the count and the 128 (raw) / 25 (filtered) slots of
 * one previous image of the selected pair set are overwritten from host memory.  Null pointers are skipped; no index is checked. */
BF_API int bf_siftmgr_set_raw_matches(bf_siftmgr* m, uint32_t imagePairIndex, int32_t numMatches,
                                      const uint32_t* h_keyPointIndices, const float* h_distances);
BF_API int bf_siftmgr_set_filt_matches(bf_siftmgr* m, uint32_t imagePairIndex, int32_t numMatches,
                                       const uint32_t* h_keyPointIndices, const float* h_distances, const float* h_transform,
                                       const float* h_transformInv);
/* addToRetryList / getTopRetryImage                            .h:263-271 */
BF_API int bf_siftmgr_add_to_retry_list(bf_siftmgr* m, uint32_t idx);
BF_API int bf_siftmgr_get_top_retry_image(bf_siftmgr* m, uint32_t* idx, int* found);
/* fuseToGlobal(global, colorIntrinsics, d_transforms, colorIntrinsicsInv)   SIFTImageManager.cpp:367-476
 * Runs on the device (track building by connected components + the reference's depth-first order per component; the new key frame
 * and its key count are written in HBM, nothing is copied to the host); asynchronous on the manager's stream.
 * bf_siftmgr_fuse_to_global_host is the reference's own form (all key points / descriptors / correspondences to the host, recursive
 * search there, upload) - same results bit for bit.
 * bf_siftmgr_fuse_error: capacity conditions of the device search since creation (none at present: always 0). */
BF_API int bf_siftmgr_fuse_to_global(bf_siftmgr* local, bf_siftmgr* global, const float colorIntrinsics[16],
                                     const float* d_transforms, const float colorIntrinsicsInv[16]);
BF_API int bf_siftmgr_fuse_to_global_host(bf_siftmgr* local, bf_siftmgr* global, const float colorIntrinsics[16],
                                          const float* d_transforms, const float colorIntrinsicsInv[16]);
BF_API int bf_siftmgr_fuse_error(bf_siftmgr* local, int* err);
/* MI355X addition: the device search keeps its graph in LDS while the keys that have a valid correspondence number at most `keys` (default, and upper
 * bound: what one workgroup's LDS holds - every chunk of 11 images fits) and in global memory beyond; 0: always in global memory (also BF_FUSE_LDS=0 in
 * the environment at creation).  Same results either way.  _fuse_path: the form the last fuse ran in, 1 LDS / 0 global memory (syncs). */
BF_API int bf_siftmgr_set_fuse_lds_limit(bf_siftmgr* local, uint32_t keys);
BF_API int bf_siftmgr_fuse_path(bf_siftmgr* local, int* path);


/* ------------------------------------------------------------------------- */
/* Frame-ingest image operators:  CUDAImageUtil.h / CUDAImageUtil.cu          */
/* (device pointers, asynchronous on hip_stream)                              */
/* ------------------------------------------------------------------------- */
/* erodeDepthMap(d_output, d_input, structureSize, w, h, dThresh, fracReq)     CUDAImageUtil.cu:701-757 */
BF_API int bf_image_erode_depth_map(float* d_output, const float* d_input, int structureSize, uint32_t width, uint32_t height,
                                    float dThresh, float fracReq, void* hip_stream);
/* gaussFilterDepthMap(d_output, d_input, sigmaD, sigmaR, w, h)                :759-809 */
BF_API int bf_image_gauss_filter_depth_map(float* d_output, const float* d_input, float sigmaD, float sigmaR, uint32_t width,
                                           uint32_t height, void* hip_stream);
/* fused forms for an ingest whose frame already lives in device memory: the first erosion carries the colour image's copies along, the depth filter writes
 * the stored frame as well (three launches instead of seven; same images bit for bit) */
BF_API int bf_image_erode_depth_map_and_copy(float* d_output, const float* d_input, int structureSize, uint32_t width, uint32_t height, float dThresh, float fracReq,
                                             const void* d_copySrc, void* d_copyDst1, void* d_copyDst2, void* stream);
BF_API int bf_image_gauss_filter_depth_map2(float* d_output, float* d_output2, const float* d_input, float sigmaD, float sigmaR, uint32_t width, uint32_t height, void* stream);
/* gaussFilterIntensity(d_output, d_input, sigmaD, w, h)                       :811-859 */
BF_API int bf_image_gauss_filter_intensity(float* d_output, const float* d_input, float sigmaD, uint32_t width, uint32_t height,
                                           void* hip_stream);
/* resampleFloat / resampleUCHAR4 / resampleToIntensity                        :93-124, :160-191, :201-258 */
BF_API int bf_image_resample_float(float* d_output, uint32_t outputWidth, uint32_t outputHeight, const float* d_input,
                                   uint32_t inputWidth, uint32_t inputHeight, void* hip_stream);
BF_API int bf_image_resample_uchar4(uint8_t* d_output, uint32_t outputWidth, uint32_t outputHeight, const uint8_t* d_input,
                                    uint32_t inputWidth, uint32_t inputHeight, void* hip_stream);
BF_API int bf_image_resample_to_intensity(float* d_output, uint32_t outputWidth, uint32_t outputHeight, const uint8_t* d_input,
                                          uint32_t inputWidth, uint32_t inputHeight, void* hip_stream);

/* ------------------------------------------------------------------------- */
/* Sensor-format ingest (csrc/sensoringest.hip): what SensorDataReader::      */
/* processDepth (SensorDataReader.cpp:98-111) does on the host, on the device */
/* (device pointers, asynchronous on hip_stream)                              */
/* ------------------------------------------------------------------------- */
/* u16 depth -> metres: 0 -> -inf, otherwise (float)raw / depthShift (a correctly rounded division: the bytes of bf_sensor_data_read_depth) */
BF_API int bf_image_convert_depth_u16(float* d_output, const uint16_t* d_input, float depthShift, uint32_t numPixels, void* hip_stream);
/* RGB8 -> RGBX8 with X = 255 (the vec4uc(vec3uc) widening; the bytes of bf_sensor_data_read_color_rgbx) */
BF_API int bf_image_convert_rgb8_to_rgbx(uint8_t* d_output, const uint8_t* d_input, uint32_t numPixels, void* hip_stream);

/* A baseline JPEG frame between its entropy decode (host: bf_jpeg_parse / bf_jpeg_entropy_decode, bf_sensordata.h) and its reconstruction
 * (host: inside bf_decode_color_rgb; device: bf_jpeg_reconstruct_device).
 * Coefficient buffer: numBlocks * 64 int16, QUANTISED, each block in natural (row-major, not zigzag) order.  Blocks are stored
 * component after component (comp[c].blockOffset), and inside a component in raster order of its block grid, which is padded to whole
 * MCUs: block (bx, by) of component c is block number comp[c].blockOffset + by * comp[c].blocksX + bx. */
typedef struct bf_jpeg_component {
    uint32_t h, v;                  /* sampling factors (1 or 2) */
    uint32_t tq;                    /* its quantisation table */
    uint32_t blocksX, blocksY;      /* block grid = mcusX * h, mcusY * v */
    uint32_t blockOffset;           /* first block of the component in the coefficient buffer */
    uint32_t planeOffset;           /* first byte of its sample plane (8 blocksX x 8 blocksY bytes) in the reconstruction's scratch */
    uint32_t reserved;
} bf_jpeg_component;
typedef struct bf_jpeg_info {
    uint32_t width, height;
    uint32_t numComponents;         /* 1 (grey) or 3 (YCbCr) */
    uint32_t hmax, vmax, mcusX, mcusY;
    uint32_t restartInterval;       /* in MCUs, 0 = none */
    uint32_t numBlocks;             /* of all components: the coefficient buffer holds numBlocks * 64 int16 */
    uint32_t planeBytes;            /* scratch of the reconstruction: the sample planes of all components */
    bf_jpeg_component comp[3];
    uint16_t qt[4][64];             /* quantisation tables, natural order (8- or 16-bit precision) */
    uint8_t qtPresent[4];
} bf_jpeg_info;
/* dequantise, islow inverse DCT, chroma up-sampling, YCbCr -> RGB, written as width*height RGBX8 with X = 255: byte for byte the image
 * bf_decode_color_rgb gives, widened.  d_planes: info->planeBytes bytes of scratch (8-byte aligned).  Layouts: 1 component; 3 components with luma at
 * hmax x vmax and each chroma component at 1x1, 2x1 or 2x2 of it.  Everything else the host decoder reads (chroma sub-sampled vertically only)
 * returns BF_ERR_NOT_ON_DEVICE and launches nothing. */
BF_API int bf_jpeg_reconstruct_device(const bf_jpeg_info* info, const int16_t* d_coefficients, uint8_t* d_planes, uint8_t* d_rgbxOut, void* hip_stream);

/* ------------------------------------------------------------------------- */
/* Recording: a frame packed for a .sens file on the device (csrc/sensorrecord.hip), the mirror image of the two conversions above */
/* ------------------------------------------------------------------------- */
/* metres -> u16, the rule of RGBDSensor::recordFrame (RGBDSensor.cpp:305): v = d * depthShift; (v > 0 && v < 65535.5) ? (uint16_t)(v + 0.5f) : 0.
 * -inf, +inf, NaN, zero and negatives give 0.  Writes exactly numPixels * 2 bytes. */
BF_API int bf_image_convert_depth_to_u16(uint16_t* d_output, const float* d_input, float depthShift, uint32_t numPixels, void* hip_stream);
/* the forward stage of the JPEG encoder (bf_jpeg_forward_host, bf_sensordata.h) on a width x height RGBX8 image (X ignored), 1 <= width, height < 65536:
 * ceil(width/8) * ceil(height/8) * 192 int16 in that function's layout, and its bytes.  d_coefficients must be 16-byte aligned, d_rgbx 4-byte. */
BF_API int bf_jpeg_forward_device(const uint8_t* d_rgbx, uint32_t width, uint32_t height, int32_t quality, int16_t* d_coefficients, void* hip_stream);

/* ------------------------------------------------------------------------- */
/* CUDAImageCalibrator:  CUDAImageCalibrator.h:1-40, .cpp:8-64                */
/* (csrc/calibrator.hip) - registers a depth image to the colour camera       */
/* ------------------------------------------------------------------------- */
/* The reference renders the depth image as a triangle mesh into the colour camera with Direct3D (DX11RGBDRenderer::RenderDepthMap,
 * Shaders/RGBDRenderer.hlsl).  Here the same stages - one quad per pixel with the shader's discontinuity test, the shader's vertex transform
 * in binary32, a top-left-rule rasteriser at 1/256 pixel - are two kernels on the caller's stream; DESIGN.md "Depth registration" is the definition,
 * with its three departures (pixel centres at integer coordinates, the value written is the depth in the COLOUR camera, triangles that cross the
 * near / far plane 0.1 m / 20 m are dropped whole).  Where several triangles cover a pixel the smallest depth wins; uncovered pixels are -inf. */
typedef struct bf_image_calibrator bf_image_calibrator;
/* OnD3D11CreateDevice(device, width, height)  .cpp:16-37.  width x height: the depth image's (and the result's) size */
BF_API int bf_image_calibrator_create(uint32_t width, uint32_t height, bf_image_calibrator** out);
/* OnD3D11DestroyDevice()  .cpp:8-14 */
BF_API int bf_image_calibrator_destroy(bf_image_calibrator* c);
BF_API int bf_image_calibrator_set_stream(bf_image_calibrator* c, void* hip_stream);
/* process(context, d_depth, colorIntrinsics, depthIntrinsicsInv, depthExtrinsics)  .cpp:39-64, minus the D3D context.  d_depth (width * height floats,
 * metres, -inf invalid) is replaced in place.  colorIntrinsics: the colour camera's at the DEPTH image's size; depthExtrinsics: depth camera -> colour
 * camera; the matrices are row-major host arrays.  threshOffset / threshLin: s_remappingDepthDiscontinuityThresOffset / ...Lin (the reference reads them
 * from GlobalAppState, :56).  Asynchronous: two launches, no host synchronisation. */
BF_API int bf_image_calibrator_process(bf_image_calibrator* c, float* d_depth, const float colorIntrinsics[16], const float depthIntrinsicsInv[16],
                                       const float depthExtrinsics[16], float threshOffset, float threshLin);

/* ------------------------------------------------------------------------- */
/* Marching cubes over the voxel hash:                                        */
/* DepthSensing/CUDAMarchingCubesHashSDF.h:8-58, .cpp, CUDAMarchingCubesSDF.cu, */
/* MarchingCubesSDFUtil.h:9-287 (a consumer of getHashData(): it reads the raw  */
/* arrays in the reference layout)                                             */
/* ------------------------------------------------------------------------- */
typedef struct bf_mc_vertex { float p[3]; float c[3]; } bf_mc_vertex;              /* MarchingCubesData::Vertex  :28-32 */
typedef struct bf_mc_triangle { bf_mc_vertex v[3]; } bf_mc_triangle;               /* MarchingCubesData::Triangle :34-39 (72 bytes) */
typedef struct bf_marching_cubes_params {                                          /* MarchingCubesParams :9-22, parametersFromGlobalAppState (.h:20-29) */
    uint32_t m_maxNumTriangles;          /* s_marchingCubesMaxNumTriangles */
    uint32_t m_sdfBlockSize, m_hashNumBuckets, m_hashBucketSize;
    float m_threshMarchingCubes;         /* s_SDFMarchingCubeThreshFactor * s_SDFVoxelSize */
    float m_threshMarchingCubes2;
} bf_marching_cubes_params;
typedef struct bf_marching_cubes bf_marching_cubes;   /* == class CUDAMarchingCubesHashSDF */

BF_API int bf_marching_cubes_create(const bf_marching_cubes_params* p, bf_marching_cubes** out);
BF_API int bf_marching_cubes_destroy(bf_marching_cubes* m);
BF_API int bf_marching_cubes_set_stream(bf_marching_cubes* m, void* hip_stream);
/* extractIsoSurface(hashData, hashParams, rayCastData, minCorner, maxCorner, boxEnabled)  .cpp:107-119; the triangles are also appended
 * to the host mesh buffer (copyTrianglesToCPU :27-46).  Triangle order is deterministic: (hash slot, voxel index, table order). */
BF_API int bf_marching_cubes_extract(bf_marching_cubes* m, const bf_hash_data* hashData, const bf_hash_params* hashParams,
                                     const float minCorner[3], const float maxCorner[3], int boxEnabled);
/* device buffer of the last extraction: *numTriangles <= m_maxNumTriangles were written, *numFound is the number the volume holds */
BF_API int bf_marching_cubes_get_triangles_gpu(bf_marching_cubes* m, const bf_mc_triangle** d_triangles, uint32_t* numTriangles, uint32_t* numFound);
BF_API int bf_marching_cubes_get_mesh(bf_marching_cubes* m, bf_mc_triangle* h_out, uint32_t capacity, uint32_t* count);   /* m_meshData */
BF_API int bf_marching_cubes_clear_mesh_buffer(bf_marching_cubes* m);                                                     /* clearMeshBuffer */
/* saveMesh(filename, transform)  .cpp:48-105: merge vertices closer than 1e-5, drop duplicate / degenerate faces, binary PLY */
BF_API int bf_marching_cubes_save_mesh(bf_marching_cubes* m, const char* filename, const float transform[16], uint32_t* numVertices, uint32_t* numFaces);
/* ---- MI355X additions: the mesh without the triangles leaving HBM (csrc/meshweld.hip) ----
 * bf_marching_cubes_create with m_maxNumTriangles == 0: every extraction sizes the triangle buffer to the volume (the count is known before anything is
 * written), so nothing is clamped; with a capacity the buffer and its clamping are the reference's. */
/* extractIsoSurface without copyTrianglesToCPU: m_meshData keeps what it held; bf_marching_cubes_get_triangles_gpu reports the result */
BF_API int bf_marching_cubes_extract_gpu(bf_marching_cubes* m, const bf_hash_data* hashData, const bf_hash_params* hashParams,
                                         const float minCorner[3], const float maxCorner[3], int boxEnabled);
/* the indexed mesh in HBM: positions and colours numVertices x 3 float, faces numFaces x 3 uint32; owned by the object, valid until its next extract, weld or destroy */
typedef struct bf_indexed_mesh { const float* d_positions; const float* d_colors; const uint32_t* d_faces; uint32_t numVertices, numFaces; } bf_indexed_mesh;
/* saveMesh's merge on the device, with exactly its result: a corner's key is (int64)floor((double)p * (1.0 / 0.00001) + 0.5) per axis; the vertex of a key is its
 * first corner in triangle order and vertex ids follow first occurrence; faces with two equal ids are dropped, of faces with the same id set the first is kept,
 * in triangle order with its winding; transform (row-major, may be NULL) is applied to the welded positions.  d_triangles NULL: the last extraction (then
 * numTriangles is ignored).  Zero triangles give an empty mesh.  Runs on the object's stream and waits for it. */
BF_API int bf_marching_cubes_weld(bf_marching_cubes* m, const bf_mc_triangle* d_triangles, uint32_t numTriangles, const float transform[16], bf_indexed_mesh* out);
/* host copies of the last weld's arrays (any of them may be NULL) */
BF_API int bf_marching_cubes_download_indexed(bf_marching_cubes* m, float* h_positions, float* h_colors, uint32_t* h_faces);
/* weld of the last extraction + download + bf_write_ply_indexed: the file bf_marching_cubes_save_mesh writes for the same triangles; m_meshData is not touched */
BF_API int bf_marching_cubes_save_mesh_gpu(bf_marching_cubes* m, const char* filename, const float transform[16], uint32_t* numVertices, uint32_t* numFaces);
/* the PLY writer of both routes (host only): binary little-endian, vertex = 3 floats + RGBA bytes ((uint8)max(0, min(255, c * 255.0f + 0.5f)), alpha 255),
 * face = count byte 3 + 3 int32 */
BF_API int bf_write_ply_indexed(const char* filename, const float* h_positions, const float* h_colors, const uint32_t* h_faces, uint32_t numVertices, uint32_t numFaces);
/* ---- MI355X additions: the indexed mesh cleaned in HBM (csrc/meshclean.hip; DESIGN.md "Mesh cleaning: the definition") ----
 * Vertices that share a face are adjacent; a component is a connected set of vertices, its label its lowest vertex id, its size its number of faces; a vertex in
 * no face is an isolated vertex (a component of size 0).  A component passes iff size >= max(1, minComponentFaces); with keepLargestOnly != 0 only the passing
 * component of greatest size stays (equal sizes: the lowest label).  The output holds the vertices of the kept components in increasing old id, positions and
 * colours copied bit for bit, and their faces in their old order and winding with the ids remapped.  computeNormals != 0: per output vertex the area-weighted
 * normal - the faces' unnormalised cross products (P[b] - P[a]) x (P[c] - P[a]) summed once per corner in increasing corner number 3f + c, binary32 op by op,
 * divided by its length sqrt((x*x + y*y) + z*z); (0, 0, 0) where the length is zero or not finite.  No result depends on the order in which threads run. */
typedef struct bf_mesh_clean_params { uint32_t minComponentFaces; int32_t keepLargestOnly; int32_t computeNormals; } bf_mesh_clean_params;
/* numComponents counts the components of size >= 1, largestComponentFaces is the greatest size among them (0 without faces) */
typedef struct bf_mesh_clean_stats {
    uint32_t numVerticesIn, numFacesIn, numVerticesOut, numFacesOut, numComponents, numComponentsKept, numIsolatedVertices, largestComponentFaces;
} bf_mesh_clean_stats;
/* the cleaned mesh in HBM: positions, colours and normals numVertices x 3 float (d_normals NULL without computeNormals), faces numFaces x 3 uint32; owned by the
 * object, valid until its next extract, weld, clean or destroy (the same struct describes the result of bf_marching_cubes_simplify) */
typedef struct bf_clean_mesh { const float* d_positions; const float* d_colors; const float* d_normals; const uint32_t* d_faces; uint32_t numVertices, numFaces; } bf_clean_mesh;
/* Cleans the indexed mesh `in` (device arrays of any origin; NULL: the last weld) on the object's stream and waits for it twice (the refusal below, then the counts).  A face id
 * >= numVertices or more than 300 000 000 faces: BF_ERR_INVALID_ARG, the last result stays as it was.  out and stats may be NULL. */
BF_API int bf_marching_cubes_clean(bf_marching_cubes* m, const bf_indexed_mesh* in, const bf_mesh_clean_params* params, bf_clean_mesh* out, bf_mesh_clean_stats* stats);
/* the component label of every INPUT vertex of the last clean (at most `capacity` of them), for tests and inspection */
BF_API int bf_marching_cubes_clean_labels(bf_marching_cubes* m, uint32_t* h_labels, uint32_t capacity);
/* host copies of the last clean's arrays (any of them may be NULL; h_normals is left alone where the clean computed none) */
BF_API int bf_marching_cubes_download_clean(bf_marching_cubes* m, float* h_positions, float* h_colors, float* h_normals, uint32_t* h_faces);
/* weld of the last extraction (with the transform, so normals are those of the transformed mesh) + clean + download + PLY: bf_write_ply_indexed_normals with
 * computeNormals, bf_write_ply_indexed without; m_meshData is not touched */
BF_API int bf_marching_cubes_save_mesh_clean(bf_marching_cubes* m, const char* filename, const float transform[16], const bf_mesh_clean_params* params, bf_mesh_clean_stats* stats);
/* The definition on one core (needs no device): host arrays in, host arrays out.  h_labelsOut: numVertices labels; the other outputs hold up to vertexCapacity
 * vertices / faceCapacity faces (BF_ERR_CAPACITY, with *stats filled in, where the result is larger; nothing but stats is written then).  Any output may be NULL. */
BF_API int bf_mesh_clean_host(const float* h_positions, const float* h_colors, const uint32_t* h_faces, uint32_t numVertices, uint32_t numFaces, const bf_mesh_clean_params* params,
                              float* h_positionsOut, float* h_colorsOut, float* h_normalsOut, uint32_t* h_facesOut, uint32_t* h_labelsOut, uint32_t vertexCapacity,
                              uint32_t faceCapacity, bf_mesh_clean_stats* stats);
/* the PLY of an indexed mesh with normals (host only): vertex = x y z nx ny nz float + RGBA bytes as in bf_write_ply_indexed (28 bytes, the field order of
 * bf_write_ply_points), the same face records; h_normals NULL: exactly bf_write_ply_indexed */
BF_API int bf_write_ply_indexed_normals(const char* filename, const float* h_positions, const float* h_normals, const float* h_colors, const uint32_t* h_faces, uint32_t numVertices,
                                        uint32_t numFaces);
/* ---- MI355X additions: the indexed mesh simplified in HBM by vertex clustering on a uniform grid (csrc/meshsimplify.hip; DESIGN.md "Mesh simplification: the
 * definition"; reference: none, the definition is the library's own) ----
 * Cell of a vertex: per axis k = (int64)floor((double)p * (1.0 / (double)cellSize)), binary64, no contraction.  A cluster is the set of ALL input vertices of one
 * cell, its leader its lowest vertex id.  With q(x) = (int64)floor((double)x * 1048576.0 + 0.5), a cluster of n members has the int64 sums SP[3], SC[3] of q over
 * its members' positions and colours; its representative is the member itself, bit for bit, where n == 1, and per component
 * (float)((double)S / ((double)n * 1048576.0)) otherwise.  Face ids are mapped to clusters; a face whose three clusters are not pairwise different is collapsed
 * and dropped; among the others, faces with the same sorted triple keep the one with the lowest face index (the duplicates go); kept faces stay in face order with
 * their winding.  Output vertices are the clusters a kept face uses, in increasing leader id; computeNormals != 0 adds the normals of bf_marching_cubes_clean's
 * definition over the output mesh.  The map holds per input vertex its output id, or 0xFFFFFFFF where its cluster is not in the output.  No result depends on the
 * order in which threads run.  Refused with BF_ERR_INVALID_ARG, the last result staying as it was: cellSize not finite or <= 0; a face id >= numVertices; a
 * position or colour component that is not finite or has |x| >= 1024; a cell index with |k| >= 2^20; more than 300 000 000 faces. */
typedef struct bf_mesh_simplify_params { float cellSize; int32_t computeNormals; } bf_mesh_simplify_params;
/* numFacesIn == numFacesOut + numFacesCollapsed + numFacesDuplicate; numVerticesOut <= numClusters <= numVerticesIn; largestCluster: the most members of one cluster */
typedef struct bf_mesh_simplify_stats {
    uint32_t numVerticesIn, numFacesIn, numClusters, numVerticesOut, numFacesOut, numFacesCollapsed, numFacesDuplicate, largestCluster;
} bf_mesh_simplify_stats;
/* Simplifies the indexed mesh `in` (device arrays of any origin; NULL: the result of the last clean, BF_ERR_INVALID_ARG if there is none) on the object's stream
 * and waits for it three times (the refusals, the cluster count, the output counts).  The result is owned by the object and valid until its next extract, weld,
 * clean, simplify or destroy; out->d_normals is NULL without computeNormals.  out and stats may be NULL.  reference: none, the definition is the library's own */
BF_API int bf_marching_cubes_simplify(bf_marching_cubes* m, const bf_indexed_mesh* in, const bf_mesh_simplify_params* params, bf_clean_mesh* out, bf_mesh_simplify_stats* stats);
/* the map of the last simplify: per INPUT vertex its output id or 0xFFFFFFFF (at most `capacity` of them).  reference: none, the definition is the library's own */
BF_API int bf_marching_cubes_simplify_map(bf_marching_cubes* m, uint32_t* h_map, uint32_t capacity);
/* host copies of the last simplify's arrays (any of them may be NULL; h_normals is left alone where it computed none).  reference: none, the definition is the
 * library's own */
BF_API int bf_marching_cubes_download_simplified(bf_marching_cubes* m, float* h_positions, float* h_colors, float* h_normals, uint32_t* h_faces);
/* weld of the last extraction (with the transform) + clean + simplify + download + PLY.  The clean's own normals are skipped: normals are computed once, on the
 * simplified mesh, if either params struct asks for them (bf_write_ply_indexed_normals then, bf_write_ply_indexed otherwise); m_meshData is not touched.  Both
 * stats may be NULL.  reference: none, the definition is the library's own */
BF_API int bf_marching_cubes_save_mesh_simplified(bf_marching_cubes* m, const char* filename, const float transform[16], const bf_mesh_clean_params* cleanParams,
                                                  const bf_mesh_simplify_params* simplifyParams, bf_mesh_clean_stats* cleanStats, bf_mesh_simplify_stats* simplifyStats);
/* The definition on one core (needs no device): host arrays in, host arrays out.  h_mapOut: numVertices entries; the other outputs hold up to vertexCapacity
 * vertices / faceCapacity faces (BF_ERR_CAPACITY, with *stats filled in, where the result is larger; nothing but stats is written then).  Any output may be NULL.
 * reference: none, the definition is the library's own */
BF_API int bf_mesh_simplify_host(const float* h_positions, const float* h_colors, const uint32_t* h_faces, uint32_t numVertices, uint32_t numFaces, const bf_mesh_simplify_params* params,
                                 float* h_positionsOut, float* h_colorsOut, float* h_normalsOut, uint32_t* h_facesOut, uint32_t* h_mapOut, uint32_t vertexCapacity,
                                 uint32_t faceCapacity, bf_mesh_simplify_stats* stats);
/* ---- MI355X additions: the mesh's vertex colours taken from the key frames in HBM (csrc/meshrecolour.hip; DESIGN.md "Mesh colour from the key frames: the
 * definition"; reference: none, the definition is the library's own) ----
 * Arithmetic: binary32, one rounding per operation, IEEE division and square root; dot(r, a, b, c, d) = ((r0*a + r1*b) + r2*c) + r3*d.  Intrinsics (4x4
 * row-major, shared by the frames): fx = K[0], fy = K[5], cx = K[2], cy = K[6].  A (vertex, frame) pair is tested by six rules in order, and the first that fails
 * names the pair's code (BF_RECOLOUR_*): NORMAL - P and N finite and (N.x*N.x + N.y*N.y) + N.z*N.z > 0; RANGE - p_j = dot(meshToCamera row j, P.x, P.y, P.z, 1),
 * z = p_2, depthMin <= z <= depthMax; IMAGE - u = (p_0 * fx) / z + cx, v = (p_1 * fy) / z + cy, 0 <= u < (float)(w - 1), 0 <= v < (float)(h - 1), x0 = (int)u,
 * y0 = (int)v, a = u - (float)x0, b = v - (float)y0, the texels (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1); FACING - c = cameraCentre - P,
 * l = sqrt((c.x*c.x + c.y*c.y) + c.z*c.z) finite and > 0, cosv = BF_RECOLOUR_NORMAL_SIGN * (((N.x*c.x + N.y*c.y) + N.z*c.z) / l) >= minCos; OCCLUDED - with
 * tol = depthTolerance + depthToleranceLin * z every one of the four depths d is finite, > 0 and has fabsf(d - z) <= tol; COLOUR - none of the four texels has
 * r == g == b == 0.  A pair that passes all six is a view (code BF_RECOLOUR_VIEW) of weight wgt = (cosv * cosv) / (z * z) and, per channel on the bytes as
 * floats, sample top = c00 + a * (c10 - c00), bot = c01 + a * (c11 - c01), val = top + b * (bot - top).  Per vertex over the frames in the order given: mode 0
 * starts from S = (+0, +0, +0), SW = +0, every view does S_c = S_c + wgt * val_c, SW = SW + wgt, and with at least one view and SW finite and > 0 the colour is
 * (S_c / SW) / 255.0f; mode 1 takes the view of greatest wgt (strictly greater replaces) and the colour is val_c / 255.0f.  A vertex without a view keeps its
 * input colour bit for bit.  Positions, normals and faces are never written.  No result depends on the order in which threads run. */
#define BF_RECOLOUR_NORMAL_SIGN (1.0f)       /* the clean's normals point to the side of the cameras that saw the surface (DESIGN.md has the finding) */
enum { BF_RECOLOUR_VIEW = 0, BF_RECOLOUR_NORMAL = 1, BF_RECOLOUR_RANGE = 2, BF_RECOLOUR_IMAGE = 3, BF_RECOLOUR_FACING = 4, BF_RECOLOUR_OCCLUDED = 5, BF_RECOLOUR_COLOUR = 6 };
typedef struct bf_mesh_recolour_params { float depthMin, depthMax, depthTolerance, depthToleranceLin, minCos; int32_t mode; } bf_mesh_recolour_params;
/* numRecoloured + numUnseen == numVertices; numFramesUsed + numFramesSkipped == the frames given; maxViews: the most views of one vertex */
typedef struct bf_mesh_recolour_stats { uint32_t numVertices, numRecoloured, numUnseen, numFramesUsed, numFramesSkipped, maxViews; } bf_mesh_recolour_stats;
/* one frame: depth (w x h float, metres) and colour (w x h RGBX8) in device memory (host memory for bf_mesh_recolour_host), mesh to camera (4x4 row-major), the
 * camera centre in mesh coordinates; skipped != 0: the frame adds nothing (and its pointers are not read) */
typedef struct bf_mesh_recolour_frame { const float* d_depth; const uint8_t* d_colorRGBX; float meshToCamera[16]; float cameraCentre[3]; int32_t skipped; } bf_mesh_recolour_frame;
/* Fills meshToCamera = inverse44(cameraToMesh) (the cofactor inverse of the kernels' bf_device.h, evaluated on the host), cameraCentre = (M[3], M[7], M[11]) and
 * skipped: 1 where M[0] is NaN or -inf (the reference's invalid pose) or any value produced is not finite, 0 otherwise.  The image pointers are left alone.
 * Host only.  reference: none, the definition is the library's own */
BF_API int bf_mesh_recolour_frame_from_pose(const float cameraToMesh[16], bf_mesh_recolour_frame* frame);
/* Recolours the mesh `in` (device arrays of any origin, normals required; NULL: the result of the last clean, or of the last simplify if that is later) from
 * `frames` on the object's stream, one thread per vertex, and waits for it once.  out: the input's pointers and counts with d_colors replaced by the object's own
 * colour array, valid until its next extract, weld, clean, simplify, recolour or destroy (no simplify takes it as scratch: a recoloured mesh is a legal input of
 * bf_marching_cubes_simplify).  Refused with BF_ERR_INVALID_ARG, nothing written and the last result staying: null normals; width or height < 2; a parameter
 * that is not finite; depthMin <= 0; depthMax < depthMin; a negative tolerance; minCos outside (0, 1]; mode not 0 or 1.  Zero frames or zero vertices give the
 * input's colours back.  out and stats may be NULL.  reference: none, the definition is the library's own */
BF_API int bf_marching_cubes_recolour(bf_marching_cubes* m, const bf_clean_mesh* in, const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t width, uint32_t height,
                                      const float intrinsics[16], const bf_mesh_recolour_params* params, bf_clean_mesh* out, bf_mesh_recolour_stats* stats);
/* the number of views of every vertex of the last recolour (at most `capacity` of them).  reference: none, the definition is the library's own */
BF_API int bf_marching_cubes_recolour_views(bf_marching_cubes* m, uint32_t* h_views, uint32_t capacity);
/* host copies of the last recolour's mesh (any of them may be NULL; h_normals and h_faces come from the input's arrays, which must still be valid).  reference:
 * none, the definition is the library's own */
BF_API int bf_marching_cubes_download_recoloured(bf_marching_cubes* m, float* h_positions, float* h_colors, float* h_normals, uint32_t* h_faces);
/* weld of the last extraction (with the transform) + clean with its normals forced on + recolour + (simplifyParams non-NULL) simplify of the recoloured mesh +
 * download + PLY.  The file carries normals (those of the mesh that is written) if either params struct asks for them.  The frames' poses are camera to MESH:
 * the caller has applied the transform to them.  Any stats may be NULL.  reference: none, the definition is the library's own */
BF_API int bf_marching_cubes_save_mesh_recoloured(bf_marching_cubes* m, const char* filename, const float transform[16], const bf_mesh_clean_params* cleanParams,
                                                  const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t width, uint32_t height, const float intrinsics[16],
                                                  const bf_mesh_recolour_params* recolourParams, const bf_mesh_simplify_params* simplifyParams, bf_mesh_clean_stats* cleanStats,
                                                  bf_mesh_recolour_stats* recolourStats, bf_mesh_simplify_stats* simplifyStats);
/* The definition on one core (needs no device): host arrays in (the frames' image pointers are host pointers), h_colorsOut numVertices x 3, h_viewsOut
 * numVertices, h_codesOut numVertices x numFrames rule codes (BF_RECOLOUR_*; a skipped frame's pairs are left alone).  Any output may be NULL.  reference: none,
 * the definition is the library's own */
BF_API int bf_mesh_recolour_host(const float* h_positions, const float* h_normals, const float* h_colors, uint32_t numVertices, const bf_mesh_recolour_frame* frames, uint32_t numFrames,
                                 uint32_t width, uint32_t height, const float intrinsics[16], const bf_mesh_recolour_params* params, float* h_colorsOut, uint32_t* h_viewsOut,
                                 uint8_t* h_codesOut, bf_mesh_recolour_stats* stats);
/* ---- MI355X additions: a texture atlas for the mesh taken from the key frames in HBM (csrc/meshtexture.hip; DESIGN.md "Mesh texture: the definition"; reference:
 * none, the definition is the library's own) ----
 * Arithmetic as the recolouring's.  (1) Face choice, per face (a, b, c): e1 = P_b - P_a, e2 = P_c - P_a, n = e1 x e2 (n.x = e1.y*e2.z - e1.z*e2.y, ...),
 * len = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z), N = n / len per component; the face is degenerate if an index is >= numVertices, a position is not finite or len
 * is not finite or not > 0.  A frame that is not skipped views the face iff rules RANGE .. COLOUR of the recolouring give BF_RECOLOUR_VIEW for all three corners
 * with N in place of the vertex normal; its weight is fminf(fminf(wgt_a, wgt_b), wgt_c).  Over the frames in the order given the first viewing frame is taken
 * and a later one replaces it iff its weight is strictly greater.  faceFrame[f]: the index into `frames` (skipped ones counted), -1 for a degenerate or unviewed
 * face.  (2) Layout, integers: S = patchSize in 4 .. 64, m = S - 3, A = atlasWidth in S .. 16384, cellsPerRow = A / S; face f lives in cell q = f >> 1, half
 * t = f & 1, the cell's origin is (X, Y) = ((q % cellsPerRow) * S, (q / cellsPerRow) * S), H = S * ceil(ceil(numFaces / 2) / cellsPerRow) (H > 32768:
 * BF_ERR_CAPACITY; no faces: H = 0).  Texel (i, j) of a cell belongs to half 0 iff i + j <= S - 1.  Corner texels: half 0 a = (0, 0), b = (m, 0), c = (0, m);
 * half 1 a = (S-1, S-1), b = (S-1-m, S-1), c = (S-1, S-1-m).  A corner texel (ci, cj) has u = ((float)(X + ci) + 0.5f) / (float)A,
 * v = 1.0f - ((float)(Y + cj) + 0.5f) / (float)H; faceUV[f] = u_a v_a u_b v_b u_c v_c.  Atlas row 0 is Y = 0.  (3) Fill, per texel: right of cellsPerRow * S
 * or with a face index >= numFaces it is unused, RGBA 0 0 0 0.  Otherwise s = (float)i / (float)m, r = (float)j / (float)m (half 1: S-1-i and S-1-j), wb = s,
 * wc = r, wa = (1.0f - s) - r (gutter texels extrapolate), P = (wa*P_a + wb*P_b) + wc*P_c per component, and with k = faceFrame[f] >= 0: p_j and z as rule RANGE
 * computes them, z finite and > 0, u, v, x0, y0, a, b and the four texels by rule IMAGE, none of the four colour texels black, val_c the bilinear sample; there
 * is NO depth test per texel.  With k < 0 or any of these failing: val_c = ((wa*C_a + wb*C_b) + wc*C_c) * 255.0f from the vertex colours; a face with an index
 * out of range gives 0 0 0.  Byte (uint8_t)(int)(fminf(fmaxf(val_c, 0.0f), 255.0f) + 0.5f), alpha 255.  No result depends on the order in which threads run. */
typedef struct bf_mesh_texture_params { float depthMin, depthMax, depthTolerance, depthToleranceLin, minCos; uint32_t patchSize, atlasWidth; } bf_mesh_texture_params;
/* numFacesTextured + numFacesUntextured == numFaces; numFramesUsed + numFramesSkipped == the frames given; the three texel counts sum to atlasWidth * atlasHeight */
typedef struct bf_mesh_texture_stats { uint32_t numFaces, numFacesTextured, numFacesUntextured, numFramesUsed, numFramesSkipped, atlasWidth, atlasHeight;
                                       uint64_t numTexelsFromFrames, numTexelsFromVertices, numTexelsUnused; } bf_mesh_texture_stats;
/* Textures the mesh `in` (device arrays of any origin, normals not needed; NULL: the result of the last clean, or of the last simplify if that is later) from
 * `frames` (bf_mesh_recolour_frame, filled by bf_mesh_recolour_frame_from_pose) on the object's stream - the face choice with one thread per face, the fill with
 * one thread per texel - and waits for it once.  The atlas (atlasWidth x atlasHeight RGBA8), the per-face frame index and the per-face texture coordinates stay
 * on the device with the object, valid until its next extract, weld, clean, simplify, texture or destroy.  Refused with BF_ERR_INVALID_ARG, nothing written and
 * the last result staying: the recolouring's list without the normals and the mode; patchSize or atlasWidth out of range.  Zero frames, or all of them skipped:
 * every face falls back, the atlas is the interpolated vertex colours.  stats may be NULL.  reference: none, the definition is the library's own */
BF_API int bf_marching_cubes_texture(bf_marching_cubes* m, const bf_clean_mesh* in, const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t width, uint32_t height,
                                     const float intrinsics[16], const bf_mesh_texture_params* params, bf_mesh_texture_stats* stats);
/* host copies of the last texture: atlasWidth * atlasHeight * 4 bytes, numFaces int32, numFaces * 6 floats (any of them may be NULL).  reference: none, the
 * definition is the library's own */
BF_API int bf_marching_cubes_download_texture(bf_marching_cubes* m, uint8_t* h_atlasRGBA, int32_t* h_faceFrame, float* h_faceUV);
/* weld of the last extraction (with the transform) + clean + (recolourParams non-NULL) recolour + (simplifyParams non-NULL) simplify + texture + download + the
 * two files: bf_write_ply_textured to `filename` and the atlas as a PNG next to it, under the same name with its extension replaced by ".png" (the PLY's comment
 * carries that name without its directory; the extension is what follows the last dot of the base name, a dot that begins the base name is not one: "a/.scan"
 * gives "a/.scan.png", and a name without a dot gets ".png" appended).  The vertices keep their colours beside the texture.  A mesh without faces has no atlas: the PLY alone is written.
 * The file carries normals if either params struct asks for them.  The frames' poses are camera to MESH: the caller has applied the transform to them.  Any
 * stats may be NULL.  reference: none, the definition is the library's own */
BF_API int bf_marching_cubes_save_mesh_textured(bf_marching_cubes* m, const char* filename, const float transform[16], const bf_mesh_clean_params* cleanParams,
                                                const bf_mesh_recolour_frame* frames, uint32_t numFrames, uint32_t width, uint32_t height, const float intrinsics[16],
                                                const bf_mesh_texture_params* textureParams, const bf_mesh_recolour_params* recolourParams, const bf_mesh_simplify_params* simplifyParams,
                                                bf_mesh_clean_stats* cleanStats, bf_mesh_recolour_stats* recolourStats, bf_mesh_simplify_stats* simplifyStats,
                                                bf_mesh_texture_stats* textureStats);
/* the atlas height H of the layout for numFaces faces (BF_ERR_CAPACITY where H > 32768), for sizing the outputs of bf_mesh_texture_host.  Host only.  reference:
 * none, the definition is the library's own */
BF_API int bf_mesh_texture_atlas_height(uint32_t numFaces, const bf_mesh_texture_params* params, uint32_t* atlasHeight);
/* The definition on one core (needs no device): host arrays in (the frames' image pointers are host pointers), h_atlasRGBA atlasWidth * H * 4 bytes,
 * h_faceFrame numFaces, h_faceUV numFaces x 6.  Any output may be NULL.  reference: none, the definition is the library's own */
BF_API int bf_mesh_texture_host(const float* h_positions, const float* h_colors, const uint32_t* h_faces, uint32_t numVertices, uint32_t numFaces, const bf_mesh_recolour_frame* frames,
                                uint32_t numFrames, uint32_t width, uint32_t height, const float intrinsics[16], const bf_mesh_texture_params* params, uint8_t* h_atlasRGBA,
                                int32_t* h_faceFrame, float* h_faceUV, bf_mesh_texture_stats* stats);
/* the PLY of a textured mesh (host only): the header of bf_write_ply_indexed_normals (h_normals NULL: of bf_write_ply_indexed) with "comment TextureFile
 * <textureFileName>" behind its comment line and "property list uchar float texcoord" behind vertex_indices; the vertex records are those writers', a face record
 * is theirs followed by the byte 6 and the six floats u_a v_a u_b v_b u_c v_c (38 bytes).  reference: none, the definition is the library's own */
BF_API int bf_write_ply_textured(const char* filename, const char* textureFileName, const float* h_positions, const float* h_normals, const float* h_colors, const uint32_t* h_faces,
                                 const float* h_faceUV, uint32_t numVertices, uint32_t numFaces);
/* ---- MI355X additions: the distance of a mesh to a reference surface in HBM (csrc/meshdistance.hip; DESIGN.md "Mesh distance: the definition"; reference: none,
 * the definition is the library's own) ----
 * Mesh A (the samples) is measured against mesh B (the surface); both are indexed meshes, positions n x 3 binary32, faces m x 3 uint32, colours not read.  All
 * arithmetic is binary64 from the binary32 inputs, one rounding per operation, no contraction, IEEE division and square root; dot(x, y) = (x0*y0 + x1*y1) + x2*y2.
 * Degenerate: with u = b - a, v = c - a, n = (u1*v2 - u2*v1, u2*v0 - u0*v2, u0*v1 - u1*v0) and N2 = dot(n, n), a face is degenerate iff not (0 < N2 < inf) (so is
 * every face with a corner that is not finite).  A degenerate face of B is never a candidate, one of A gives no samples; both are counted.
 * Samples: sampleMode 0 - the vertices of A in vertex order, weight 1, those no face uses included.  sampleMode 1 - per non-degenerate face in face order, with
 * L = sqrt(max(dot(b-a, b-a), dot(c-a, c-a), dot(c-b, c-b))) and n = max(1, ceil(L / (double)sampleSpacing)) (sampleSpacing == 0: n = 1), the n*n centroids of
 * its congruent sub-triangles: sample k = 0 .. n*n - 1 lies in row j = n - r, r the least integer with r*r >= n*n - k, at t = k - (n*n - r*r) in the row, i = t / 2;
 * t even (upright): u = (3i + 1) / (3n), v = (3j + 1) / (3n); t odd (inverted): u = (3i + 2) / (3n), v = (3j + 2) / (3n), the numerators and 3n exact in binary64;
 * p = (a + u * (b - a)) + v * (c - a) per component, in binary64 (the sample is not rounded to binary32); weight (0.5 * sqrt(N2)) / (double)(n*n).  Sample ids: the
 * prefix sum of the faces' n*n.
 * Distance: d2(p, f) = dot(p - q, p - q), q the closest point of Ericson, Real-Time Collision Detection 5.1.5, with ab = b-a, ac = c-a, ap = p-a, bp = p-b,
 * cp = p-c, d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp), vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6,
 * va = d3*d6 - d5*d4, the first rule that holds: d1 <= 0 and d2 <= 0: q = a; d3 >= 0 and d4 <= d3: q = b; vc <= 0, d1 >= 0, d3 <= 0: q = a + (d1 / (d1 - d3)) * ab;
 * d6 >= 0 and d5 <= d6: q = c; vb <= 0, d2 >= 0, d6 <= 0: q = a + (d2 / (d2 - d6)) * ac; va <= 0, d4 - d3 >= 0, d5 - d6 >= 0: q = b + ((d4 - d3) / ((d4 - d3) +
 * (d5 - d6))) * (c - b); otherwise den = 1 / ((va + vb) + vc), q = (a + ab * (vb * den)) + ac * (vc * den).  A sample's result is the minimum of d2 over the
 * non-degenerate faces of B, the lowest face index among equal d2.  With D = (double)maxDistance: minimum > D * D (or no face): beyond, distance +inf, face
 * 0xFFFFFFFF; otherwise within, distance sqrt(minimum).
 * Sums: q(x, k) = (int64)floor(x * 2^k + 0.5).  With L the least integer with numSamples <= 2^L, E = 0 (sampleMode 0) or 6 (sampleMode 1) and e the least integer
 * in [-20, 6] with D <= 2^e: scaleW = 62 - L - E, scaleWD = scaleW - e, scaleWD2 = scaleW - 2e.  Over the within-samples sumW = sum q(w, scaleW), sumWD =
 * sum q(w * d, scaleWD), sumWD2 = sum q((w * d) * d, scaleWD2), histogram[min(1023, floor(d * (1024.0 / D)))] += q(w, scaleW); over the beyond-samples
 * sumWBeyond = sum q(w, scaleW).  maxWithin is the greatest within-distance (0 without one).  No sum passes 2^62 + numSamples; no result depends on the order in
 * which threads run or on the search structure.
 * Refused with BF_ERR_INVALID_ARG, nothing written and the last result staying: maxDistance not finite, <= 0 or > 64; sampleSpacing negative or not finite;
 * sampleMode not 0 or 1; a face id >= numVertices in either mesh; a finite component with |x| >= 1024 at a corner of any face of either mesh; in
 * sampleMode 0 a component of a vertex of A that is not finite or has |x| >= 1024; a face of A with n > 1024 or a sample weight >= 64 (lower sampleSpacing);
 * more than 2^28 samples; more than 300 000 000 faces in either mesh.  (A corner that is not finite makes its face degenerate: skipped and counted, not refused.)
 * An empty A gives zero samples; an empty or all-degenerate B puts every sample beyond.  BF_ERR_CAPACITY, the last result staying: the search grid over B (cell
 * edge max(D, 2^-9) * (1 + 2^-10); a face is listed in every cell of its bounding box that its plane may cross, a sliver with sin^2 of its angle at a below 2^-20 in
 * every cell of its box) would hold more than 2^27 (face, cell) pairs. */
typedef struct bf_mesh_distance_params { float maxDistance; float sampleSpacing; int32_t sampleMode; } bf_mesh_distance_params;
/* a sum S with scale k stands for S / 2^k: mean = (sumWD / 2^scaleWD) / (sumW / 2^scaleW), rms^2 = (sumWD2 / 2^scaleWD2) / (sumW / 2^scaleW) */
typedef struct bf_mesh_distance_stats {
    uint64_t numSamples, numWithin, numBeyond;
    uint32_t numDegenerateA, numDegenerateB;
    double maxWithin;
    int64_t sumW, sumWD, sumWD2, sumWBeyond;
    int32_t scaleW, scaleWD, scaleWD2, reserved;
    int64_t histogram[1024];
} bf_mesh_distance_stats;
/* Measures mesh `a` against mesh `b` (device arrays of any origin, d_colors not read) on the object's stream and waits for it twice (the refusals and counts,
 * then the sums).  a NULL: the result of the object's last simplify, else of its last clean, else of its last weld - the latest of the three stages that has run, so a
 * mesh of an earlier extraction is never taken behind a newer weld (BF_ERR_INVALID_ARG if none has).  The
 * per-sample result stays on the device with the object until its next measurement or destroy.  stats may be NULL.  reference: none, the definition is the
 * library's own */
BF_API int bf_marching_cubes_distance(bf_marching_cubes* m, const bf_indexed_mesh* a, const bf_indexed_mesh* b, const bf_mesh_distance_params* params, bf_mesh_distance_stats* stats);
/* host copies of the last measurement's per-sample arrays, at most `capacity` samples of each (any of them may be NULL).  reference: none, the definition is
 * the library's own */
BF_API int bf_marching_cubes_download_distance(bf_marching_cubes* m, double* h_distance, uint32_t* h_face, double* h_weight, uint32_t capacity);
/* weld of the last extraction (with the transform) + clean (its normals skipped) + (simplifyParams non-NULL) simplify + the upload of the reference mesh (host
 * arrays, kept on the device with the object) + the measurement: direction 0 measures the scan against the reference (accuracy), direction 1 the reference against
 * the scan (completeness).  The per-sample result is bf_marching_cubes_download_distance's; m_meshData is not touched.  Any stats may be NULL.  reference: none,
 * the definition is the library's own */
BF_API int bf_marching_cubes_measure_mesh(bf_marching_cubes* m, const float transform[16], const bf_mesh_clean_params* cleanParams, const bf_mesh_simplify_params* simplifyParams,
                                          const float* h_refPositions, const uint32_t* h_refFaces, uint32_t numVertices, uint32_t numFaces, const bf_mesh_distance_params* distanceParams,
                                          int32_t direction, bf_mesh_clean_stats* cleanStats, bf_mesh_simplify_stats* simplifyStats, bf_mesh_distance_stats* distanceStats);
/* The number of samples the definition takes from mesh A (host arrays; with every refusal that concerns A alone).  Host only.  reference: none, the definition
 * is the library's own */
BF_API int bf_mesh_distance_sample_count_host(const float* h_positionsA, const uint32_t* h_facesA, uint32_t numVerticesA, uint32_t numFacesA, const bf_mesh_distance_params* params,
                                              uint64_t* numSamples);
/* The definition on one core (needs no device): host arrays in, host arrays out, the same closest-point function as the kernels, over a grid of its own whose
 * cells follow the faces' size and are searched ring by ring.  The first min(capacity, numSamples) samples are written; any output may be NULL.  reference:
 * none, the definition is the library's own */
BF_API int bf_mesh_distance_host(const float* h_positionsA, const uint32_t* h_facesA, uint32_t numVerticesA, uint32_t numFacesA, const float* h_positionsB, const uint32_t* h_facesB,
                                 uint32_t numVerticesB, uint32_t numFacesB, const bf_mesh_distance_params* params, double* h_distance, uint32_t* h_face, double* h_weight,
                                 uint32_t capacity, bf_mesh_distance_stats* stats);
/* bf_write_ply_indexed with the vertex-mode distance as the colours (host only).  t = (float)(d / (double)maxDistance); a vertex with d <= maxDistance gets
 * (max(0, 2t - 1), 1 - |2t - 1|, max(0, 1 - 2t)) in binary32 - blue at 0 through green to red at maxDistance -, any other (beyond, NaN) gets (1, 0, 1).
 * reference: none, the definition is the library's own */
BF_API int bf_write_ply_indexed_error(const char* filename, const float* h_positions, const uint32_t* h_faces, const double* h_distance, float maxDistance, uint32_t numVertices,
                                      uint32_t numFaces);
/* the generated case tables (edge mask per case, up to 5 triangles of edge indices, -1 terminated), for inspection / tests */
BF_API int bf_marching_cubes_tables(uint16_t edgeTable[256], int8_t triTable[256 * 16]);

/* ------------------------------------------------------------------------- */
/* Ray cast of the volume: class CUDARayCastSDF (DepthSensing/CUDARayCastSDF.h:14-101, .cpp, .cu),        */
/* RayCastSDFUtil.h, DX11RayIntervalSplatting (the rasterised interval splat is a compute pass here)      */
/* ------------------------------------------------------------------------- */
typedef struct bf_ray_cast_params {        /* struct RayCastParams, CUDARayCastParams.h:7-27 (same field order) */
    float m_viewMatrix[16];
    float m_viewMatrixInverse[16];
    float mx, my, fx, fy;                  /* ray cast intrinsics */
    uint32_t m_width, m_height;
    uint32_t m_numOccupiedSDFBlocks;
    uint32_t m_maxNumVertices;             /* kept for the capacity check of rayIntervalSplatting (6 vertices per block) */
    int32_t m_splatMinimum;                /* unused: both intervals are splatted in one pass */
    float m_minDepth, m_maxDepth;
    float m_rayIncrement, m_thresSampleDist, m_thresDist;
    int32_t m_useGradients;
    uint32_t dummy0;
} bf_ray_cast_params;

typedef struct bf_ray_cast_data {          /* struct RayCastData, RayCastSDFUtil.h:33-303: device images of m_width x m_height */
    float* d_depth;                        /* depth along the camera z axis, -inf where no surface was hit */
    float* d_depth4;                       /* float4 camera-space point (x, y, z, 1) or -inf */
    float* d_normals;                      /* float4 camera-space normal (w = 1) or -inf */
    float* d_colors;                       /* float4 rgb in [0,1] (w = 1) or -inf */
    float* d_rayIntervalSplatMin;          /* per-pixel entry / exit depth of the allocated blocks (the two D3D11 render targets), -inf = no block */
    float* d_rayIntervalSplatMax;
} bf_ray_cast_data;

typedef struct bf_ray_cast bf_ray_cast;    /* == class CUDARayCastSDF */
BF_API int bf_ray_cast_create(const bf_ray_cast_params* params, bf_ray_cast** out);          /* CUDARayCastSDF(params) */
BF_API int bf_ray_cast_destroy(bf_ray_cast* rc);
BF_API int bf_ray_cast_set_stream(bf_ray_cast* rc, void* hip_stream);
/* render(hashData, hashParams, lastRigidTransform)  .cpp:42-72: hashData / hashParams as bf_scene_get_hash_data / _get_hash_params
 * return them after an integrate or setLastRigidTransformAndCompactify (frustum list + m_numOccupiedBlocks + m_rigidTransformInverse);
 * depthCamera = the DepthCameraParams the volume was compactified with (c_depthCameraParams of the splat's frustum test).  */
BF_API int bf_ray_cast_render(bf_ray_cast* rc, const bf_hash_data* hashData, const bf_hash_params* hashParams,
                              const bf_depth_camera_params* depthCamera, const float lastRigidTransform[16]);
BF_API int bf_ray_cast_get_data(bf_ray_cast* rc, bf_ray_cast_data* out);                      /* getRayCastData */
BF_API int bf_ray_cast_get_params(bf_ray_cast* rc, bf_ray_cast_params* out);                  /* getRayCastParams */
BF_API int bf_ray_cast_update_min_max(bf_ray_cast* rc, float depthMin, float depthMax);       /* updateRayCastMinMax */
BF_API int bf_ray_cast_set_intrinsics(bf_ray_cast* rc, uint32_t width, uint32_t height, const float intrinsics[16]);   /* setRayCastIntrinsics */
BF_API int bf_ray_cast_convert_to_camera_space(bf_ray_cast* rc, const bf_depth_camera_params* depthCamera);            /* convertToCameraSpace */

#ifdef __cplusplus
}
#endif
#endif /* BF_HIP_H */
