/*
 * bf_render.h — the reconstruction as a picture, headless: s_RenderMode 1-4 of visualizeFrame (DepthSensing.cpp:766-850) and the PNG sequences
 * of renderToFile / renderTopDown (:1131-1390) under s_generateVideo, without Direct3D.
 *
 * The reference draws the ray cast's depth image as a mesh into a four-target G-buffer (DX11RGBDRenderer, Shaders/RGBDRenderer.hlsl), shades
 * it (DX11PhongLighting, Shaders/PhongLighting.hlsl: PhongPS) and presents it with a quad (DX11QuadDrawer).  Its view matrix is the identity
 * (:785-786), so the three passes are one pass per pixel here: csrc/render.hip, defined in DESIGN.md "Frame rendering" and restated in numpy in
 * tests/render_ref.py; the two are compared as bits.  The window, the GUI and the camera controls are out of scope, and so are the
 * camera-frustum line overlay of renderTopDown, the Uplink feedback image and the text overlay.
 */
#ifndef BF_RENDER_H
#define BF_RENDER_H

#include "bf_hip.h"
#include "bf_pipeline.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the rendering keys of zParametersDefault.txt (GlobalAppState.h); bf_global_app_state keeps ignoring them */
typedef struct bf_render_state {
    float s_materialShininess;
    float s_materialAmbient[4], s_materialDiffuse[4], s_materialSpecular[4];
    float s_lightAmbient[4], s_lightDiffuse[4], s_lightSpecular[4];
    float s_lightDirection[3];
    uint32_t s_RenderMode;                 /* 1 shaded, 2 shaded ray-cast colour, 3 input colour, 4 input depth as HSV */
    float s_renderingDepthDiscontinuityThresOffset, s_renderingDepthDiscontinuityThresLin;
    int32_t s_generateVideo;
    char s_generateVideoDir[256];
    float s_topVideoTransformWorld[16];
    float s_topVideoCameraPose[4];         /* rotation (degrees about z), translation (m) */
    float s_topVideoMinMax[2];
} bf_render_state;
#define BF_RENDER_STATE_NUM_FIELDS 16

BF_API int bf_render_state_default(bf_render_state* out);                                    /* the shipped zParametersDefault.txt */
/* reads the same parameter file bf_global_app_state_read reads; *numMissing: fields of bf_render_state the file does not name */
BF_API int bf_render_state_read(const char* filename, bf_render_state* out, uint32_t* numMissing);

/* the ray cast's inverse intrinsics (CUDARayCastSDF::getIntrinsicsInv) in closed form, binary32: 1/fx, -mx/fx, 1/fy, -my/fy */
BF_API int bf_ray_cast_intrinsics_inv(const bf_ray_cast_params* params, float out[16]);

/* ---- DX11RGBDRenderer + DX11PhongLighting + DX11QuadDrawer on a width x height image ---- */
typedef struct bf_frame_renderer bf_frame_renderer;
BF_API int bf_frame_renderer_create(uint32_t width, uint32_t height, bf_frame_renderer** out);
BF_API int bf_frame_renderer_destroy(bf_frame_renderer* r);
BF_API int bf_frame_renderer_set_stream(bf_frame_renderer* r, void* hip_stream);
/* RenderDepthMap + DX11PhongLighting::render + RenderQuad in one launch.  d_depth (width * height floats, -inf = no hit) and d_colors (float4)
 * as bf_ray_cast_get_data returns them; intrinsicsInv row-major on the host.  useMaterial: PhongPS's g_useMaterial (1 shades the ray-cast
 * colour: modes 2 / "colored"); trackingLost != 0: g_overlayColor.x == -1, the grey picture.  threshOffset / threshLin are arguments because
 * renderTopDown passes 0.02 / 0.01 instead of the state's.  Every pixel of both images is written.  Asynchronous. */
BF_API int bf_frame_renderer_shade(bf_frame_renderer* r, const float* d_depth, const float* d_colors, const float intrinsicsInv[16], const bf_render_state* state,
                                   int useMaterial, int trackingLost, float threshOffset, float threshLin);
/* mode 4: depthToHSV (CameraUtil.cu:1633-1699) of a width x height depth image, then the presentation stage */
BF_API int bf_frame_renderer_depth_hsv(bf_frame_renderer* r, const float* d_depth, float minDepth, float maxDepth);
/* mode 3: a width x height RGBX8 image with alpha 255 (the float target keeps what it held) */
BF_API int bf_frame_renderer_rgbx(bf_frame_renderer* r, const uint8_t* d_rgbx);
/* device pointers: the float4 target (DX11PhongLighting::GetColorsSRV; -inf in all four channels = not drawn) and the RGBA8 image */
BF_API int bf_frame_renderer_get_images(bf_frame_renderer* r, const float** d_target, const uint8_t** d_rgba8);
BF_API int bf_frame_renderer_download_rgba8(bf_frame_renderer* r, uint8_t* h_out);          /* width * height * 4 bytes; waits for the stream */

/* LodePNG::save of a ColorImageR8G8B8A8: 8-bit RGBA, no interlace, filter 0, one IDAT with a valid zlib stream */
BF_API int bf_write_png_rgba8(const char* path, const uint8_t* rgba, uint32_t width, uint32_t height);

/* ---- the frame loop's own pictures ----
 * The pipeline creates its ray caster (s_rayCastWidth x s_rayCastHeight, s_renderDepthMin / Max) and renderer on first use.  A render is a command
 * of the volume thread's queue, executed between two frames' batches: it compactifies at the view pose, ray casts, shades and copies the picture out;
 * the caller waits for its own command only.  It does not change the reconstruction: the volume's last rigid transform and the block list a later
 * operator or garbage collection reads are what they would have been without it.
 *   mode            1 - 4 as s_RenderMode (3 / 4 show the last frame handed to the volume, 4 with s_sensorDepthMin / Max; for those two the
 *                   picture has the integration size)
 *   cameraToWorld   NULL: the pose of the last frame handed to the volume
 *   trackingLost    -1: from that frame's validity
 *   h_rgba8_out     width * height * 4 bytes.  Before the first frame reaches the volume the picture is empty (all zero), as the reference's. */
BF_API int bf_pipeline_set_render_state(bf_pipeline* p, const bf_render_state* state);
BF_API int bf_pipeline_get_render_size(bf_pipeline* p, int mode, uint32_t* width, uint32_t* height);
BF_API int bf_pipeline_render(bf_pipeline* p, int mode, const float* cameraToWorld, int trackingLost, uint8_t* h_rgba8_out);
/* renderTopDown's "reconstruction" picture: pose from s_topVideoCameraPose, depth range s_topVideoMinMax (updateRayCastMinMax; the pipeline's own
 * range is restored afterwards), thresholds 0.02 / 0.01, no overlay */
BF_API int bf_pipeline_render_top_down(bf_pipeline* p, uint8_t* h_rgba8_out);

#ifdef __cplusplus
}
#endif
#endif /* BF_RENDER_H */
