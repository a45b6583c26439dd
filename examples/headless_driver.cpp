// Headless driver written against the reference's class names (include/bundlefusion/bundlefusion.hpp):
// the serial body of DepthSensing.cpp's OnD3D11FrameRender without DirectX.  Build:
//   g++ -std=c++17 -I include examples/headless_driver.cpp -L bundlefusion_amd/lib -lbf_hip -Wl,-rpath,$PWD/bundlefusion_amd/lib -o headless_driver
// Run:  ./headless_driver zParametersDefault.txt zParametersBundlingDefault.txt [--video DIR]
// --video DIR (or s_generateVideo = true with s_generateVideoDir): after every frame the PNG sequences of renderToFile (DepthSensing.cpp:1131-1260:
// DIR/self_reconstruction/, DIR/self_reconstruction_color/) and of renderTopDown (:1262-1390: DIR/reconstruction/, DIR/reconstruction_color/, DIR/input_color/,
// DIR/input_depth/), six-digit frame numbers.  The frustum overlay of renderTopDown is not drawn.
// With s_sensorIdx = 8 the file named by s_binaryDumpSensorFile is played (SensorDataReader, FriedLiver.cpp:89-94) and the
// optimised trajectory is evaluated against the poses stored in it; any other sensor index feeds a constant-depth dummy sensor.
#include <cstdio>
#include <limits>
#include <memory>
#include <string>
#include <sys/stat.h>

#include "bundlefusion/bundlefusion.hpp"

using namespace bundlefusion;

struct DummySensor : RGBDSensor {           // RGBDSensor contract: host float depth (metres, -inf invalid) + RGBX8 colour
    std::vector<float> depth; std::vector<unsigned char> color; unsigned int frame = 0, numFrames;
    DummySensor(unsigned int w, unsigned int h, unsigned int n) : numFrames(n) {
        std::memset(&m_desc, 0, sizeof m_desc);
        m_desc.depthWidth = m_desc.colorWidth = w; m_desc.depthHeight = m_desc.colorHeight = h;
        const mat4f I = mat4f::identity();
        mat4f K = I; K(0, 0) = K(1, 1) = 583.0f * w / 640.0f; K(0, 2) = (w - 1) / 2.0f; K(1, 2) = (h - 1) / 2.0f;
        std::memcpy(m_desc.depthIntrinsics, K.m, 64); std::memcpy(m_desc.colorIntrinsics, K.m, 64);
        std::memcpy(m_desc.depthExtrinsics, I.m, 64); std::memcpy(m_desc.colorExtrinsics, I.m, 64);
        depth.assign((size_t)w * h, 2.0f); color.assign((size_t)w * h * 4, 128);
    }
    bool processDepth() override { return frame++ < numFrames; }
    bool processColor() override { return true; }
    const float* getDepthFloat() const override { return depth.data(); }
    const unsigned char* getColorRGBX() const override { return color.data(); }
};

// the PNG sequences of s_generateVideo: renderToFile and renderTopDown restated over CUDARayCastSDF + FrameRenderer
struct VideoWriter {
    std::string base; unsigned int frameNumber = 0;
    CUDARayCastSDF rayCast; FrameRenderer target, input; DepthCameraParams cam;
    VideoWriter(const std::string& dir, const GlobalAppState& gas, const mat4f& K, const DepthCameraParams& c)
        : base(dir.empty() || dir.back() == '/' ? dir : dir + "/"), rayCast(CUDARayCastSDF::parametersFromGlobalAppState(gas, K, K.getInverse())),
          target(gas.s_rayCastWidth, gas.s_rayCastHeight), input(gas.s_integrationWidth, gas.s_integrationHeight), cam(c) {
        ::mkdir(base.c_str(), 0777);
        for (const char* sub : {"self_reconstruction/", "self_reconstruction_color/", "input_color/", "input_depth/", "reconstruction/", "reconstruction_color/"}) ::mkdir((base + sub).c_str(), 0777);
    }
    std::string name(const char* sub) const { char n[16]; std::snprintf(n, sizeof n, "%06u", frameNumber); return base + sub + n + ".png"; }
    void castAt(CUDASceneRepHashSDF& sceneRep, const mat4f& T) {
        sceneRep.setLastRigidTransformAndCompactify(T, cam);
        rayCast.render(sceneRep.getHashData(), sceneRep.getHashParams(), cam, T);
    }
    // renderToFile(context, lastRigidTransform, trackingLost)  :1131-1260
    void renderToFile(CUDASceneRepHashSDF& sceneRep, const mat4f& lastRigidTransform, bool trackingLost) {
        const GlobalRenderState& rs = GlobalRenderState::get();
        castAt(sceneRep, lastRigidTransform);
        target.render(rayCast, false, trackingLost, rs.s_renderingDepthDiscontinuityThresOffset, rs.s_renderingDepthDiscontinuityThresLin);
        target.saveToFile(name("self_reconstruction/"));
        target.render(rayCast, true, false, rs.s_renderingDepthDiscontinuityThresOffset, rs.s_renderingDepthDiscontinuityThresLin);
        target.saveToFile(name("self_reconstruction_color/"));
    }
    // renderTopDown(context, lastRigidTransform, trackingLost)  :1262-1390, without the frustum; input_color / input_depth are render modes 3 and 4 of visualizeFrame
    void renderTopDown(CUDASceneRepHashSDF& sceneRep, const float* d_depth, const unsigned char* d_color) {
        const GlobalRenderState& rs = GlobalRenderState::get();
        const GlobalAppState& gas = GlobalAppState::get();
        const float* pose = rs.s_topVideoCameraPose;
        const float a = pose[0] * 3.14159265358979323846f / 180.0f;
        mat4f T = mat4f::identity();                             // mat4f::translation(pose[1], pose[2], pose[3]) * mat4f::rotationZ(pose[0])
        T(0, 0) = std::cos(a); T(0, 1) = -std::sin(a); T(1, 0) = std::sin(a); T(1, 1) = std::cos(a); T(0, 3) = pose[1]; T(1, 3) = pose[2]; T(2, 3) = pose[3];
        rayCast.updateRayCastMinMax(rs.s_topVideoMinMax[0], rs.s_topVideoMinMax[1]);
        castAt(sceneRep, T);
        // Departure: the reference leaves the top-video range in force (its reset is commented out, DepthSensing.cpp:1291), so from the second frame on its
        // self_reconstruction pictures are cast with s_topVideoMinMax.  Here each sequence keeps its own range.
        rayCast.updateRayCastMinMax(gas.s_renderDepthMin, gas.s_renderDepthMax);
        target.render(rayCast, false, false, 0.02f, 0.01f);
        target.saveToFile(name("reconstruction/"));
        target.render(rayCast, true, false, 0.02f, 0.01f);
        target.saveToFile(name("reconstruction_color/"));
        input.RenderQuadDynamicUCHAR4(d_color);
        input.saveToFile(name("input_color/"));
        input.RenderQuadDynamicDEPTHasHSV(d_depth, gas.s_sensorDepthMin, gas.s_sensorDepthMax);
        input.saveToFile(name("input_depth/"));
    }
};

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: %s zParametersDefault.txt zParametersBundlingDefault.txt [--video DIR]\n", argv[0]); return 0; }
    try {
        GlobalAppState::get().readMembers(argv[1]);
        GlobalBundlingState::get().readMembers(argv[2]);
        GlobalRenderState::get().readMembers(argv[1]);
        std::string videoDir = GlobalRenderState::get().s_generateVideo ? GlobalRenderState::get().s_generateVideoDir : "";
        for (int i = 3; i + 1 < argc; ++i) if (std::string(argv[i]) == "--video") videoDir = argv[i + 1];
        bf_record_state rec;                                    // s_recordData / s_recordDataFile of the same file (bf_record.h)
        check(bf_record_state_read(argv[1], &rec, nullptr));
        if (rec.s_recordData && !rec.s_recordCompression) throw std::runtime_error("s_recordCompression = false (the legacy .sensor container) is not supported; record with s_recordCompression = true");
        const GlobalAppState& gas = GlobalAppState::get();
        const GlobalBundlingState& gbs = GlobalBundlingState::get();
        DummySensor dummy(640, 480, 30);
        SensorDataReader reader;
        const bool useFile = gas.s_sensorIdx == 8;
        if (useFile) reader.createFirstConnected();
        RGBDSensor& sensor = useFile ? static_cast<RGBDSensor&>(reader) : static_cast<RGBDSensor&>(dummy);
        CUDAImageManager imageManager(gas.s_integrationWidth, gas.s_integrationHeight, gbs.s_widthSIFT, gbs.s_heightSIFT, &sensor, /*storeFramesOnGPU=*/true);
        OnlineBundler bundler(&sensor, &imageManager);
        CUDASceneRepHashSDF sceneRep(CUDASceneRepHashSDF::parametersFromGlobalAppState(gas));
        DepthCameraParams cam;                                  // DepthSensing.cpp:636-643
        const mat4f K = imageManager.getDepthIntrinsics();
        cam.fx = K(0, 0); cam.fy = K(1, 1); cam.mx = K(0, 2); cam.my = K(1, 2);
        cam.m_sensorDepthWorldMin = gas.s_renderDepthMin; cam.m_sensorDepthWorldMax = gas.s_renderDepthMax;
        cam.m_imageWidth = imageManager.getIntegrationWidth(); cam.m_imageHeight = imageManager.getIntegrationHeight();
        TrajectoryManager* tm = bundler.getTrajectoryManager();
        std::unique_ptr<VideoWriter> video;
        if (!videoDir.empty()) video.reset(new VideoWriter(videoDir, gas, K, cam));
        mat4f lastRigidTransform = mat4f::identity();
        for (;;) {
            const bool bGotDepth = imageManager.process();
            if (!bGotDepth) break;
            if (rec.s_recordData) sensor.recordFrame();          // DepthSensing.cpp:1042-1045: the encode runs on the recorder's threads
            bundler.processInput();
            // reintegrate(): DepthSensing.cpp:854-902
            if (tm->getNumActiveOperations() < gas.s_maxFrameFixes) tm->generateUpdateLists();
            for (unsigned int fixes = 0; fixes < gas.s_maxFrameFixes; fixes++) {
                mat4f newT, oldT; unsigned int idx;
                if (tm->getTopFromDeIntegrateList(oldT, idx)) {
                    auto f = imageManager.getIntegrateFrame(idx);
                    sceneRep.deIntegrate(oldT, DepthCameraData(f.getDepthFrameGPU(), f.getColorFrameGPU()), cam, nullptr);
                } else if (tm->getTopFromIntegrateList(newT, idx)) {
                    auto f = imageManager.getIntegrateFrame(idx);
                    sceneRep.integrate(newT, DepthCameraData(f.getDepthFrameGPU(), f.getColorFrameGPU()), cam, nullptr);
                    tm->confirmIntegration(idx);
                } else if (tm->getTopFromReIntegrateList(oldT, newT, idx)) {
                    if (newT(0, 0) == -std::numeric_limits<float>::infinity()) continue;
                    auto f = imageManager.getIntegrateFrame(idx);
                    sceneRep.deIntegrate(oldT, DepthCameraData(f.getDepthFrameGPU(), f.getColorFrameGPU()), cam, nullptr);
                    sceneRep.integrate(newT, DepthCameraData(f.getDepthFrameGPU(), f.getColorFrameGPU()), cam, nullptr);
                    tm->confirmIntegration(idx);
                } else break;
            }
            sceneRep.garbageCollect();
            mat4f T; unsigned int frameIdx; bool bGlobalTrackingLost;
            const bool validFrame = bundler.getCurrentIntegrationFrame(T, frameIdx, bGlobalTrackingLost);
            if (validFrame) {
                auto f = imageManager.getIntegrateFrame(frameIdx);
                sceneRep.integrate(T, DepthCameraData(f.getDepthFrameGPU(), f.getColorFrameGPU()), cam, nullptr);
                tm->addFrame(TrajectoryManager::TrajectoryFrame::Integrated, T, imageManager.getCurrFrameNumber());
            } else {
                mat4f inv; for (int i = 0; i < 16; ++i) inv.m[i] = -std::numeric_limits<float>::infinity();
                tm->addFrame(TrajectoryManager::TrajectoryFrame::NotIntegrated_NoTransform, inv, imageManager.getCurrFrameNumber());
            }
            if (video && sceneRep.getNumIntegratedFrames() > 0) {             // DepthSensing.cpp:1097-1101: s_generateVideo replaces visualizeFrame
                if (validFrame) lastRigidTransform = T;
                auto f = imageManager.getIntegrateFrame(imageManager.getCurrFrameNumber());
                video->renderToFile(sceneRep, lastRigidTransform, bGlobalTrackingLost || !validFrame);
                video->renderTopDown(sceneRep, f.getDepthFrameGPU(), f.getColorFrameGPU());
                video->frameNumber++;
            }
            bundler.process(gbs.s_numLocalNonLinIterations, gbs.s_numLocalLinIterations, gbs.s_numGlobalNonLinIterations, gbs.s_numGlobalLinIterations);
            std::printf("<<< [Frame: %u ] %u >>>\n", imageManager.getCurrFrameNumber(), sceneRep.getHeapFreeCount());
        }
        if (rec.s_recordData) {                                 // DepthSensing.cpp:475-483 (StopScanningAndSaveSensorData)
            std::vector<mat4f> trajectory;
            tm->getOptimizedTransforms(trajectory);
            const std::string written = sensor.saveRecordedFramesToFile(rec.s_recordDataFile, trajectory);
            if (!written.empty()) std::printf("recorded %zu frames to %s\n", trajectory.size(), written.c_str());
        }
        if (useFile) {                                          // DepthSensing.cpp:905-910 (StopScanningAndExit): evaluate against the recorded trajectory
            std::vector<mat4f> trajectory;
            tm->getOptimizedTransforms(trajectory);
            if (!trajectory.empty()) reader.evaluateTrajectory(trajectory);      // (not part of --video: a stream too short for an optimised trajectory has nothing to evaluate, and the call rejects an empty one)
        }
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
