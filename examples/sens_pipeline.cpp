// Plays a recorded ".sens" file through the whole-loop C entry points (bf_pipeline_*: four streams, volume worker thread,
// one-frame detection look-ahead) and evaluates the optimised trajectory against the poses stored in the file.
// Build:  g++ -std=c++17 -I include examples/sens_pipeline.cpp -L bundlefusion_amd/lib -lbf_hip -Wl,-rpath,$PWD/bundlefusion_amd/lib -o sens_pipeline
// Run:    ./sens_pipeline sequence.sens [--ingest host|device] [--decode-threads N] [zParametersDefault.txt zParametersBundlingDefault.txt] [scan.ply]
//   --ingest host    (default) frames are decoded to float depth / RGBX on this thread (SensorDataReader) and handed over as host buffers
//   --ingest device  SensPlayer: N threads (default 4, at most 12) decode ahead; depth conversion and JPEG reconstruction run on the device.  Same results.
//   scan.ply         (a trailing argument ending in .ply) the scan's mesh after the end of the sequence: bf_pipeline_save_mesh
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bundlefusion/bundlefusion.hpp"

using namespace bundlefusion;

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s sequence.sens [--ingest host|device] [--decode-threads N] [--record out.sens] [zParametersDefault.txt zParametersBundlingDefault.txt] [scan.ply]\n", argv[0]); return 0; }
    try {
        bool deviceIngest = false;
        unsigned int decodeThreads = 4;
        const char* recordPath = nullptr;
        std::vector<const char*> files;
        for (int i = 2; i < argc; ++i) {
            if (!std::strcmp(argv[i], "--ingest") && i + 1 < argc) { deviceIngest = !std::strcmp(argv[++i], "device"); }
            else if (!std::strcmp(argv[i], "--decode-threads") && i + 1 < argc) decodeThreads = (unsigned int)std::atoi(argv[++i]);
            else if (!std::strcmp(argv[i], "--record") && i + 1 < argc) recordPath = argv[++i];
            else files.push_back(argv[i]);
        }
        const char* meshPath = nullptr;
        if (!files.empty()) {
            const size_t len = std::strlen(files.back());
            if (len > 4 && !std::strcmp(files.back() + len - 4, ".ply")) { meshPath = files.back(); files.pop_back(); }
        }
        GlobalAppState& gas = GlobalAppState::get();
        GlobalBundlingState& gbs = GlobalBundlingState::get();
        if (files.size() >= 2) { gas.readMembers(files[0]); gbs.readMembers(files[1]); }
        SensorDataReader sensor;                                     // (the device ingest uses it for the description and the evaluation only)
        sensor.createFirstConnected(argv[1]);
        if (files.size() < 2) { gas.s_integrationWidth = sensor.getDepthWidth(); gas.s_integrationHeight = sensor.getDepthHeight(); }
        gas.s_sensorIdx = 8;
        bf_pipeline* p = nullptr;
        check(bf_pipeline_create(&gas, &gbs, &sensor.desc(), &p));
        if (recordPath) {                                            // s_recordData: every accepted frame is packed on the device and encoded on the recorder's threads
            bf_record_state rs;
            check(files.size() >= 2 ? bf_record_state_read(files[0], &rs, nullptr) : bf_record_state_default(&rs));
            rs.s_recordData = 1; rs.s_recordCompression = 1;
            check(bf_pipeline_set_record_state(p, &rs, 0, nullptr));
        }
        unsigned int frames = 0;
        if (deviceIngest) {
            SensPlayer player;
            player.open(argv[1]);
            player.start(p, decodeThreads);
            while (player.next()) ++frames;
        } else {
            while (sensor.processDepth() && sensor.processColor()) {
                int got = 0;
                check(bf_pipeline_process_frame(p, sensor.getDepthFloat(), sensor.getColorRGBX(), &got));     // buffers are free again on return
                if (!got) break;
                ++frames;
            }
        }
        for (int k = 0; k < 5; ++k) check(bf_pipeline_process_end_of_sequence(p, nullptr));               // let the last solves and fixes finish
        check(bf_pipeline_synchronize(p));
        bf_online_bundler* ob = nullptr;
        check(bf_pipeline_get_online_bundler(p, &ob));
        bf_trajectory_manager* tm = nullptr;
        check(bf_online_bundler_get_trajectory_manager(ob, &tm));
        std::vector<mat4f> trajectory(frames);
        uint32_t n = 0;
        if (frames) check(bf_trajectory_manager_get_optimized_transforms(tm, trajectory[0].m, frames, &n));
        trajectory.resize(n);
        uint32_t nInt = 0, nDe = 0, nLocal = 0, nGlobal = 0;
        check(bf_pipeline_get_counters(p, &nInt, &nDe, &nLocal, &nGlobal));
        std::printf("%s: %u frames, %u integrations, %u de-integrations, %u local / %u global solves\n", sensor.getSensorName().c_str(), frames, nInt, nDe, nLocal, nGlobal);
        sensor.evaluateTrajectory(trajectory);
        if (recordPath) {
            char actual[4096]; uint64_t written = 0;
            check(bf_pipeline_save_recording(p, recordPath, 0, actual, sizeof actual, &written));
            std::printf("%s: %llu recorded frames with their optimised poses\n", actual, (unsigned long long)written);
        }
        if (meshPath) {
            uint32_t nv = 0, nf = 0, nt = 0;
            check(bf_pipeline_save_mesh(p, meshPath, nullptr, &nv, &nf, &nt));
            std::printf("%s: %u vertices, %u faces from %u triangles\n", meshPath, nv, nf, nt);
        }
        check(bf_pipeline_destroy(p));
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
