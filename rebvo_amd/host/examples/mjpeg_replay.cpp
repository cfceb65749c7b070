// mjpeg_replay — N rebvo::REBVO objects in ONE batch group fed from .mjpeg files (for instance the ones video_replay writes): what a USB
// or network camera delivers.  A file is split into frames at SOI / EOI; object i reads file i % files, and its frame k is the file's
// frame k % frames, stamped t0 + k dt.  By default the frames go in through REBVO::pushCustomCamJpeg with &GPU CompressedUpload = 1: they
// cross the bus compressed and the device decodes them.  --raw feeds the same frames decoded by the host reader through
// requestCustomCamBuffer, as an application without the call would.
//
//   mjpeg_replay <GlobalConfig> <objects> <frames_per_object> <t0> <dt> [--raw] [--callback] [--rawvideo PREFIX] file.mjpeg [file.mjpeg ...]
//
// --rawvideo PREFIX: VideoSave = 1 with EncoderType 0, object i's frames as the camera delivered them into PREFIX.<i>.rgb24.
// Prints the last nav record of every object ("nav <i> t Pos[3] Vel[3] RotLie[3] PoseLie[3]", 17 significant digits) and, as the last
// line, JSON: {"objects": N, "frames_per_object": K, "raw": 0|1, "callbacks": ..., "imgc_sum": ...} (imgc_sum: the byte sum of every
// PipeBuffer::imgc the callbacks saw, with --callback).
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "rebvo/jpeg_encode.h"
#include "rebvo/rebvo.h"

using namespace rebvo;

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the frames of an MJPEG file: from every FF D8 to the next FF D9 (stuffing keeps FF D9 out of entropy-coded data)
static std::vector<std::vector<uint8_t>> split_mjpeg(const std::vector<uint8_t> &d) {
    std::vector<std::vector<uint8_t>> out;
    size_t p = 0;
    while (p + 1 < d.size()) {
        if (!(d[p] == 0xFF && d[p + 1] == 0xD8)) { p++; continue; }
        size_t e = p + 2;
        while (e + 1 < d.size() && !(d[e] == 0xFF && d[e + 1] == 0xD9)) e++;
        if (e + 1 >= d.size()) break;
        out.emplace_back(d.begin() + p, d.begin() + e + 2);
        p = e + 2;
    }
    return out;
}

struct Sink {
    std::atomic<int> calls{0};
    std::atomic<unsigned long long> sum{0};
    size_t bytes = 0;
    bool cb(PipeBuffer &p) {
        calls++;
        if (p.imgc) {
            const uint8_t *q = reinterpret_cast<const uint8_t *>(p.imgc->Data());
            unsigned long long s = 0;
            for (size_t i = 0; i < bytes; i++) s += q[i];
            sum += s;
        }
        return true;
    }
};

int main(int argc, char **argv) {
    if (argc < 7) {
        std::cout << "usage: mjpeg_replay <GlobalConfig> <objects> <frames_per_object> <t0> <dt> [--raw] [--callback] [--rawvideo PREFIX] file.mjpeg [file.mjpeg ...]\n";
        return 2;
    }
    const int N = std::atoi(argv[2]), K = std::atoi(argv[3]);
    const double t0 = std::atof(argv[4]), dt = std::atof(argv[5]);
    bool raw = false, callback = false;
    std::string rawvideo;
    std::vector<std::vector<std::vector<uint8_t>>> files;
    for (int a = 6; a < argc; a++) {
        if (!std::strcmp(argv[a], "--raw")) { raw = true; continue; }
        if (!std::strcmp(argv[a], "--callback")) { callback = true; continue; }
        if (!std::strcmp(argv[a], "--rawvideo") && a + 1 < argc) { rawvideo = argv[++a]; continue; }
        std::ifstream in(argv[a], std::ios::binary);
        const std::vector<uint8_t> d((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        files.push_back(split_mjpeg(d));
        if (files.back().empty()) { std::cout << "no frames in " << argv[a] << "\n"; return 5; }
    }
    if (N < 1 || K < 1 || files.empty()) { std::cout << "bad arguments\n"; return 2; }
    REBVO proto(argv[1]);
    if (!proto.isInitOk()) { std::cout << "config error\n"; return 3; }
    REBVOParameters prm = proto.getParams();
    prm.GpuBatchGroup = "mjpeg";
    prm.GpuBatchSize = N;
    prm.GpuCompressedUpload = !raw;
    const size_t fb = (size_t)prm.ImageSize.w * prm.ImageSize.h * 3;
    std::vector<std::unique_ptr<REBVO>> obj;
    std::vector<std::unique_ptr<Sink>> sink;
    for (int i = 0; i < N; i++) {
        if (!rawvideo.empty()) {
            prm.VideoSave = 1;
            prm.encoder_type = 0;
            prm.VideoSaveBuffersize = (int)(fb * (size_t)K);
            prm.VideoSaveFile = rawvideo + "." + std::to_string(i) + ".rgb24";
        }
        obj.emplace_back(new REBVO(prm));
        sink.emplace_back(new Sink);
        sink[i]->bytes = fb;
        if (!obj[i]->isInitOk()) { std::cout << "object " << i << ": bad parameters\n"; return 3; }
        if (callback) obj[i]->setOutputCallback(&Sink::cb, sink[i].get());
    }
    for (int i = 0; i < N; i++)
        if (!obj[i]->Init()) { std::cout << "object " << i << ": Init failed: " << obj[i]->lastError() << "\n"; return 4; }
    bool bad = false;
    std::vector<uint8_t> px(fb);
    for (int k = 0; k < K && !bad; k++)
        for (int i = 0; i < N && !bad; i++) {
            const std::vector<std::vector<uint8_t>> &fr = files[i % files.size()];
            const std::vector<uint8_t> &f = fr[k % fr.size()];
            if (raw) {
                int w = 0, h = 0;
                if (rebvo_decode_jpeg(f.data(), (long long)f.size(), px.data(), (long long)fb, &w, &h) != 0 || w != (int)prm.ImageSize.w || h != (int)prm.ImageSize.h) {
                    std::cout << "frame " << k << " of object " << i << " does not decode to the configured size\n";
                    bad = true;
                    break;
                }
                std::shared_ptr<Image<RGB24Pixel>> ptr;
                while (!obj[i]->requestCustomCamBuffer(ptr, t0 + dt * k, 0.1))
                    if (!obj[i]->Running()) { bad = true; break; }
                if (bad) break;
                (*ptr).copyFrom(reinterpret_cast<const RGB24Pixel *>(px.data()));
                obj[i]->releaseCustomCamBuffer();
            } else {
                const double give_up = now_s() + 30;
                while (!obj[i]->pushCustomCamJpeg(f.data(), f.size(), t0 + dt * k, 0.1))
                    if (!obj[i]->Running() || now_s() > give_up) { bad = true; break; }
            }
        }
    const double deadline = now_s() + 30, t_last = t0 + dt * (K - 1);
    for (int i = 0; i < N && !bad; i++)
        while (obj[i]->getNav().t < t_last - 1e-9 * (1 + std::fabs(t_last))) {
            if (!obj[i]->Running() || now_s() > deadline) { bad = true; break; }
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    std::vector<NavData> nav;
    for (int i = 0; i < N; i++) nav.push_back(obj[i]->getNav());
    for (int i = 0; i < N; i++) obj[i]->CleanUp();
    if (bad) { std::cout << "an object stopped before its last frame\n"; return 6; }
    int calls = 0;
    unsigned long long sum = 0;
    for (int i = 0; i < N; i++) {
        const NavData &n = nav[i];
        std::printf("nav %d %.17g", i, n.t);
        for (const Vector3 *v : {&n.Pos, &n.Vel, &n.RotLie, &n.PoseLie})
            for (int j = 0; j < 3; j++) std::printf(" %.17g", v->v[j]);
        std::printf("\n");
        calls += sink[i]->calls;
        sum += sink[i]->sum;
    }
    std::printf("{\"objects\": %d, \"frames_per_object\": %d, \"raw\": %d, \"callbacks\": %d, \"imgc_sum\": %llu}\n", N, K, raw ? 1 : 0, calls, sum);
    return 0;
}
