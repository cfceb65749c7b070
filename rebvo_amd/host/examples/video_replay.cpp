// video_replay — N rebvo::REBVO objects in ONE batch group, fed through the plugin surface like surface_replay, with the video half of the
// reference's third thread switched on: every frame is compressed on the device (EncoderType 1: MJPEGEncoder at quality 90) and appended
// to the object's VideoSave buffer, which goes to its VideoSaveFile when the object stops; the output callbacks see the same bytes as
// PipeBuffer::jpeg and, with --net, the packet the third thread would send as PipeBuffer::net_packet.
//
//   video_replay <GlobalConfig> <frames.rgb24> <pool_frames> <objects> <frames_per_object> <t0> <dt> --video PREFIX
//                [--buffersize BYTES] [--encoder 0|1] [--net] [--delay FRAMES] [--dump PREFIX]
//
// Object i's frame k is pool frame tri(k + i), stamped t0 + k dt; its VideoSaveFile is <--video PREFIX>.<i>.mjpeg.  --dump PREFIX: every
// callback of object i appends to PREFIX.<i>.cb, in binary: int32 p_id, jpeg_size, packet size (-1: none), then the frame's bytes and the
// packet's.  The last line on stdout is JSON: {"objects": N, "frames_per_object": K, "callbacks": ..., "jpeg_bytes": ...}
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "rebvo/rebvo.h"

using namespace rebvo;

static int tri(long k, int n) {
    if (n < 2) return 0;
    const int p = 2 * (n - 1);
    const int r = (int)(k % p);
    return r < n ? r : p - r;
}
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Sink {
    std::ofstream dump;
    std::atomic<int> calls{0};
    std::atomic<long> bytes{0};
    bool cb(PipeBuffer &p) {
        calls++;
        bytes += (long)p.jpeg_size;
        if (!dump.is_open()) return true;
        const int32_t hdr[3] = {p.p_id, (int32_t)p.jpeg_size, p.net_packet ? (int32_t)p.net_packet->size() : -1};
        dump.write(reinterpret_cast<const char *>(hdr), sizeof hdr);
        if (p.jpeg) dump.write(reinterpret_cast<const char *>(p.jpeg), (std::streamsize)p.jpeg_size);
        if (p.net_packet) dump.write(reinterpret_cast<const char *>(p.net_packet->data()), (std::streamsize)p.net_packet->size());
        dump.flush();
        return true;
    }
};

int main(int argc, char **argv) {
    if (argc < 8) {
        std::cout << "usage: video_replay <GlobalConfig> <frames.rgb24> <pool_frames> <objects> <frames_per_object> <t0> <dt> --video PREFIX "
                     "[--buffersize BYTES] [--encoder 0|1] [--net] [--delay FRAMES] [--dump PREFIX]\n";
        return 2;
    }
    const int pool_frames = std::atoi(argv[3]), N = std::atoi(argv[4]), K = std::atoi(argv[5]);
    const double t0 = std::atof(argv[6]), dt = std::atof(argv[7]);
    std::string dump_prefix, video_prefix;
    int W = 0, buffersize = 64 << 20, encoder = 1, delay = 0;
    bool net = false;
    for (int a = 8; a < argc; a++) {
        if (!std::strcmp(argv[a], "--dump") && a + 1 < argc) dump_prefix = argv[++a];
        else if (!std::strcmp(argv[a], "--video") && a + 1 < argc) video_prefix = argv[++a];
        else if (!std::strcmp(argv[a], "--buffersize") && a + 1 < argc) buffersize = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--encoder") && a + 1 < argc) encoder = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--delay") && a + 1 < argc) delay = std::atoi(argv[++a]);
        else if (!std::strcmp(argv[a], "--net")) net = true;
        else { std::cout << "unknown option " << argv[a] << "\n"; return 2; }
    }
    if (pool_frames < 1 || N < 1 || K < 1 || video_prefix.empty() || buffersize < 1 || delay < 0) { std::cout << "bad arguments\n"; return 2; }
    REBVO proto(argv[1]);
    if (!proto.isInitOk()) { std::cout << "config error\n"; return 3; }
    REBVOParameters prm = proto.getParams();
    prm.GpuBatchGroup = "video";
    prm.VideoSave = 1;
    prm.VideoSaveBuffersize = buffersize;
    prm.encoder_type = encoder;
    prm.VideoNetEnabled = net;
    prm.EdgeMapDelay = (uint)delay;
    prm.GpuBatchSize = N;
    const Size2D sz = prm.ImageSize;
    const size_t fb = (size_t)sz.w * sz.h * 3;
    std::vector<uint8_t> pool(fb * pool_frames);
    {
        std::ifstream in(argv[2], std::ios::binary);
        in.read(reinterpret_cast<char *>(pool.data()), (std::streamsize)pool.size());
        if (!in.is_open() || (size_t)in.gcount() != pool.size()) { std::cout << "cannot read " << argv[2] << "\n"; return 5; }
    }
    std::vector<std::unique_ptr<REBVO>> obj;
    std::vector<std::unique_ptr<Sink>> sink;
    for (int i = 0; i < N; i++) {
        prm.VideoSaveFile = video_prefix + "." + std::to_string(i) + ".mjpeg";
        obj.emplace_back(new REBVO(prm));
        sink.emplace_back(new Sink);
        if (!obj[i]->isInitOk()) { std::cout << "object " << i << ": bad parameters\n"; return 3; }
        if (!dump_prefix.empty()) sink[i]->dump.open(dump_prefix + "." + std::to_string(i) + ".cb", std::ios::binary);
        obj[i]->setOutputCallback(&Sink::cb, sink[i].get());
    }
    for (int i = 0; i < N; i++)
        if (!obj[i]->Init()) { std::cout << "object " << i << ": Init failed: " << obj[i]->lastError() << "\n"; return 4; }
    bool bad = false;
    double t_start = 0;
    for (int k = 0; k < K && !bad; k++) {
        if (k == W) t_start = now_s();
        for (int i = 0; i < N && !bad; i++) {
            std::shared_ptr<Image<RGB24Pixel>> ptr;
            while (!obj[i]->requestCustomCamBuffer(ptr, t0 + dt * k, 0.1))
                if (!obj[i]->Running()) { bad = true; break; }
            if (bad) break;
            (*ptr).copyFrom(reinterpret_cast<const RGB24Pixel *>(pool.data() + fb * tri((long)k + i, pool_frames)));
            obj[i]->releaseCustomCamBuffer();
        }
    }
    const double deadline = now_s() + 30, t_last = t0 + dt * (K - 1);
    for (int i = 0; i < N && !bad; i++)
        while (obj[i]->getNav().t < t_last - 1e-9 * (1 + std::fabs(t_last))) {
            if (!obj[i]->Running() || now_s() > deadline) { bad = true; break; }
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    const double seconds = now_s() - t_start;
    for (int i = 0; i < N; i++) obj[i]->CleanUp();
    if (bad) { std::cout << "an object stopped before its last frame\n"; return 6; }
    int calls = 0;
    long bytes = 0;
    for (int i = 0; i < N; i++) { calls += sink[i]->calls; bytes += sink[i]->bytes; }
    (void)seconds;
    std::printf("{\"objects\": %d, \"frames_per_object\": %d, \"callbacks\": %d, \"jpeg_bytes\": %ld}\n", N, K, calls, bytes);
    return 0;
}
