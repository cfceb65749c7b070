// ros_output_replay — N rebvo::REBVO objects in ONE batch group, fed through the plugin surface like surface_replay, whose output callbacks
// take what the reference's ROS nodelet builds (ros/src/rebvo_ros/src/rebvo_nodelet.cpp:176-212) ready-made from the PipeBuffer:
// PipeBuffer::point_cloud and PipeBuffer::edge_map_msg (&EdgeMapOutput PointCloud / KeylineMsg / KeyLineList in the GlobalConfig).
//
//   ros_output_replay <GlobalConfig> <frames.rgb24> <pool_frames> <objects> <frames_per_object> <t0> <dt> [--dump PREFIX] [--warmup W]
//                     [--compressed PREFIX] [--single]
// --single: the objects are not put into a batch group (each has its own context and tracking thread).
// --compressed PREFIX (&EdgeMapOutput CompressedEdgeMap = 1): every callback prints its record count and bytes beside the KeyLine list's,
// and appends to PREFIX.<i>.cem: int32 p_id, KNum(), count (-1: no compressed edge map), status, edgemap_id; float rho_scale; the KNum()
// KeyLine records (168 bytes each); the count records (5 bytes each).
//
// Object i's frame k is pool frame tri(k + i), stamped t0 + k dt (surface_replay's scheme).  --dump PREFIX: every callback of object i
// appends to PREFIX.<i>.ros, in binary: int32 p_id, KNum() of p.ef, cloud points (-1: no cloud), records (-1: no message); float64 K,
// nav.Pos[3], nav.PoseLie[3], nav.Vel[3]; then the cloud's xyz floats and the records' bytes (52 each).  The last line on stdout is JSON:
//   {"objects": N, "frames_per_object": K, "timed_frames": ..., "seconds": ..., "fps": ..., "callbacks": ..., "point_cloud": 0/1,
//    "keyline_msg": 0/1, "keyline_list": 0/1}
// timed over the frames after the first W of every object, from the submission of frame W until every object's getNav() shows its last frame.
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
    std::ofstream dump, cdump;
    int index = 0;
    void compressed(PipeBuffer &p) {
        const CompressedEdgeMap *cm = p.edge_map_compressed;
        const int kn = p.ef->KNum();
        std::printf("compressed edge map: object %d frame %d: %d records, %d bytes (KeyLine list: %d, %zu bytes)\n", index, p.p_id, cm ? cm->count : -1,
                    cm ? 5 * cm->count : 0, kn, (size_t)168 * kn);
        const int32_t hdr[5] = {p.p_id, kn, cm ? cm->count : -1, cm ? cm->status : 0, cm ? (int32_t)cm->edgemap_id : 0};
        const float scale = cm ? cm->rho_scale : 0.f;
        cdump.write(reinterpret_cast<const char *>(hdr), sizeof hdr);
        cdump.write(reinterpret_cast<const char *>(&scale), sizeof scale);
        if (kn > 0) cdump.write(reinterpret_cast<const char *>(&(*p.ef)[0]), (std::streamsize)((size_t)168 * kn));
        if (cm) cdump.write(reinterpret_cast<const char *>(cm->records.data()), (std::streamsize)(5 * (size_t)cm->count));
        cdump.flush();
    }
    std::atomic<int> calls{0};
    std::atomic<long> points{0};
    bool cb(PipeBuffer &p) {
        calls++;
        const PointCloud *pc = p.point_cloud;
        const EdgeMapMsg *em = p.edge_map_msg;
        if (pc) points += pc->n;
        if (cdump.is_open()) compressed(p);
        if (!dump.is_open()) return true;
        const int32_t hdr[4] = {p.p_id, p.ef->KNum(), pc ? pc->n : -1, em ? em->n : -1};
        dump.write(reinterpret_cast<const char *>(hdr), sizeof hdr);
        double nav[10] = {p.K};
        for (int i = 0; i < 3; i++) { nav[1 + i] = p.nav.Pos[i]; nav[4 + i] = p.nav.PoseLie[i]; nav[7 + i] = p.nav.Vel[i]; }
        dump.write(reinterpret_cast<const char *>(nav), sizeof nav);
        if (pc) dump.write(reinterpret_cast<const char *>(pc->xyz.data()), (std::streamsize)(12 * (size_t)pc->n));
        if (em) dump.write(reinterpret_cast<const char *>(em->records.data()), (std::streamsize)(52 * (size_t)em->n));
        dump.flush();
        return true;
    }
};

int main(int argc, char **argv) {
    if (argc < 8) {
        std::cout << "usage: ros_output_replay <GlobalConfig> <frames.rgb24> <pool_frames> <objects> <frames_per_object> <t0> <dt> [--dump PREFIX] [--warmup W]\n";
        return 2;
    }
    const int pool_frames = std::atoi(argv[3]), N = std::atoi(argv[4]), K = std::atoi(argv[5]);
    const double t0 = std::atof(argv[6]), dt = std::atof(argv[7]);
    std::string dump_prefix, comp_prefix;
    int W = 0;
    bool single = false;
    for (int a = 8; a < argc; a++) {
        if (!std::strcmp(argv[a], "--dump") && a + 1 < argc) dump_prefix = argv[++a];
        else if (!std::strcmp(argv[a], "--compressed") && a + 1 < argc) comp_prefix = argv[++a];
        else if (!std::strcmp(argv[a], "--single")) single = true;
        else if (!std::strcmp(argv[a], "--warmup") && a + 1 < argc) W = std::atoi(argv[++a]);
        else { std::cout << "unknown option " << argv[a] << "\n"; return 2; }
    }
    if (pool_frames < 1 || N < 1 || K < 1 || W < 0 || W >= K) { std::cout << "bad counts\n"; return 2; }
    REBVO proto(argv[1]);
    if (!proto.isInitOk()) { std::cout << "config error\n"; return 3; }
    REBVOParameters prm = proto.getParams();
    if (!single) {
        prm.GpuBatchGroup = "ros_output";
        prm.GpuBatchSize = N;
    }
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
        obj.emplace_back(new REBVO(prm));
        sink.emplace_back(new Sink);
        if (!obj[i]->isInitOk()) { std::cout << "object " << i << ": bad parameters\n"; return 3; }
        if (!dump_prefix.empty()) sink[i]->dump.open(dump_prefix + "." + std::to_string(i) + ".ros", std::ios::binary);
        sink[i]->index = i;
        if (!comp_prefix.empty()) sink[i]->cdump.open(comp_prefix + "." + std::to_string(i) + ".cem", std::ios::binary);
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
    long points = 0;
    for (int i = 0; i < N; i++) { calls += sink[i]->calls; points += sink[i]->points; }
    const long timed = (long)N * (K - W);
    std::printf("{\"objects\": %d, \"frames_per_object\": %d, \"timed_frames\": %ld, \"seconds\": %.6f, \"fps\": %.1f, \"callbacks\": %d, "
                "\"cloud_points\": %ld, \"point_cloud\": %d, \"keyline_msg\": %d, \"keyline_list\": %d}\n",
                N, K, timed, seconds, timed / seconds, calls, points, prm.EM_PointCloud, prm.EM_KeylineMsg, prm.EM_KeyLineList);
    return 0;
}
