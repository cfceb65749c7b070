// keyframe_replay — what the reference's user does with rebvorun's `k` key (app/rebvorun/main.cpp:114-115, 133): N rebvo::REBVO objects
// with TrackKeyFrames = 1 replay raw frames, key-frame saving is switched on and off at given frames, and after CleanUp() every object's
// REBVO::kf_list goes into a key-frame file the reference's kf_visualizer loads.  Used by tests/test_keyframe_host_gpu.py.
//
//   keyframe_replay <GlobalConfig> <frames.rgb24> <objects> <frames_per_object> <t0> <dt> <out_prefix>
//                   [--group NAME] [--start F] [--end F] [--disagree] [--map] [--covis] [--constraint] [--depth] [--relocalize [N]]
//
// frames.rgb24 = objects x frames_per_object x ImageHeight x ImageWidth x 3 bytes: object i's frame k is frame i * frames_per_object + k
// and carries the stamp t0 + k dt.  --group puts all objects into one batch group of that name (without it every object has its own
// context).  startKeyFrames() is called on every object before its frame F of --start is handed over, endKeyFrames() before frame F of
// --end.  --disagree: object 1 is built with TrackKeyFrames switched the other way (a group refuses it at Init()).  Output:
// <out_prefix>kf_<i>.kf per object, and one line "object <i>: <n> key frames" on stdout.
// --map: what app/kf_visualizer/main.cpp:84-116 does with object 0's list, through the C ABI of the device library: every key frame's
// KeyLines into a ring slot (edgehip_upload_keylines), edgehip_depth_fill, edgehip_surface_view_capture with its pose; then
// edgehip_surface_space, edgehip_surface_integrate and the visibility download.  Prints "view <j>: <hidden> of <cells> cells hidden".
// --covis: after the last frame's record and before CleanUp(), REBVO::keyframeCovisibility of every object with (SearchRange, 0,
// MatchThreshModule, MatchThreshAngle in radians, 3, SearchRange).  Prints "covis <i> m <m>:" and the m x m x 4 counts, [to][from].
// --constraint: at the same point, REBVO::keyframeConstraint of every object in both directions with (iter_max, k_huber) = (10, 2): the
// current key frame against the newest frame.  Prints "constraint <i> dir <d>:" and X[6], ratio, E, E0, Kp, W_Kp with 17 significant
// digits, then links, inliers, evals, accepted, guard.
// --relocalize [N]: REBVO::keyframeRelocalize of every object against all its positions with (SearchRange, 0, iter_max 5, rew_dis 2,
// rho_tol 3): the newest frame against every key frame the device holds.  With N, after every N-th frame but the first (the objects are then
// stepped frame by frame, as with --depth): "relocalize <i> frame <k> position <t>: <mnum> <score_ratio> <Kp>" for every position the
// object has.  Before CleanUp(), at the same point as --covis: "relocalize <i> position <t>:" and mnum, evals, accepted, guard, then
// score_ratio, Kp, K, X[6], Pose[9], Pos[3] with 17 significant digits, for all positions.
// --depth: REBVO::keyframeMapDepth of every object with (ReshapeQAbsolute, ReshapeQRelative, LocationUncertainty) = (1e-3, 5e-2, 2) after
// every frame but the first (the objects are then stepped frame by frame: each frame's record is waited for).  Prints "mapdepth <i> frame <k>: <count>";
// before CleanUp(), REBVO::keyframeTranslateDepth (0, optim_scale) and then (1, false) of every object: "translate <i> dir <d>:" and
// count, guard, K, rTr, rTr0 (17 significant digits).  With or without the flag the run ends with "depth <i>: median s_rho <x> of <n>
// KeyLines" for every object's current key frame (the last entry of its kf_list), so two runs show what the flag did to it.
#include <algorithm>
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

#include "edgehip.h"
#include "rebvo/rebvo.h"

using namespace rebvo;

static int map_views(const REBVOParameters &prm, std::vector<keyframe> &list) {
    if (list.empty()) { std::cout << "--map: no key frames\n"; return 0; }
    edgehip_params hp;
    edgehipParams(prm, hp);
    edgehip_ctx *ctx = nullptr;
    int rc = edgehip_create(&hp, 1, 2, prm.GpuDevice, &ctx);
    edgehip_depth_fill_params dfp;
    std::memset(&dfp, 0, sizeof dfp);
    dfp.block_w = dfp.block_h = prm.DF_BlockSize > 0 ? prm.DF_BlockSize : 5;   // app/kf_visualizer's defaults where the config has no &DepthFiller
    dfp.iter_num = prm.DF_BlockSize > 0 ? prm.DF_IterNum : 10;
    dfp.thresh_rel_rho = prm.DF_BlockSize > 0 ? prm.DF_ThreshRelRho : 1.0;
    dfp.thresh_match_num = prm.DF_BlockSize > 0 ? prm.DF_ThreshMatchNum : 5;
    dfp.bound_mode = EDGEHIP_BOUND_NONE;
    dfp.discard = 1;
    edgehip_surface_views_params svp = {(int32_t)list.size(), 100, 100, 100};
    if (rc == 0) rc = edgehip_depth_fill_enable(ctx, &dfp);
    if (rc == 0) rc = edgehip_surface_views_enable(ctx, &svp);
    for (size_t j = 0; j < list.size() && rc == 0; j++) {
        keyframe &kf = list[j];
        double Pose[9], Pos[3];
        for (int i = 0; i < 9; i++) Pose[i] = kf.Pose(i / 3, i % 3);
        for (int i = 0; i < 3; i++) Pos[i] = kf.Pos[i];
        static const edgehip_keyline none = {};
        rc = edgehip_upload_keylines(ctx, 0, 0, kf.KNum() ? reinterpret_cast<const edgehip_keyline *>(kf.kl.data()) : &none, kf.KNum(), nullptr, 0.f);
        if (rc == 0) rc = edgehip_depth_fill(ctx, 0);
        if (rc == 0) rc = edgehip_surface_view_capture(ctx, 0, (int)j, Pose, Pos, kf.K);
    }
    double origin[3], size[3];
    if (rc == 0) rc = edgehip_surface_space(ctx, origin, size);
    if (rc == 0) rc = edgehip_surface_integrate(ctx, origin, size, 0, nullptr, 0);
    int32_t gw = 0, gh = 0;
    if (rc == 0) rc = edgehip_depth_fill_size(ctx, &gw, &gh);
    std::vector<uint8_t> vis((size_t)gw * gh);
    for (size_t j = 0; j < list.size() && rc == 0; j++) {
        rc = edgehip_download_surface_visibility(ctx, (int)j, vis.data());
        size_t hidden = 0;
        for (uint8_t v : vis) hidden += v == 0;
        if (rc == 0) std::cout << "view " << j << ": " << hidden << " of " << vis.size() << " cells hidden\n";
    }
    if (rc != 0) std::cout << "--map failed: " << edgehip_last_error() << "\n";
    if (ctx) edgehip_destroy(ctx);
    return rc;
}

int main(int argn, char **argv) {
    if (argn < 8) {
        std::cout << "usage: keyframe_replay <GlobalConfig> <frames.rgb24> <objects> <frames_per_object> <t0> <dt> <out_prefix> "
                     "[--group NAME] [--start F] [--end F] [--disagree] [--map] [--covis] [--constraint] [--depth] [--relocalize [N]]\n";
        return 2;
    }
    const int N = atoi(argv[3]), K = atoi(argv[4]);
    const double t0 = atof(argv[5]), dt = atof(argv[6]);
    const std::string prefix = argv[7];
    std::string group;
    int start = -1, end = -1;
    bool disagree = false, map = false, covis = false, constraint = false, depth = false, relocalize = false;
    int reloc_every = 0;
    for (int a = 8; a < argn; a++) {
        const std::string s = argv[a];
        if (s == "--group" && a + 1 < argn) group = argv[++a];
        else if (s == "--start" && a + 1 < argn) start = atoi(argv[++a]);
        else if (s == "--end" && a + 1 < argn) end = atoi(argv[++a]);
        else if (s == "--disagree") disagree = true;
        else if (s == "--map") map = true;
        else if (s == "--covis") covis = true;
        else if (s == "--constraint") constraint = true;
        else if (s == "--depth") depth = true;
        else if (s == "--relocalize") {
            relocalize = true;
            if (a + 1 < argn && argv[a + 1][0] >= '0' && argv[a + 1][0] <= '9') reloc_every = atoi(argv[++a]);
        }
        else { std::cout << "unknown argument " << s << "\n"; return 2; }
    }
    if (N < 1 || K < 2) { std::cout << "bad counts\n"; return 2; }

    REBVO proto(argv[1]);
    if (!proto.isInitOk()) { std::cout << "config error\n"; return 3; }
    REBVOParameters prm = proto.getParams();
    if (!group.empty()) { prm.GpuBatchGroup = group; prm.GpuBatchSize = N; }
    const size_t fb = (size_t)prm.ImageSize.w * prm.ImageSize.h * 3;
    std::vector<uint8_t> pool(fb * N * K);
    {
        std::ifstream in(argv[2], std::ios::binary);
        in.read(reinterpret_cast<char *>(pool.data()), (std::streamsize)pool.size());
        if (!in.is_open() || (size_t)in.gcount() != pool.size()) { std::cout << "cannot read " << argv[2] << "\n"; return 5; }
    }
    std::vector<std::unique_ptr<REBVO>> obj;
    for (int i = 0; i < N; i++) {
        REBVOParameters p = prm;
        if (disagree && i == 1) { p.TrackKeyFrames = !p.TrackKeyFrames; p.KFSavePercent = prm.KFSavePercent; }
        obj.emplace_back(new REBVO(p));
    }
    for (int i = 0; i < N; i++)
        if (!obj[i]->Init()) {
            std::cout << "object " << i << ": Init failed: " << obj[i]->lastError() << "\n";
            for (int j = 0; j < i; j++) obj[j]->CleanUp();
            return 4;
        }
    bool bad = false;
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(60);
    // every object's record of the frame stamped t
    auto wait_for = [&](double t) {
        for (int i = 0; i < N && !bad; i++)
            while (obj[i]->getNav().t < t - 1e-9 * (1 + std::fabs(t))) {
                if (!obj[i]->Running() || std::chrono::steady_clock::now() > deadline) { bad = true; break; }
                std::this_thread::sleep_for(std::chrono::microseconds(100));
            }
    };
    for (int k = 0; k < K && !bad; k++) {
        for (int i = 0; i < N && !bad; i++) {
            if (k == start) obj[i]->startKeyFrames();
            if (k == end) obj[i]->endKeyFrames();
            std::shared_ptr<Image<RGB24Pixel>> ptr;
            while (!obj[i]->requestCustomCamBuffer(ptr, t0 + dt * k, 0.1))
                if (!obj[i]->Running()) { bad = true; break; }
            if (bad) break;
            (*ptr).copyFrom(reinterpret_cast<const RGB24Pixel *>(pool.data() + fb * ((size_t)i * K + k)));
            obj[i]->releaseCustomCamBuffer();
        }
        const bool reloc_now = reloc_every > 0 && k % reloc_every == 0;
        if ((!depth && !reloc_now) || k == 0) continue;   // (the first frame has no record and no key frame)
        wait_for(t0 + dt * k);
        for (int i = 0; i < N && reloc_now && !bad; i++) {
            KfRelocArgs ra;
            ra.field_radius = (int)prm.SearchRange; ra.field_min_mod = 0.f; ra.iter_max = 5; ra.rew_dis = 2.0; ra.rho_tol = 3.0;
            std::vector<KfReloc> rows;
            int m = 0;
            if (!obj[i]->keyframeRelocalize(ra, nullptr, rows, m)) { std::cout << "relocalize " << i << " frame " << k << ": refused\n"; continue; }
            for (int t = 0; t < m; t++) {
                if (rows[(size_t)t].mnum < 0) continue;
                char buf[96];
                snprintf(buf, sizeof buf, " %.17g %.17g", rows[(size_t)t].score_ratio, rows[(size_t)t].Kp);
                std::cout << "relocalize " << i << " frame " << k << " position " << t << ": " << rows[(size_t)t].mnum << buf << "\n";
            }
        }
        for (int i = 0; i < N && depth && !bad; i++) {
            int count = 0;
            if (!obj[i]->keyframeMapDepth(1e-3, 5e-2, 2.0, count)) { std::cout << "mapdepth " << i << " frame " << k << ": refused\n"; continue; }
            std::cout << "mapdepth " << i << " frame " << k << ": " << count << "\n";
        }
    }
    // every object's record of its last frame, then the end
    wait_for(t0 + dt * (K - 1));
    for (int i = 0; i < N && covis && !bad; i++) {
        KfCovisArgs ca;
        ca.field_radius = (int)prm.SearchRange; ca.field_min_mod = 0.f;
        ca.match_mod = (float)prm.MatchThreshModule; ca.match_ang = (float)(prm.MatchThreshAngle * M_PI / 180.0);
        ca.rho_tol = 3.f; ca.max_r = (float)prm.SearchRange;
        std::vector<KfPairCount> rows;
        int m = 0;
        if (!obj[i]->keyframeCovisibility(ca, rows, m)) { std::cout << "covis " << i << ": refused\n"; continue; }
        std::cout << "covis " << i << " m " << m << ":";
        for (const KfPairCount &c : rows) std::cout << " " << c.kl_on_fov << " " << c.kl_match << " " << c.kls_on_fov << " " << c.guard;
        std::cout << "\n";
    }
    for (int i = 0; i < N && constraint && !bad; i++)
        for (int d = 0; d < 2; d++) {
            KfConstraintArgs ka;
            ka.direction = d; ka.iter_max = 10; ka.k_huber = 2.0;
            KfConstraint kc;
            if (!obj[i]->keyframeConstraint(ka, kc)) { std::cout << "constraint " << i << " dir " << d << ": refused\n"; continue; }
            char buf[64];
            std::cout << "constraint " << i << " dir " << d << ":";
            const double v[11] = {kc.X[0], kc.X[1], kc.X[2], kc.X[3], kc.X[4], kc.X[5], kc.ratio, kc.E, kc.E0, kc.Kp, kc.W_Kp};
            for (double x : v) { snprintf(buf, sizeof buf, " %.17g", x); std::cout << buf; }
            std::cout << " " << kc.links << " " << kc.inliers << " " << kc.evals << " " << kc.accepted << " " << kc.guard << "\n";
        }
    for (int i = 0; i < N && relocalize && !bad; i++) {
        KfRelocArgs ra;
        ra.field_radius = (int)prm.SearchRange; ra.field_min_mod = 0.f; ra.iter_max = 5; ra.rew_dis = 2.0; ra.rho_tol = 3.0;
        std::vector<KfReloc> rows;
        int m = 0;
        if (!obj[i]->keyframeRelocalize(ra, nullptr, rows, m)) { std::cout << "relocalize " << i << ": refused\n"; continue; }
        for (int t = 0; t < m; t++) {
            const KfReloc &r = rows[(size_t)t];
            char buf[64];
            std::cout << "relocalize " << i << " position " << t << ": " << r.mnum << " " << r.evals << " " << r.accepted << " " << r.guard;
            std::vector<double> v = {r.score_ratio, r.Kp, r.K};
            v.insert(v.end(), r.X, r.X + 6); v.insert(v.end(), r.Pose, r.Pose + 9); v.insert(v.end(), r.Pos, r.Pos + 3);
            for (double x : v) { snprintf(buf, sizeof buf, " %.17g", x); std::cout << buf; }
            std::cout << "\n";
        }
    }
    for (int i = 0; i < N && depth && !bad; i++)
        for (int d = 0; d < 2; d++) {
            KfDepth kd;
            if (!obj[i]->keyframeTranslateDepth(d, d == 0, kd)) { std::cout << "translate " << i << " dir " << d << ": refused\n"; continue; }
            char buf[64];
            std::cout << "translate " << i << " dir " << d << ": " << kd.count << " " << kd.guard;
            for (double x : {kd.K, kd.rTr, kd.rTr0}) { snprintf(buf, sizeof buf, " %.17g", x); std::cout << buf; }
            std::cout << "\n";
        }
    for (int i = 0; i < N; i++) obj[i]->CleanUp();
    if (bad) { std::cout << "an object stopped early: " << obj[0]->lastError() << "\n"; return 6; }
    for (int i = 0; i < N; i++) {
        const std::string name = prefix + "kf_" + std::to_string(i) + ".kf";
        if (!keyframe::saveKeyframes2File(name.c_str(), obj[i]->kf_list)) { std::cout << "cannot write " << name << "\n"; return 7; }
        std::cout << "object " << i << ": " << obj[i]->kf_list.size() << " key frames\n";
        if (!obj[i]->kf_list.empty()) {   // the current key frame's depth uncertainty
            std::vector<double> s;
            for (const KeyLine &kl : obj[i]->kf_list.back().kl) s.push_back(kl.s_rho);
            std::sort(s.begin(), s.end());
            char buf[64];
            snprintf(buf, sizeof buf, "%.17g", s.empty() ? 0.0 : s[s.size() / 2]);
            std::cout << "depth " << i << ": median s_rho " << buf << " of " << s.size() << " KeyLines\n";
        }
    }
    if (map && map_views(prm, obj[0]->kf_list) != 0) return 8;
    return 0;
}
