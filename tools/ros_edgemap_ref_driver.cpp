// Driver of the reference's own arithmetic for the ROS nodelet's per-KeyLine output, for tools/make_ros_edgemap_golden.py (build
// machine only, never shipped).  It stands in for the loop of RebvoNodelet::edgeMapPubCb (ros/src/rebvo_ros/src/rebvo_nodelet.cpp:176-212),
// which cannot be compiled without ROS: the reference's KeyLine (mtracklib/edge_finder.h) and cam_model (UtilLib/cam_model.h) are
// included in place, the point is the reference's own cam_model::unprojectHomCordVec on TooN::makeVector(kl.p_m.x, kl.p_m.y,
// kl.rho / K) narrowed to float as PointCloud2Iterator<float> stores it, and the message fields are assigned, as the nodelet assigns
// them, into locals of the C++ types genmsg gives Keyline.msg (float32 -> float, float64 -> double, int32 -> int32_t, int16 -> int16_t).
//
// stdin : int32 kn; double K; float zfx, zfy; kn x 168-byte KeyLines
// stdout: double zfm; kn x {float x, y, z}; kn x 52-byte records in Keyline.msg order
#include <cstdio>
#include <cstdint>
#include <vector>

#include <TooN/TooN.h>
#include "UtilLib/cam_model.h"
#include "mtracklib/edge_finder.h"

using namespace rebvo;

static bool rd(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }
template <class T> static void wr(const T &v) { fwrite(&v, sizeof v, 1, stdout); }

int main() {
    int32_t kn;
    double K;
    float zf[2];
    if (!rd(&kn, 4) || !rd(&K, 8) || !rd(zf, 8)) return 2;
    static_assert(sizeof(KeyLine) == 168, "KeyLine layout");
    if (kn < 0 || kn > KEYLINE_MAX) return 3;
    std::vector<KeyLine> kls(kn > 0 ? kn : 1);
    if (kn > 0 && !rd(kls.data(), sizeof(KeyLine) * (size_t)kn)) return 4;
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {376u, 240u};
    cam_model cam({0.f, 0.f}, {zf[0], zf[1]}, kc, sz);
    wr(cam.zfm);
    for (int i = 0; i < kn; i++) {
        KeyLine &kl = kls[i];
        TooN::Vector<3> p3d = cam.unprojectHomCordVec(TooN::makeVector(kl.p_m.x, kl.p_m.y, kl.rho / K));
        float out_x = p3d[0], out_y = p3d[1], out_z = p3d[2];
        wr(out_x); wr(out_y); wr(out_z);
    }
    for (int i = 0; i < kn; i++) {
        KeyLine &kl = kls[i];
        float KlGrad[2], KlImgPos[2], KlFocPos[2];
        double invDepth, invDepthS;
        int32_t KlMatchID, ConsMatch;
        int16_t KlPrevMatchID, KlNextMatchID;
        KlGrad[0] = kl.m_m.x;
        KlGrad[1] = kl.m_m.y;
        KlImgPos[0] = kl.c_p.x;
        KlImgPos[1] = kl.c_p.y;
        invDepth = kl.rho;
        invDepthS = kl.s_rho;
        KlFocPos[0] = kl.p_m.x;
        KlFocPos[1] = kl.p_m.y;
        KlMatchID = kl.m_id;
        ConsMatch = kl.m_num;
        KlPrevMatchID = kl.p_id;
        KlNextMatchID = kl.n_id;
        wr(KlGrad); wr(KlImgPos); wr(invDepth); wr(invDepthS); wr(KlFocPos); wr(KlMatchID); wr(ConsMatch); wr(KlPrevMatchID); wr(KlNextMatchID);
    }
    return 0;
}
