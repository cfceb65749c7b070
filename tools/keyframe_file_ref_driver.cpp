// Driver of the reference's key-frame file for tools/make_keyframe_file_golden.py (build machine only, never shipped).
//
// Compiled into a temporary directory outside the repository, together with the reference's src/mtracklib/keyframe.cpp and
// src/visualizer/depth_filler.cpp, in place; everything else comes from oracle/_ref/libreforacle.so.
//
//   layout                    -> text: "<struct>.<field> <offset> <size>" for KeyLine and cam_model, and their sizeof
//   save IN OUT               -> builds keyframe objects with the reference's constructor from IN and runs keyframe::saveKeyframes2File(OUT).
//                                IN (this driver's own input format, parsed below): int32 n; per key frame double t, K, Rot[9], RotLie[3],
//                                Vel[3], Pose[9], PoseLie[3], Pos[3], max_r; float pp[2], zf[2]; double Kc[5]; int32 w, h; int32 kn;
//                                kn x 168-byte records.  max_r reaches the file the way it does upstream: through global_tracker::build_field.
//   load IN                   -> keyframe::loadKeyframesFromFile(IN); stdout: int32 n; per key frame the 32 doubles of the pose block,
//                                pp[2], zf[2] (float), zfm, Kc[5] (double), w, h (int32), kn (int32), then per KeyLine every field on its
//                                own, packed in declaration order (164 bytes: no padding)
//   fill IN bw bh iter thresh mnum discard
//                             -> loadKeyframesFromFile(IN), then per key frame initDepthFiller({bw, bh}, iter, thresh, mnum, BOUND_NONE, discard);
//                                stdout: int32 n; per key frame int32 gw, gh; double rho[gh*gw], s_rho[gh*gw]; uint8 fixed[gh*gw]
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mtracklib/edge_tracker.h"
#include "mtracklib/global_tracker.h"
#include "mtracklib/keyframe.h"

using namespace rebvo;
using namespace TooN;

static_assert(sizeof(KeyLine) == 168, "KeyLine layout");
static_assert(sizeof(cam_model) == 72, "cam_model layout");

template <class T> static void put(const T &v) { fwrite(&v, sizeof(T), 1, stdout); }
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

#define FIELD(S, f) printf(#S "." #f " %zu %zu\n", offsetof(S, f), sizeof(((S *)0)->f))

static int layout() {
    FIELD(KeyLine, p_inx); FIELD(KeyLine, m_m); FIELD(KeyLine, u_m); FIELD(KeyLine, n_m); FIELD(KeyLine, score); FIELD(KeyLine, c_p);
    FIELD(KeyLine, rho); FIELD(KeyLine, s_rho); FIELD(KeyLine, rho_nr); FIELD(KeyLine, s_rho_nr); FIELD(KeyLine, rho0); FIELD(KeyLine, s_rho0);
    FIELD(KeyLine, p_m); FIELD(KeyLine, p_m_0); FIELD(KeyLine, m_id); FIELD(KeyLine, m_id_f); FIELD(KeyLine, m_id_kf); FIELD(KeyLine, m_num);
    FIELD(KeyLine, m_m0); FIELD(KeyLine, n_m0); FIELD(KeyLine, p_id); FIELD(KeyLine, n_id); FIELD(KeyLine, net_id); FIELD(KeyLine, stereo_m_id);
    FIELD(KeyLine, stereo_rho); FIELD(KeyLine, stereo_s_rho);
    FIELD(cam_model, pp); FIELD(cam_model, zf); FIELD(cam_model, zfm); FIELD(cam_model, Kc); FIELD(cam_model, sz);
    printf("KeyLine.sizeof 0 %zu\ncam_model.sizeof 0 %zu\n", sizeof(KeyLine), sizeof(cam_model));
    return 0;
}

static int save(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    int32_t n;
    if (!f || !rd(f, &n, 4)) return 2;
    std::vector<keyframe> list;
    for (int i = 0; i < n; i++) {
        double d[33];
        float pz[4];
        double kc[5];
        int32_t wh[2], kn;
        if (!rd(f, d, sizeof d) || !rd(f, pz, sizeof pz) || !rd(f, kc, sizeof kc) || !rd(f, wh, sizeof wh) || !rd(f, &kn, 4)) return 3;
        cam_model::rad_tan_distortion Kc = {kc[0], kc[1], kc[2], kc[3], kc[4]};
        Size2D sz = {wh[0], wh[1]};
        cam_model cam({pz[0], pz[1]}, {pz[2], pz[3]}, Kc, sz);
        edge_tracker et(cam, 255 * 3);
        if (kn < 0 || kn > et.kl_size) return 4;
        if (!rd(f, et.kl, sizeof(KeyLine) * (size_t)kn)) return 5;
        et.kn = kn;
        global_tracker gt(et.GetCam());
        gt.build_field(et, (int)d[32]);
        Matrix<3, 3> Rot, Pose;
        Vector<3> RotLie, Vel, PoseLie, Pos;
        for (int k = 0; k < 9; k++) { Rot(k / 3, k % 3) = d[2 + k]; Pose(k / 3, k % 3) = d[17 + k]; }
        for (int k = 0; k < 3; k++) { RotLie[k] = d[11 + k]; Vel[k] = d[14 + k]; PoseLie[k] = d[26 + k]; Pos[k] = d[29 + k]; }
        list.push_back(keyframe(et, gt, d[0], d[1], Rot, RotLie, Vel, Pose, PoseLie, Pos));
    }
    fclose(f);
    return keyframe::saveKeyframes2File(out, list) ? 0 : 6;
}

static int load(const char *in, std::vector<keyframe> &list) { return keyframe::loadKeyframesFromFile(in, list) ? 0 : 2; }

static int dump(const char *in) {
    std::vector<keyframe> list;
    if (int e = load(in, list)) return e;
    put((int32_t)list.size());
    for (keyframe &kf : list) {
        put(kf.t); put(kf.K);
        for (int k = 0; k < 9; k++) put((double)kf.Rot(k / 3, k % 3));
        for (int k = 0; k < 3; k++) put((double)kf.RotLie[k]);
        for (int k = 0; k < 3; k++) put((double)kf.Vel[k]);
        for (int k = 0; k < 9; k++) put((double)kf.Pose(k / 3, k % 3));
        for (int k = 0; k < 3; k++) put((double)kf.PoseLie[k]);
        for (int k = 0; k < 3; k++) put((double)kf.Pos[k]);
        const cam_model &c = kf.camera;
        put(c.pp.x); put(c.pp.y); put(c.zf.x); put(c.zf.y); put(c.zfm);
        put(c.Kc.Kc2); put(c.Kc.Kc4); put(c.Kc.Kc6); put(c.Kc.P1); put(c.Kc.P2);
        put((int32_t)c.sz.w); put((int32_t)c.sz.h);
        edge_tracker &et = kf.edges();
        put((int32_t)et.KNum());
        for (int i = 0; i < et.KNum(); i++) {
            const KeyLine &k = et[i];
            put((int32_t)k.p_inx); put(k.m_m.x); put(k.m_m.y); put(k.u_m.x); put(k.u_m.y); put(k.n_m); put(k.score); put(k.c_p.x); put(k.c_p.y);
            put(k.rho); put(k.s_rho); put(k.rho_nr); put(k.s_rho_nr); put(k.rho0); put(k.s_rho0);
            put(k.p_m.x); put(k.p_m.y); put(k.p_m_0.x); put(k.p_m_0.y);
            put((int32_t)k.m_id); put((int32_t)k.m_id_f); put((int32_t)k.m_id_kf); put((int32_t)k.m_num);
            put(k.m_m0.x); put(k.m_m0.y); put(k.n_m0);
            put((int32_t)k.p_id); put((int32_t)k.n_id); put((int32_t)k.net_id); put((int32_t)k.stereo_m_id);
            put(k.stereo_rho); put(k.stereo_s_rho);
        }
    }
    return 0;
}

static int fill(const char *in, int bw, int bh, int iter, double thresh, double mnum, int discard) {
    std::vector<keyframe> list;
    if (int e = load(in, list)) return e;
    put((int32_t)list.size());
    for (keyframe &kf : list) {
        kf.initDepthFiller({bw, bh}, iter, thresh, mnum, depth_filler::BOUND_NONE, discard != 0);
        depth_filler &df = kf.depthFill();
        const Size2D g = df.gridSize();
        const int n = g.w * g.h;
        put((int32_t)g.w); put((int32_t)g.h);
        for (int i = 0; i < n; i++) put((double)df.data[i].rho);
        for (int i = 0; i < n; i++) put((double)df.data[i].s_rho);
        for (int i = 0; i < n; i++) put((uint8_t)(df.data[i].fixed ? 1 : 0));
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "layout")) return layout();
    if (argc == 4 && !strcmp(argv[1], "save")) return save(argv[2], argv[3]);
    if (argc == 3 && !strcmp(argv[1], "load")) return dump(argv[2]);
    if (argc == 9 && !strcmp(argv[1], "fill")) return fill(argv[2], atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atof(argv[6]), atof(argv[7]), atoi(argv[8]));
    return 64;
}
