// ros_edgemap.cpp — see rebvo/ros_edgemap.h (reference: ros/src/rebvo_ros/src/rebvo_nodelet.cpp:176-212).
#include "rebvo/ros_edgemap.h"

namespace rebvo {

void pack_ros_edgemap(const KeyLine *kl, int kn, double K, double zfm, ros_point *out_p, ros_keyline *out_k) {
    for (int j = 0; j < kn; j++) {
        const KeyLine &k = kl[j];
        if (out_k) {
            ros_keyline &m = out_k[j];
            m.KlGrad[0] = k.m_m.x;
            m.KlGrad[1] = k.m_m.y;
            m.KlImgPos[0] = k.c_p.x;
            m.KlImgPos[1] = k.c_p.y;
            m.invDepth = k.rho;
            m.invDepthS = k.s_rho;
            m.KlFocPos[0] = k.p_m.x;
            m.KlFocPos[1] = k.p_m.y;
            m.KlMatchID = k.m_id;
            m.ConsMatch = k.m_num;
            m.KlPrevMatchID = (int16_t)(uint16_t)(uint32_t)k.p_id;   // the low 16 bits, as the nodelet's int -> int16 assignment keeps on x86-64
            m.KlNextMatchID = (int16_t)(uint16_t)(uint32_t)k.n_id;
        }
        if (out_p) {
            // TooN::makeVector(kl.p_m.x, kl.p_m.y, kl.rho / K): a Vector<3, double>; unprojectHomCordVec divides in double, in this order
            const double px = k.p_m.x, py = k.p_m.y, q = k.rho / K;
            out_p[j].x = (float)(px / q / zfm);
            out_p[j].y = (float)(py / q / zfm);
            out_p[j].z = (float)(1.0 / q);
        }
    }
}

}  // namespace rebvo

extern "C" void rebvo_pack_ros_edgemap(const void *keylines, int kn, double K, double zfm, void *out_points, void *out_keylines) {
    rebvo::pack_ros_edgemap((const rebvo::KeyLine *)keylines, kn, K, zfm, (rebvo::ros_point *)out_points, (rebvo::ros_keyline *)out_keylines);
}
