// rebvo/keyframe.h — the reference's keyframe as plain data (include/mtracklib/keyframe.h:33-116), and its file
// (keyframe::saveKeyframes2File / loadKeyframesFromFile / dumpToBinaryFile, src/mtracklib/keyframe.cpp:73-169; the input of
// app/kf_visualizer).  The reference's keyframe owns an edge_tracker, a global_tracker and a depth_filler; those stay on the device
// here, so this one carries what the file carries: the pose block, the camera, max_r (global_tracker::getMaxSRadius(): what build_field
// was last given, SearchRange) and the KeyLines.
//
// The file, little-endian: int32 kfnum, then per key frame double t, K, Rot[9] row-major, RotLie[3], Vel[3], Pose[9], PoseLie[3], Pos[3]
// (32 doubles), double max_r, the raw 72-byte cam_model, int32 kn, kn x 168-byte KeyLine.  The reference writes whatever its heap holds
// into the padding of each record (bytes 36..39); zeros are written here.  Header only: no device, no library.
#ifndef REBVO_AMD_KEYFRAME_H
#define REBVO_AMD_KEYFRAME_H

#include <cstring>
#include <fstream>
#include <vector>

#include "rebvo/rebvo.h"

namespace rebvo {

static_assert(sizeof(cam_model) == 72, "cam_model must keep the reference layout: the key-frame file holds it raw");

class keyframe {
public:
    double t = 0;
    double K = 1;
    Matrix3x3 Rot = Identity3();
    Vector3 RotLie = Zeros3();
    Vector3 Vel = Zeros3();
    Matrix3x3 Pose = Identity3();
    Vector3 PoseLie = Zeros3();
    Vector3 Pos = Zeros3();
    cam_model camera;
    double max_r = 0;
    std::vector<KeyLine> kl;

    int KNum() const { return (int)kl.size(); }

    void dumpToBinaryFile(std::ofstream &file) const {
        double d[33];
        d[0] = t; d[1] = K;
        for (int i = 0; i < 9; i++) { d[2 + i] = Rot(i / 3, i % 3); d[17 + i] = Pose(i / 3, i % 3); }
        for (int i = 0; i < 3; i++) { d[11 + i] = RotLie[i]; d[14 + i] = Vel[i]; d[26 + i] = PoseLie[i]; d[29 + i] = Pos[i]; }
        d[32] = max_r;
        file.write((const char *)d, sizeof d);
        file.write((const char *)&camera, sizeof camera);
        const int32_t kn = KNum();
        file.write((const char *)&kn, sizeof kn);
        for (const KeyLine &k : kl) {
            char rec[sizeof(KeyLine)];
            std::memcpy(rec, &k, sizeof rec);
            std::memset(rec + 36, 0, 4);   // the one padding hole of the record
            file.write(rec, sizeof rec);
        }
    }
    // false: the file ended early or holds a count that cannot be (nothing of *this is then meaningful)
    bool loadFromBinaryFile(std::ifstream &file) {
        double d[33];
        int32_t kn = 0;
        if (!file.read((char *)d, sizeof d) || !file.read((char *)&camera, sizeof camera) || !file.read((char *)&kn, sizeof kn)) return false;
        if (kn < 0) return false;
        const std::streampos at = file.tellg();
        file.seekg(0, std::ios::end);
        const std::streamoff left = file.tellg() - at;
        file.seekg(at);
        if ((std::streamoff)kn * (std::streamoff)sizeof(KeyLine) > left) return false;   // (before anything of that size is allocated)
        t = d[0]; K = d[1];
        for (int i = 0; i < 9; i++) { Rot(i / 3, i % 3) = d[2 + i]; Pose(i / 3, i % 3) = d[17 + i]; }
        for (int i = 0; i < 3; i++) { RotLie[i] = d[11 + i]; Vel[i] = d[14 + i]; PoseLie[i] = d[26 + i]; Pos[i] = d[29 + i]; }
        max_r = d[32];
        kl.resize(kn);
        if (kn > 0 && !file.read((char *)kl.data(), sizeof(KeyLine) * (size_t)kn)) return false;
        return true;
    }

    static bool saveKeyframes2File(const char *name, std::vector<keyframe> &kf_list) {
        std::ofstream f(name, std::ios::binary);
        if (!f.is_open()) return false;
        const int32_t kfnum = (int32_t)kf_list.size();
        f.write((const char *)&kfnum, sizeof kfnum);
        for (keyframe &kf : kf_list) kf.dumpToBinaryFile(f);
        f.close();
        return !f.fail();
    }
    // Appends to kf_list, as upstream.  false for a file that cannot be opened or ends early: kf_list then holds the key frames that
    // were read whole.
    static bool loadKeyframesFromFile(const char *name, std::vector<keyframe> &kf_list) {
        std::ifstream f(name, std::ios::binary);
        if (!f.is_open()) return false;
        int32_t kfnum = 0;
        if (!f.read((char *)&kfnum, sizeof kfnum) || kfnum < 0) return false;
        for (int i = 0; i < kfnum; i++) {
            keyframe kf;
            if (!kf.loadFromBinaryFile(f)) return false;
            kf_list.push_back(std::move(kf));
        }
        return true;
    }
};

}  // namespace rebvo
#endif
