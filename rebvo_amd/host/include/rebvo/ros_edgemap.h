// ros_edgemap.h — what the reference's ROS nodelet builds per KeyLine in its output callback (RebvoNodelet::edgeMapPubCb,
// ros/src/rebvo_ros/src/rebvo_nodelet.cpp:176-212): one xyz float point of the rebvo_pcl cloud and one Keyline.msg record of the EdgeMap
// message.  The packer below is that loop in plain C++, without ROS: the CPU yardstick of the device packer (edgehip_ros_pack).
#ifndef REBVO_AMD_HOST_ROS_EDGEMAP_H
#define REBVO_AMD_HOST_ROS_EDGEMAP_H

#include <cstdint>

#include "rebvo/rebvo.h"

namespace rebvo {

struct ros_point { float x, y, z; };   // one point of a PointCloud2 with the fields "xyz" (:169-174)
#pragma pack(push, 1)
struct ros_keyline {                   // rebvo/Keyline.msg, field for field: the little-endian wire body of one element of Keyline[]
    float KlGrad[2];
    float KlImgPos[2];
    double invDepth;
    double invDepthS;
    float KlFocPos[2];
    int32_t KlMatchID;
    int32_t ConsMatch;
    int16_t KlPrevMatchID;
    int16_t KlNextMatchID;
};
#pragma pack(pop)
static_assert(sizeof(ros_point) == 12, "xyz point layout");
static_assert(sizeof(ros_keyline) == 52, "Keyline.msg wire layout");

// The nodelet's loop over kl[0 .. kn): out_p[j] = cam.unprojectHomCordVec(makeVector(p_m.x, p_m.y, rho / K)) narrowed to float
// (include/UtilLib/cam_model.h:163-169, zfm the camera's), out_k[j] the message's fields (rho NOT divided by K).  Either output may be null.
void pack_ros_edgemap(const KeyLine *kl, int kn, double K, double zfm, ros_point *out_p, ros_keyline *out_k);

}  // namespace rebvo

extern "C" {
/* flat view for non-C++ callers (tests): KeyLine array in the reference's 168-byte layout, 12-byte points and 52-byte records out */
void rebvo_pack_ros_edgemap(const void *keylines, int kn, double K, double zfm, void *out_points, void *out_keylines);
}
#endif
