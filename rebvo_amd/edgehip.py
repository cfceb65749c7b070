"""ctypes binding of libedgehip.so (include/edgehip.h) — the HIP/gfx950 edge pipeline.

This module is only glue: every call goes straight to the C ABI.  There is no CPU fallback; importing
works anywhere (so the CPU test-suite can check the exported symbols) but creating a context needs an
MI355X.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libedgehip.so")

KEYLINE_DTYPE = np.dtype(
    [
        ("p_inx", "<i4"), ("m_m", "<f4", (2,)), ("u_m", "<f4", (2,)), ("n_m", "<f4"), ("score", "<f4"),
        ("c_p", "<f4", (2,)), ("_pad0", "<i4"),
        ("rho", "<f8"), ("s_rho", "<f8"), ("rho_nr", "<f8"), ("s_rho_nr", "<f8"), ("rho0", "<f8"), ("s_rho0", "<f8"),
        ("p_m", "<f4", (2,)), ("p_m_0", "<f4", (2,)),
        ("m_id", "<i4"), ("m_id_f", "<i4"), ("m_id_kf", "<i4"), ("m_num", "<i4"),
        ("m_m0", "<f4", (2,)), ("n_m0", "<f8"),
        ("p_id", "<i4"), ("n_id", "<i4"), ("net_id", "<i4"), ("stereo_m_id", "<i4"),
        ("stereo_rho", "<f8"), ("stereo_s_rho", "<f8"),
    ]
)
assert KEYLINE_DTYPE.itemsize == 168

# edgehip_net_keyline = rebvo::net_keyline (include/CommLib/net_keypoint.h:35-62), packed: 15 bytes
NET_KEYLINE_DTYPE = np.dtype({"names": ["qx", "qy", "rho", "s_rho", "n_kl", "m_num", "flow"],
                              "formats": ["<u2", "<u2", "<u2", "<u2", "<i4", "u1", ("u1", (2,))],
                              "offsets": [0, 2, 4, 6, 8, 12, 13], "itemsize": 15})
assert NET_KEYLINE_DTYPE.itemsize == 15
NET_HEADER_DTYPE = np.dtype([("kline_num", "<i4"), ("km_num", "<i4"), ("k", "<f4")])   # edgehip_net_header
# edgehip_compressed_kl = rebvo::compressed_kl (include/CommLib/edgemap_com.h:45-51), packed: 5 bytes
COMPRESSED_KL_DTYPE = np.dtype({"names": ["x", "y", "rho", "s_rho"], "formats": ["u1", "u1", "<i2", "u1"], "offsets": [0, 1, 2, 4], "itemsize": 5})
EDGEMAP_BAD_LINK, EDGEMAP_OVERFLOW, EDGEMAP_STEP_GUARD = 1, 2, 4   # status bits of edgehip_download_edgemap
EDGEMAP_SEGMENT_OVERFLOW, EDGEMAP_ITEM_OVERFLOW = 1, 2             # status bits of edgehip_download_edgemap_segments
# edgehip_ros_point / edgehip_ros_keyline: what the ROS nodelet builds per KeyLine (ros/src/rebvo_ros/src/rebvo_nodelet.cpp:176-212):
# one xyz point of the cloud, one rebvo/Keyline.msg record (its little-endian wire body, packed: 52 bytes)
ROS_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
ROS_KEYLINE_DTYPE = np.dtype({"names": ["KlGrad", "KlImgPos", "invDepth", "invDepthS", "KlFocPos", "KlMatchID", "ConsMatch",
                                        "KlPrevMatchID", "KlNextMatchID"],
                              "formats": [("<f4", 2), ("<f4", 2), "<f8", "<f8", ("<f4", 2), "<i4", "<i4", "<i2", "<i2"],
                              "offsets": [0, 8, 16, 24, 32, 40, 44, 48, 50], "itemsize": 52})
assert ROS_POINT_DTYPE.itemsize == 12 and ROS_KEYLINE_DTYPE.itemsize == 52
ROS_POINTS, ROS_KEYLINES = 1, 2   # EDGEHIP_ROS_POINTS, EDGEHIP_ROS_KEYLINES


class Params(C.Structure):
    _fields_ = [
        ("w", C.c_int32), ("h", C.c_int32),
        ("ppx", C.c_double), ("ppy", C.c_double), ("zfx", C.c_double), ("zfy", C.c_double),
        ("kc", C.c_double * 5),
        ("sigma0", C.c_double), ("ksigma", C.c_double),
        ("plane_fit_size", C.c_int32),
        ("pos_neg_thresh", C.c_double), ("dog_thresh", C.c_double),
        ("max_points", C.c_int32), ("reference_points", C.c_int32), ("track_points", C.c_int32),
        ("detector_thresh", C.c_double), ("auto_gain", C.c_double),
        ("max_thresh", C.c_double), ("min_thresh", C.c_double),
        ("search_range", C.c_int32), ("qcut_nbins", C.c_int32),
        ("qcut_quantile", C.c_double),
        ("tracker_iter_num", C.c_int32), ("tracker_init_type", C.c_int32), ("tracker_init_iter_num", C.c_int32),
        ("tracker_match_thresh", C.c_double), ("match_thresh_module", C.c_double), ("match_thresh_angle", C.c_double),
        ("match_num_thresh", C.c_uint32), ("do_rescaling", C.c_int32),
        ("reweight_distance", C.c_double), ("regularize_thresh", C.c_double),
        ("loc_unc_match", C.c_double), ("reshape_q_abs", C.c_double), ("reshape_q_rel", C.c_double),
        ("loc_unc", C.c_double),
        ("global_match_threshold", C.c_int32), ("debug_planes", C.c_int32),
        ("config_fps", C.c_double),
        ("use_undistort", C.c_int32), ("stereo_available", C.c_int32),
    ]


def euroc_params(w=752, h=480, **over):
    """app/rebvorun/GlobalConfig_EuRoC of the reference (+ TrackPoints=12000, ImuMode=0)."""
    p = Params()
    p.w, p.h = w, h
    sx, sy = w / 752.0, h / 480.0
    p.ppx, p.ppy, p.zfx, p.zfy = 367.215 * sx, 248.375 * sy, 458.654 * sx, 457.296 * sy
    p.kc[:] = [-0.28340811, 0.07395907, 0.0, 0.00019359, 1.76187114e-05]
    p.sigma0, p.ksigma = 1.7818, 1.2599
    p.plane_fit_size = 2
    p.pos_neg_thresh, p.dog_thresh = 0.4, 0.095259868922420
    p.max_points, p.reference_points, p.track_points = 16000, 12000, 12000
    p.detector_thresh, p.auto_gain, p.max_thresh, p.min_thresh = 0.01, 5e-7, 0.5, 0.005
    p.search_range, p.qcut_nbins, p.qcut_quantile = 40, 100, 0.9
    p.tracker_iter_num, p.tracker_init_type, p.tracker_init_iter_num = 5, 2, 2
    p.tracker_match_thresh, p.match_thresh_module, p.match_thresh_angle = 0.5, 1.0, 45.0
    p.match_num_thresh, p.do_rescaling = 0, 0
    p.reweight_distance, p.regularize_thresh = 2.0, 0.5
    p.loc_unc_match, p.reshape_q_abs, p.reshape_q_rel, p.loc_unc = 2.0, 1e-4, 1.6968e-04, 1.0
    p.global_match_threshold = 500
    p.debug_planes = 0
    p.config_fps = 20.0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def tum_params(w=640, h=480, **over):
    """app/rebvorun/GlobalConfig_desk.txt of the reference (TUM fr2/desk, ImuMode=0): BASELINE config 4.
    The shipped file has Kc=0/UseUndistort=0; config 4 exercises the undistorter, so callers pass
    use_undistort=1 and a distortion (the EuRoC coefficients by default, SURVEY.md section 8d scene S3)."""
    p = euroc_params(w, h)
    sx, sy = w / 640.0, h / 480.0
    p.ppx, p.ppy, p.zfx, p.zfy = 320.0 * sx, 240.0 * sy, 525.0 * sx, 525.0 * sy
    p.max_points, p.reference_points, p.track_points = 25000, 15000, 12000
    p.detector_thresh, p.auto_gain, p.max_thresh, p.min_thresh = 0.01, 1e-6, 0.05, 0.03
    p.search_range = 20
    p.tracker_iter_num, p.tracker_init_type, p.tracker_init_iter_num = 10, 2, 2
    p.tracker_match_thresh = 1.0
    p.match_num_thresh = 4
    p.reshape_q_rel = 1e-2
    p.config_fps = 50.0
    for k, v in over.items():
        setattr(p, k, v)
    return p

class SeqState(C.Structure):
    _fields_ = [
        ("tresh", C.c_double),
        ("V", C.c_double * 3), ("W", C.c_double * 3),
        ("P_V", C.c_double * 9), ("P_W", C.c_double * 9),
        ("R", C.c_double * 9),
        ("Pose", C.c_double * 9), ("Pos", C.c_double * 3),
        ("Kp", C.c_double), ("P_Kp", C.c_double), ("K", C.c_double),
        ("s_rho_q", C.c_double),
        ("score", C.c_double), ("rel_error", C.c_double), ("rel_error_score", C.c_double),
        ("t_prev", C.c_double), ("dt", C.c_double),
        ("retuned_thresh", C.c_float),
        ("l_kl_num", C.c_int32), ("frame", C.c_int32),
        ("klm_fwd", C.c_int32), ("klm_num", C.c_int32), ("kf_matchs", C.c_int32),
        ("estimation_ok", C.c_int32), ("minimizer_evals", C.c_int32),
    ]


class Nav(C.Structure):
    _fields_ = [
        ("t", C.c_double), ("dt", C.c_double),
        ("V", C.c_double * 3), ("W", C.c_double * 3), ("P_V", C.c_double * 9), ("P_W", C.c_double * 9),
        ("Rot", C.c_double * 9), ("RotLie", C.c_double * 3), ("Vel", C.c_double * 3),
        ("Pose", C.c_double * 9), ("PoseLie", C.c_double * 3), ("Pos", C.c_double * 3),
        ("Kp", C.c_double), ("RKp", C.c_double), ("s_rho_q", C.c_double), ("tresh", C.c_double),
        ("score", C.c_double), ("rel_error", C.c_double), ("rel_error_score", C.c_double),
        ("retuned_thresh", C.c_float),
        ("kn", C.c_int32), ("klm_fwd", C.c_int32), ("klm_num", C.c_int32), ("kf_matchs", C.c_int32),
        ("estimation_ok", C.c_int32), ("frame", C.c_int32), ("minimizer_evals", C.c_int32),
    ]


class KfRequest(C.Structure):
    """edgehip_kf_request (include/edgehip.h)."""
    _fields_ = [("X0", C.c_double * 6), ("Kr", C.c_double), ("max_s_rho", C.c_double)]


class KfResult(C.Structure):
    """edgehip_kf_result (include/edgehip.h)."""
    _fields_ = [("X", C.c_double * 6), ("RRV", C.c_double * 36), ("score_ratio", C.c_double), ("F", C.c_double), ("F0", C.c_double),
                ("evals", C.c_int32), ("mnum", C.c_int32)]


class ImuParams(C.Structure):
    """edgehip_imu_params; defaults = the &IMU section of app/rebvorun/GlobalConfig_EuRoC."""
    _fields_ = [("giro_meas_std", C.c_double), ("giro_bias_std", C.c_double), ("init_bias", C.c_int32),
                ("init_bias_frame_num", C.c_int32), ("bias_init_guess", C.c_double * 3), ("acel_meas_std", C.c_double),
                ("g_module", C.c_double), ("g_module_uncer", C.c_double), ("g_uncert", C.c_double), ("vbias_std", C.c_double),
                ("scale_std_mult", C.c_double), ("scale_std_max", C.c_double), ("scale_std_init", C.c_double)]


def euroc_imu_params(**over):
    p = ImuParams()
    p.giro_meas_std, p.giro_bias_std = 1.6968e-04, 1.9393e-05
    p.init_bias, p.init_bias_frame_num = 1, 10
    p.bias_init_guess[:] = [0.0188, 0.0037, 0.0776]
    p.acel_meas_std, p.g_module, p.g_module_uncer, p.g_uncert, p.vbias_std = 2.0e-3, 9.8, 0.2e3, 2e-3, 1e-7
    p.scale_std_mult, p.scale_std_max, p.scale_std_init = 1e-2, 1e-4, 1.2e-3
    for k, v in over.items():
        if k == "bias_init_guess":
            p.bias_init_guess[:] = v
        else:
            setattr(p, k, v)
    return p


class ImuIntegrated(C.Structure):
    """edgehip_imu_integrated = rebvo::IntegratedImuData."""
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32), ("dt", C.c_double), ("Rot", C.c_double * 9), ("giro", C.c_double * 3),
                ("acel", C.c_double * 3), ("comp", C.c_double * 3), ("dgiro", C.c_double * 3), ("cacel", C.c_double * 3)]

    @classmethod
    def from_row(cls, r):
        """row = [n, dt, Rot(9), giro(3), acel(3), comp(3), dgiro(3), cacel(3)] (oracle.ImuIntegrated.as_row)"""
        o = cls()
        o.n, o.dt = int(r[0]), float(r[1])
        o.Rot[:] = r[2:11]; o.giro[:] = r[11:14]; o.acel[:] = r[14:17]; o.comp[:] = r[17:20]; o.dgiro[:] = r[20:23]; o.cacel[:] = r[23:26]
        return o


class NavImu(C.Structure):
    """edgehip_nav_imu."""
    _fields_ = [("Rot", C.c_double * 9), ("RotLie", C.c_double * 3), ("RotGiro", C.c_double * 3), ("Vel", C.c_double * 3),
                ("Pose", C.c_double * 9), ("PoseLie", C.c_double * 3), ("Pos", C.c_double * 3), ("g", C.c_double * 3),
                ("scale", C.c_double), ("dt", C.c_double), ("K", C.c_double), ("Kp", C.c_double), ("RKp", C.c_double),
                ("s_rho_q", C.c_double), ("Vg", C.c_double * 3), ("Bg", C.c_double * 3), ("dVv", C.c_double * 3),
                ("dWv", C.c_double * 3), ("Vgv", C.c_double * 3), ("Vgva", C.c_double * 3), ("Av", C.c_double * 3),
                ("As", C.c_double * 3), ("X", C.c_double * 7), ("b_est", C.c_double * 3), ("u_est", C.c_double * 3),
                ("kn", C.c_int32), ("klm_num", C.c_int32), ("estimation_ok", C.c_int32), ("init", C.c_int32)]


class DepthFillParams(C.Structure):
    """edgehip_depth_fill_params: the &DepthFiller keys (PixelBlockSize, IterNum, ThreshRelRho, ThreshMatchNum) + bound mode, discard."""
    _fields_ = [("block_w", C.c_int32), ("block_h", C.c_int32), ("iter_num", C.c_int32), ("thresh_rel_rho", C.c_double),
                ("thresh_match_num", C.c_int32), ("bound_mode", C.c_int32), ("discard", C.c_int32)]


class DepthSurfaceParams(C.Structure):
    """edgehip_depth_surface_params: per-cell surface on / off, depth image mode (0 off, 1 getImgRho, 2 getImgRhoTriInterp)."""
    _fields_ = [("surface", C.c_int32), ("image_mode", C.c_int32)]


class SurfaceViewsParams(C.Structure):
    """edgehip_surface_views_params: view slots and OcGrid's voxel dimensions."""
    _fields_ = [("capacity", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32)]


class KfPose(C.Structure):
    """edgehip_kf_pose: a key frame's pose block (t, K, Rot, RotLie, Vel, Pose, PoseLie, Pos)."""
    _fields_ = [("t", C.c_double), ("K", C.c_double), ("Rot", C.c_double * 9), ("RotLie", C.c_double * 3), ("Vel", C.c_double * 3),
                ("Pose", C.c_double * 9), ("PoseLie", C.c_double * 3), ("Pos", C.c_double * 3)]


class KfTrack(C.Structure):
    """edgehip_kf_track: the per-frame record of the key-frame tracking."""
    _fields_ = [("fow_m0", C.c_int32), ("fow_m", C.c_int32), ("back_m0", C.c_int32), ("back_m", C.c_int32),
                ("inserted", C.c_int32), ("kf_count", C.c_int32), ("guard", C.c_int32), ("kf_kn", C.c_int32)]


class KfListInfo(C.Structure):
    """edgehip_kf_list_info: the key frames taken, and the ordinals [first, first + held) the list holds."""
    _fields_ = [("kf_count", C.c_int32), ("first", C.c_int32), ("held", C.c_int32), ("overwritten", C.c_int32)]


KF_POSE_DTYPE = np.dtype(KfPose)
KF_TRACK_DTYPE = np.dtype(KfTrack)
KF_LIST_INFO_DTYPE = np.dtype(KfListInfo)


class KfPairCount(C.Structure):
    """edgehip_kf_pair_count: countMatches' two counts, kls_on_fov's, and the KeyLines whose projection was not finite."""
    _fields_ = [("kl_on_fov", C.c_int32), ("kl_match", C.c_int32), ("kls_on_fov", C.c_int32), ("guard", C.c_int32)]


class KfCovisArgs(C.Structure):
    """edgehip_kf_covis_args: build_field's (radius, min_mod) and countMatches' (match_mod, match_ang, rho_tol, max_r)."""
    _fields_ = [("field_radius", C.c_int32), ("field_min_mod", C.c_float), ("match_mod", C.c_float), ("match_ang", C.c_float),
                ("rho_tol", C.c_float), ("max_r", C.c_float)]


KF_PAIR_COUNT_DTYPE = np.dtype(KfPairCount)
assert KF_PAIR_COUNT_DTYPE.itemsize == 16 and C.sizeof(KfCovisArgs) == 24


class KfRelocArgs(C.Structure):
    """edgehip_kf_reloc_args: build_field's (radius, min_mod) and OptimizePosGT's (iter_max, rew_dis, rho_tol)."""
    _fields_ = [("field_radius", C.c_int32), ("field_min_mod", C.c_float), ("iter_max", C.c_int32), ("rew_dis", C.c_double),
                ("rho_tol", C.c_double)]


class KfReloc(C.Structure):
    """edgehip_kf_reloc: Minimizer_RV_KF's X, RRV, F / F0, optimizeScale's Kp, OptimizePosGT's K, Pose, Pos, the links counted, the
    evaluations run, steps accepted and the guard count."""
    _fields_ = [("X", C.c_double * 6), ("RRV", C.c_double * 36), ("score_ratio", C.c_double), ("F", C.c_double), ("F0", C.c_double),
                ("Kp", C.c_double), ("K", C.c_double), ("Pose", C.c_double * 9), ("Pos", C.c_double * 3),
                ("mnum", C.c_int32), ("evals", C.c_int32), ("accepted", C.c_int32), ("guard", C.c_int32)]


KF_RELOC_DTYPE = np.dtype(KfReloc)
assert KF_RELOC_DTYPE.itemsize == 488 and C.sizeof(KfRelocArgs) == 32


class KfConstraintArgs(C.Structure):
    """edgehip_kf_constraint_args: OptimizeRelContraint's etracket_2_keyframe, iter_max and k_huber."""
    _fields_ = [("direction", C.c_int32), ("iter_max", C.c_int32), ("k_huber", C.c_double)]


class KfConstraint(C.Structure):
    """edgehip_kf_constraint: X, W_X, R_X, E/E0 with both terms, optimizeScaleF2KF's pair, match_num of the last evaluation, and the
    evaluations run, steps accepted and guard bits."""
    _fields_ = [("X", C.c_double * 6), ("W_X", C.c_double * 36), ("R_X", C.c_double * 36),
                ("ratio", C.c_double), ("E", C.c_double), ("E0", C.c_double), ("Kp", C.c_double), ("W_Kp", C.c_double),
                ("links", C.c_int32), ("inliers", C.c_int32), ("evals", C.c_int32), ("accepted", C.c_int32), ("guard", C.c_int32),
                ("pad", C.c_int32)]


KF_CONSTRAINT_DTYPE = np.dtype(KfConstraint)
assert KF_CONSTRAINT_DTYPE.itemsize == 688 and C.sizeof(KfConstraintArgs) == 16


class KfDepth(C.Structure):
    """edgehip_kf_depth: links used, guard bits, the kf.K the rewrite used and optimizeScaleBack's two sums."""
    _fields_ = [("count", C.c_int32), ("guard", C.c_int32), ("K", C.c_double), ("rTr", C.c_double), ("rTr0", C.c_double)]


KF_DEPTH_DTYPE = np.dtype(KfDepth)
assert KF_DEPTH_DTYPE.itemsize == 32
class EdgemapParams(C.Structure):
    """edgehip_edgemap_params: compress_edgemap's arguments; x_scaling / y_scaling 0 mean the reference's 0.5 and 1."""
    _fields_ = [("min_line_len", C.c_int32), ("max_line_len", C.c_int32), ("match_n_t", C.c_int32), ("pad", C.c_int32),
                ("max_angle", C.c_double), ("rho_rel_max", C.c_double), ("x_scaling", C.c_double), ("y_scaling", C.c_double)]


assert C.sizeof(EdgemapParams) == 48
NAV_DTYPE = np.dtype(Nav)   # numpy view of edgehip_nav (same offsets as the ctypes struct)
assert NAV_DTYPE.itemsize == C.sizeof(Nav)

# every symbol include/edgehip.h declares (checked by tests/test_abi.py without a GPU)
EXPORTS = [
    "edgehip_create", "edgehip_destroy", "edgehip_last_error", "edgehip_abi_version", "edgehip_sync",
    "edgehip_stream", "edgehip_box_widths", "edgehip_upload_rgb", "edgehip_upload_rgb_device",
    "edgehip_stage_a", "edgehip_get_kn", "edgehip_quantile", "edgehip_build_field", "edgehip_try_velrot",
    "edgehip_download_resid", "edgehip_minimizer_rv", "edgehip_forward_match", "edgehip_rotate_keylines",
    "edgehip_directed_matching", "edgehip_regularize_ekf", "edgehip_rescale", "edgehip_process_frame",
    "edgehip_next_slot", "edgehip_cur_slot", "edgehip_read_nav", "edgehip_reset", "edgehip_get_state",
    "edgehip_set_state", "edgehip_get_framecount", "edgehip_set_framecount", "edgehip_download_keylines", "edgehip_download_keylines_batch",
    "edgehip_upload_keylines", "edgehip_download_plane", "edgehip_download_field", "edgehip_profile_enable",
    "edgehip_profile_count", "edgehip_profile_name", "edgehip_profile_read", "edgehip_profile_select",
    "edgehip_upload_rgb_indexed", "edgehip_bind_rgb_indexed", "edgehip_set_nav_log", "edgehip_read_nav_log", "edgehip_read_nav_log_device", "edgehip_read_nav_imu_log", "edgehip_read_stereo_matches_log", "edgehip_set_tracker_precision", "edgehip_export_keylines", "edgehip_export_fetch", "edgehip_export_wait",
    "edgehip_build_undistort_map", "edgehip_download_undistorted", "edgehip_depth_reset", "edgehip_depth_reset_slot", "edgehip_set_slot_camera", "edgehip_directed_matching_stereo",
    "edgehip_alloc_pinned", "edgehip_free_pinned", "edgehip_upload_rgb_pinned", "edgehip_upload_sync", "edgehip_upload_wait", "edgehip_register_host", "edgehip_unregister_host", "edgehip_experiments", "edgehip_fuse_stereo_depth", "edgehip_set_stereo_rig", "edgehip_get_stereo_matches", "edgehip_minimizer_v", "edgehip_ext_rot_vel",
    "edgehip_imu_enable", "edgehip_set_imu", "edgehip_read_nav_imu", "edgehip_minimizer_rv_kf", "edgehip_lm_solve",
    "edgehip_upload_grey8", "edgehip_upload_grey8_pinned", "edgehip_bind_grey8_indexed",
    "edgehip_depth_fill_enable", "edgehip_depth_fill_size", "edgehip_depth_fill", "edgehip_download_depth_grid",
    "edgehip_download_depth_grids_batch",
    "edgehip_depth_surface_enable", "edgehip_depth_surface", "edgehip_download_depth_surface", "edgehip_download_depth_surfaces_batch",
    "edgehip_download_depth_image", "edgehip_download_depth_images_batch", "edgehip_depth_image_device",
    "edgehip_surface_views_enable", "edgehip_surface_view_capture", "edgehip_surface_view_upload", "edgehip_surface_view_clear",
    "edgehip_surface_space", "edgehip_surface_integrate", "edgehip_download_surface_visibility",
    "edgehip_download_surface_visibilities_batch", "edgehip_surface_ray_cross",
    "edgehip_net_enable", "edgehip_net_pack", "edgehip_download_net_keylines", "edgehip_download_net_keylines_batch",
    "edgehip_net_keylines_device", "edgehip_upload_net_keylines", "edgehip_depth_fill_net",
    "edgehip_edgemap_enable", "edgehip_edgemap_compress", "edgehip_download_edgemap", "edgehip_download_edgemap_batch",
    "edgehip_edgemap_device", "edgehip_edgemap_ms", "edgehip_edgemap_export", "edgehip_edgemap_export_fetch", "edgehip_edgemap_export_wait",
    "edgehip_upload_edgemap", "edgehip_edgemap_decode_enable", "edgehip_edgemap_decode", "edgehip_download_edgemap_segments",
    "edgehip_download_edgemap_segments_batch", "edgehip_edgemap_hide_visible", "edgehip_depth_fill_segments", "edgehip_edgemap_decode_ms",
    "edgehip_ros_enable", "edgehip_ros_pack", "edgehip_download_ros_edgemap", "edgehip_download_ros_edgemaps_batch",
    "edgehip_ros_edgemap_device", "edgehip_ros_edgemap_from_device", "edgehip_ros_export", "edgehip_ros_export_fetch", "edgehip_ros_export_wait",
    "edgehip_match_one_pass",
    "edgehip_keyframe_track_enable", "edgehip_keyframe_insert", "edgehip_keyframe_build_forward_match", "edgehip_keyframe_forward_correct",
    "edgehip_keyframe_back_correct", "edgehip_read_keyframe_track", "edgehip_download_keyframe", "edgehip_upload_keyframe",
    "edgehip_keyframe_set_save", "edgehip_keyframe_list_enable", "edgehip_keyframe_list_info", "edgehip_download_keyframe_list",
    "edgehip_download_keyframe_list_batch", "edgehip_keyframe_list_restore",
    "edgehip_keyframe_covisibility", "edgehip_keyframe_covisibility_slot", "edgehip_keyframe_covisibility_ms",
    "edgehip_keyframe_relocalize", "edgehip_keyframe_relocalize_links", "edgehip_keyframe_relocalize_ms",
    "edgehip_keyframe_constraint", "edgehip_keyframe_mutual_exclusion", "edgehip_keyframe_constraint_ms",
    "edgehip_keyframe_map_depth", "edgehip_keyframe_translate_depth", "edgehip_keyframe_list_translate_depth", "edgehip_keyframe_depth_ms",
    "edgehip_keyframe_depth_select",
    "edgehip_jpeg_bound", "edgehip_jpeg_enable", "edgehip_jpeg_encode", "edgehip_jpeg_select", "edgehip_download_jpeg",
    "edgehip_download_jpeg_batch", "edgehip_jpeg_device", "edgehip_jpeg_encode_images",
    "edgehip_jpeg_export", "edgehip_jpeg_export_sizes", "edgehip_jpeg_export_fetch", "edgehip_jpeg_export_wait",
    "edgehip_jpeg_probe", "edgehip_jpeg_decode_enable", "edgehip_upload_jpeg", "edgehip_read_jpeg_decode_status",
    "edgehip_jpeg_decode_images", "edgehip_download_frame", "edgehip_jpeg_decode_ms",
]
FRAME_RGB24, FRAME_GREY8 = 0, 1
JPEG_REASON_WALK = 100   # edgehip_jpeg_decode_images: reason 100 + s, the entropy walk ended with status s
JPEG_INFO_DTYPE = np.dtype([("w", "<i4"), ("h", "<i4"), ("components", "<i4"), ("hsamp", "<i4"), ("vsamp", "<i4"), ("restart_interval", "<i4"),
                            ("entropy_offset", "<u4"), ("entropy_length", "<u4"), ("reason", "<i4")])

_lib = None


def load_library():
    """dlopen libedgehip.so; raises if the HIP extension was not built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C rebvo_amd/csrc` "
                               "(or __graft_entry__.build()); rebvo_amd has no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _lib.edgehip_last_error.restype = C.c_char_p
        _lib.edgehip_profile_name.restype = C.c_char_p
        _lib.edgehip_stream.restype = C.c_void_p
        _lib.edgehip_jpeg_bound.restype = C.c_uint64
    return _lib


class EdgeHipError(RuntimeError):
    pass


def build_undistort_map(params):
    """Host-only: the bilinear undistortion map edgehip_create() builds for `params`, in the reference's
    undistMapPoint form -> (inx[h*w,4] with -1 beyond num, iw[h*w,4])."""
    lib = load_library()
    n = params.w * params.h
    inx, iw = np.empty((n, 4), np.int32), np.empty((n, 4), np.int32)
    rc = lib.edgehip_build_undistort_map(C.byref(params), C.c_void_p(inx.ctypes.data), C.c_void_p(iw.ctypes.data))
    if rc != 0:
        raise EdgeHipError(f"edgehip_build_undistort_map: {rc}")
    return inx, iw


def jpeg_bound(w, h, comment_len=0):
    """edgehip_jpeg_bound: no JPEG stream of a w x h frame is longer (host only)."""
    return int(load_library().edgehip_jpeg_bound(int(w), int(h), C.c_uint32(int(comment_len))))


def jpeg_probe(stream):
    """edgehip_jpeg_probe: the stream's header as a dict (w, h, components, hsamp, vsamp, restart_interval, entropy_offset,
    entropy_length, reason; reason 0: decodable on the device).  Host only."""
    buf = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream, np.uint8)
    info = np.zeros((), JPEG_INFO_DTYPE)
    rc = load_library().edgehip_jpeg_probe(C.c_void_p(buf.ctypes.data if buf.size else None), C.c_size_t(buf.size), C.c_void_p(info.ctypes.data))
    if rc != 0:
        raise EdgeHipError(f"edgehip_jpeg_probe: {rc}")
    return {k: int(info[k]) for k in JPEG_INFO_DTYPE.names}


def _stream_args(streams):
    """[bytes-like] -> (arrays kept alive, uint8 *data[count], size_t len[count])"""
    keep = [np.ascontiguousarray(np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b, np.uint8) for b in streams]
    data = (C.c_void_p * len(keep))(*[a.ctypes.data if a.size else None for a in keep])
    size = (C.c_size_t * len(keep))(*[a.size for a in keep])
    return keep, data, size


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ---- the reference's key-frame file (keyframe::saveKeyframes2File / loadKeyframesFromFile; no GPU, no library) ----
# int32 kfnum, then per key frame: the pose block (t, K, Rot[9] row-major, RotLie[3], Vel[3], Pose[9], PoseLie[3], Pos[3]: 32 doubles),
# double max_r (what build_field was last given: SearchRange), the raw cam_model (72 B), int32 kn, kn 168-byte KeyLine records.
KF_FILE_CAM_DTYPE = np.dtype([("pp", "<f4", (2,)), ("zf", "<f4", (2,)), ("zfm", "<f8"), ("Kc", "<f8", (5,)), ("w", "<i4"), ("h", "<i4")])
assert KF_FILE_CAM_DTYPE.itemsize == 72 and KF_POSE_DTYPE.itemsize == 256


def keyframe_file_camera(params):
    """The cam_model the reference builds from the configuration: pp, zf narrowed to float, zfm = (zf.x + zf.y) / 2 computed in float."""
    cam = np.zeros((), KF_FILE_CAM_DTYPE)
    cam["pp"] = (params.ppx, params.ppy)
    cam["zf"] = (params.zfx, params.zfy)
    cam["zfm"] = np.float32((cam["zf"][0] + cam["zf"][1]) / np.float32(2))
    cam["Kc"] = list(params.kc)
    cam["w"], cam["h"] = params.w, params.h
    return cam


def write_keyframe_file(path, keyframes, params, max_r=None):
    """keyframes: a sequence of (KfPose, KeyLine records) pairs, oldest first; params: the Params the camera and max_r (SearchRange, unless
    given) come from.  Writes the records as they are, so bytes 36..39 of each are whatever the array holds (zero from the device)."""
    cam = keyframe_file_camera(params)
    max_r = float(params.search_range if max_r is None else max_r)
    with open(path, "wb") as f:
        f.write(np.int32(len(keyframes)).tobytes())
        for pose, kl in keyframes:
            kl = np.ascontiguousarray(kl, dtype=KEYLINE_DTYPE)
            f.write(bytes(pose))
            f.write(np.float64(max_r).tobytes())
            f.write(cam.tobytes())
            f.write(np.int32(len(kl)).tobytes())
            f.write(kl.tobytes())


def read_keyframe_file(path):
    """-> a list of dicts (pose: KfPose, max_r, camera: KF_FILE_CAM_DTYPE scalar, kl: KeyLine records).  ValueError for a file that ends
    early or holds a negative count."""
    with open(path, "rb") as f:
        data = f.read()
    at = 0

    def take(n, what):
        nonlocal at
        if n < 0 or at + n > len(data):
            raise ValueError(f"{path}: truncated key-frame file ({what} at byte {at})")
        at += n
        return data[at - n:at]

    kfnum = int(np.frombuffer(take(4, "kfnum"), "<i4")[0])
    if kfnum < 0:
        raise ValueError(f"{path}: negative key-frame count")
    out = []
    for i in range(kfnum):
        pose = KfPose.from_buffer_copy(take(256, f"pose block {i}"))
        max_r = float(np.frombuffer(take(8, f"max_r {i}"), "<f8")[0])
        cam = np.frombuffer(take(72, f"camera {i}"), KF_FILE_CAM_DTYPE)[0].copy()
        kn = int(np.frombuffer(take(4, f"kn {i}"), "<i4")[0])
        if kn < 0:
            raise ValueError(f"{path}: negative KeyLine count in key frame {i}")
        kl = np.frombuffer(take(kn * KEYLINE_DTYPE.itemsize, f"records {i}"), KEYLINE_DTYPE).copy()
        out.append(dict(pose=pose, max_r=max_r, camera=cam, kl=kl))
    return out


class EdgeHip:
    """nseq image sequences advancing in lock-step on one MI355X."""

    def __init__(self, params, nseq=1, nslots=3, device=0):
        self.lib = load_library()
        self.p, self.nseq, self.nslots = params, nseq, nslots
        self.w, self.h, self.cap = params.w, params.h, min(params.max_points, 50000)
        self.ros_what = 0   # the stores edgehip_ros_enable has switched on through this wrapper
        self.device = device
        self.jpeg_cap = 0   # edgehip_jpeg_enable's cap_bytes
        self.ctx = C.c_void_p()
        self._ck(self.lib.edgehip_create(C.byref(params), nseq, nslots, device, C.byref(self.ctx)))

    def _ck(self, rc):
        if rc != 0:
            raise EdgeHipError(f"edgehip error {rc}: {self.lib.edgehip_last_error().decode()}")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.edgehip_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def minimizer_v(self, slot_new, slot_old, V, s_rho_min, min_mod, match_thresh, iter_max, match_num_thresh, reweight_distance):
        """global_tracker::Minimizer_V<double> for every sequence -> (V[nseq,3], RVel[nseq,3,3], F[nseq])."""
        V = np.ascontiguousarray(np.broadcast_to(np.asarray(V, np.float64), (self.nseq, 3))).copy()
        smin = np.ascontiguousarray(np.broadcast_to(np.asarray(s_rho_min, np.float64), (self.nseq,))).copy()
        RV, F = np.zeros((self.nseq, 3, 3)), np.zeros(self.nseq)
        self._ck(self.lib.edgehip_minimizer_v(self.ctx, slot_new, slot_old, _dp(V), _dp(smin), C.c_float(min_mod), C.c_double(match_thresh),
                                              iter_max, C.c_uint32(match_num_thresh), C.c_double(reweight_distance), _dp(RV), _dp(F)))
        return V, RV, F

    def minimizer_rv_kf(self, slot_kf, slot_cur, X0, Kr, max_s_rho, match_mod, match_ang, rho_tol, iter_max, reweight_distance,
                        match_num_thresh):
        """kfvo::Minimizer_RV_KF<double,false> for every sequence: the KeyLines of slot_cur against the field of slot_kf's
        KeyLines -> dict(X[nseq,6], RRV[nseq,6,6], score_ratio, F, F0, evals, mnum)."""
        req = (KfRequest * self.nseq)()
        X0 = np.broadcast_to(np.asarray(X0, np.float64), (self.nseq, 6))
        Kr = np.broadcast_to(np.asarray(Kr, np.float64), (self.nseq,))
        ms = np.broadcast_to(np.asarray(max_s_rho, np.float64), (self.nseq,))
        for s in range(self.nseq):
            req[s].X0[:] = list(X0[s])
            req[s].Kr, req[s].max_s_rho = float(Kr[s]), float(ms[s])
        res = (KfResult * self.nseq)()
        self._ck(self.lib.edgehip_minimizer_rv_kf(self.ctx, slot_kf, slot_cur, req, C.c_double(match_mod), C.c_double(match_ang),
                                                  C.c_double(rho_tol), iter_max, C.c_double(reweight_distance),
                                                  C.c_uint32(match_num_thresh), res))
        return dict(X=np.array([list(r.X) for r in res]), RRV=np.array([list(r.RRV) for r in res]).reshape(self.nseq, 6, 6),
                    score_ratio=np.array([r.score_ratio for r in res]), F=np.array([r.F for r in res]), F0=np.array([r.F0 for r in res]),
                    evals=np.array([r.evals for r in res]), mnum=np.array([r.mnum for r in res]))

    def ext_rot_vel(self, slot, vel, loc_unc, hub_reweight):
        """edge_tracker::ExtRotVel for every sequence -> (X[nseq,6], Wx[nseq,6,6], Rx[nseq,6,6], ok[nseq])."""
        vel = np.ascontiguousarray(np.broadcast_to(np.asarray(vel, np.float64), (self.nseq, 3))).copy()
        X, Wx, Rx = np.zeros((self.nseq, 6)), np.zeros((self.nseq, 6, 6)), np.zeros((self.nseq, 6, 6))
        ok = np.zeros(self.nseq, np.int32)
        self._ck(self.lib.edgehip_ext_rot_vel(self.ctx, slot, _dp(vel), C.c_double(loc_unc), C.c_double(hub_reweight), _dp(X), _dp(Wx),
                                              _dp(Rx), C.c_void_p(ok.ctypes.data)))
        return X, Wx, Rx, ok

    def depth_reset(self, seq=-1):
        """REBVO::Reset() (rebvo_second_t.cpp:609-620) for one sequence or all (-1)."""
        self._ck(self.lib.edgehip_depth_reset(self.ctx, seq))

    def depth_reset_slot(self, slot, seq=-1):
        self._ck(self.lib.edgehip_depth_reset_slot(self.ctx, seq, slot))

    def set_slot_camera(self, slot, ppx, ppy, zfx, zfy):
        self._ck(self.lib.edgehip_set_slot_camera(self.ctx, slot, C.c_double(ppx), C.c_double(ppy), C.c_double(zfx), C.c_double(zfy)))

    def directed_matching_stereo(self, slot, slot_pair, t, R, min_thr_mod, min_thr_ang, max_radius, loc_unc, q_abs, q_rel, loc_unc_model):
        """edge_tracker::directed_matching_stereo for every sequence -> nmatch[nseq]."""
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        nm = np.zeros(self.nseq, np.int32)
        self._ck(self.lib.edgehip_directed_matching_stereo(self.ctx, slot, slot_pair, _dp(t), _dp(R), C.c_double(min_thr_mod),
                                                           C.c_double(min_thr_ang), C.c_double(max_radius), C.c_double(loc_unc),
                                                           C.c_double(q_abs), C.c_double(q_rel), C.c_double(loc_unc_model),
                                                           C.c_void_p(nm.ctypes.data)))
        return nm

    def fuse_stereo_depth(self, slot):
        self._ck(self.lib.edgehip_fuse_stereo_depth(self.ctx, slot))

    def set_stereo_rig(self, slot_pair, t=None, R=None, max_radius=100.0):
        if slot_pair < 0:
            self._ck(self.lib.edgehip_set_stereo_rig(self.ctx, -1, None, None, C.c_double(0)))
            return
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        self._ck(self.lib.edgehip_set_stereo_rig(self.ctx, slot_pair, _dp(t), _dp(R), C.c_double(max_radius)))

    def get_stereo_matches(self):
        nm = np.zeros(self.nseq, np.int32)
        self._ck(self.lib.edgehip_get_stereo_matches(self.ctx, C.c_void_p(nm.ctypes.data)))
        return nm

    def download_undistorted(self, seq, slot):
        out = np.empty((self.h, self.w, 3), np.uint8)
        self._ck(self.lib.edgehip_download_undistorted(self.ctx, seq, slot, C.c_void_p(out.ctypes.data)))
        return out

    # ---- input ----
    def upload_rgb(self, slot, rgb, seq_first=0):
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim == 3:
            rgb = rgb[None]
        assert rgb.shape[1:] == (self.h, self.w, 3)
        self._ck(self.lib.edgehip_upload_rgb(self.ctx, slot, rgb.ctypes.data_as(C.c_void_p), seq_first, rgb.shape[0]))

    def upload_grey8(self, slot, grey, seq_first=0):
        """8-bit mono frames [count][h][w] (or one [h][w]): a third of the bytes of upload_rgb, identical results."""
        grey = np.ascontiguousarray(grey, dtype=np.uint8)
        if grey.ndim == 2:
            grey = grey[None]
        assert grey.shape[1:] == (self.h, self.w)
        self._ck(self.lib.edgehip_upload_grey8(self.ctx, slot, grey.ctypes.data_as(C.c_void_p), seq_first, grey.shape[0]))

    def upload_grey8_pinned(self, slot, ptr, seq_first=0, count=None):
        self._ck(self.lib.edgehip_upload_grey8_pinned(self.ctx, slot, ptr, seq_first, self.nseq if count is None else count))

    def bind_grey8_indexed(self, slot, pool_dev_ptr, pool_frames, idx):
        """Stage A of `slot` reads 8-bit mono frame idx[s] of a device pool in place (no copy); the pool needs 16 B of slack."""
        idx = np.ascontiguousarray(idx, np.int32)
        assert idx.shape == (self.nseq,)
        self._ck(self.lib.edgehip_bind_grey8_indexed(self.ctx, slot, C.c_void_p(pool_dev_ptr), pool_frames,
                                                     idx.ctypes.data_as(C.c_void_p)))

    def alloc_pinned_grey8(self, count=None):
        """Page-locked uint8 array [count][h][w] for upload_grey8_pinned (free with free_pinned)."""
        count = self.nseq if count is None else count
        nbytes = count * self.h * self.w
        ptr = C.c_void_p()
        self._ck(self.lib.edgehip_alloc_pinned(C.c_size_t(nbytes), C.byref(ptr)))
        buf = (C.c_uint8 * nbytes).from_address(ptr.value)
        return np.frombuffer(buf, np.uint8).reshape(count, self.h, self.w), ptr

    def upload_rgb_device(self, slot, dev_ptr):
        self._ck(self.lib.edgehip_upload_rgb_device(self.ctx, slot, C.c_void_p(dev_ptr)))

    def bind_rgb_indexed(self, slot, pool_dev_ptr, pool_frames, idx):
        """Stage A of `slot` reads frame idx[s] of a device pool in place (no copy); the pool needs 16 B of slack."""
        idx = np.ascontiguousarray(idx, np.int32)
        assert idx.shape == (self.nseq,)
        self._ck(self.lib.edgehip_bind_rgb_indexed(self.ctx, slot, C.c_void_p(pool_dev_ptr), pool_frames,
                                                   idx.ctypes.data_as(C.c_void_p)))

    def upload_rgb_indexed(self, slot, pool_dev_ptr, pool_frames, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        assert idx.shape == (self.nseq,)
        self._ck(self.lib.edgehip_upload_rgb_indexed(self.ctx, slot, C.c_void_p(pool_dev_ptr), pool_frames,
                                                     idx.ctypes.data_as(C.c_void_p)))

    def set_tracker_precision(self, bits):
        """32: Minimizer_RV<float> / TryVelRot<float> (the reference's USE_NE10 instantiation); 64: the default."""
        self._ck(self.lib.edgehip_set_tracker_precision(self.ctx, bits))

    def set_nav_log(self, length):
        self._ck(self.lib.edgehip_set_nav_log(self.ctx, length))

    def read_nav_log(self, first, count):
        out = (Nav * (count * self.nseq))()
        self._ck(self.lib.edgehip_read_nav_log(self.ctx, first, count, out))
        return [[out[k * self.nseq + s] for s in range(self.nseq)] for k in range(count)]

    def read_nav_log_array(self, first, count):
        """Same records as read_nav_log, as one numpy structured array [count, nseq] (fields = edgehip_nav's): no
        per-record Python objects, for logs of many sequences."""
        out = np.zeros((count, self.nseq), dtype=NAV_DTYPE)
        self._ck(self.lib.edgehip_read_nav_log(self.ctx, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def read_nav_imu_log(self, first, count):
        """The IMU half of the logged records of frames [first, first+count): [count][nseq] NavImu objects."""
        out = (NavImu * (count * self.nseq))()
        self._ck(self.lib.edgehip_read_nav_imu_log(self.ctx, first, count, out))
        return [[out[k * self.nseq + s] for s in range(self.nseq)] for k in range(count)]

    def read_stereo_matches_log(self, first, count):
        """stereo_match_num of the logged frames [first, first+count) (a context with a stereo rig): int32 array [count, nseq]."""
        out = np.zeros((count, self.nseq), dtype=np.int32)
        self._ck(self.lib.edgehip_read_stereo_matches_log(self.ctx, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def read_nav_log_device(self, first, count, out_dev_ptr):
        """Records of frames [first, first+count) as raw edgehip_nav structs into device memory ([count][nseq][NAV_DTYPE.itemsize]
        bytes at out_dev_ptr): what shard.NavMover hands RCCL without a host bounce."""
        self._ck(self.lib.edgehip_read_nav_log_device(self.ctx, first, count, C.c_void_p(out_dev_ptr)))

    def sync(self):
        self._ck(self.lib.edgehip_sync(self.ctx))

    def stream(self):
        return self.lib.edgehip_stream(self.ctx)

    def box_widths(self):
        out = (C.c_int * 6)()
        self._ck(self.lib.edgehip_box_widths(self.ctx, out))
        return list(out)

    # ---- stages ----
    def stage_a(self, slot):
        self._ck(self.lib.edgehip_stage_a(self.ctx, slot))

    def get_kn(self, slot):
        out = np.zeros(self.nseq, np.int32)
        self._ck(self.lib.edgehip_get_kn(self.ctx, slot, out.ctypes.data_as(C.c_void_p)))
        return out

    def quantile(self, slot, smin=1e-3, smax=20.0, pct=0.9, nbins=100):
        self._ck(self.lib.edgehip_quantile(self.ctx, slot, C.c_double(smin), C.c_double(smax), C.c_double(pct), nbins))

    def build_field(self, slot, radius, min_mod=-1.0):
        self._ck(self.lib.edgehip_build_field(self.ctx, slot, radius, C.c_float(min_mod)))

    def try_velrot(self, slot_new, slot_old, X, reweight, procjf, match_thresh, s_rho_min, match_num_thresh, k_huber,
                   resid_in=-1, resid_out=0):
        X = np.ascontiguousarray(np.broadcast_to(np.asarray(X, np.float64), (self.nseq, 6)))
        smin = np.ascontiguousarray(np.broadcast_to(np.asarray(s_rho_min, np.float64), (self.nseq,)))
        out = np.zeros((self.nseq, 43))
        self._ck(self.lib.edgehip_try_velrot(self.ctx, slot_new, slot_old, _dp(X), int(reweight), int(procjf),
                                             C.c_double(match_thresh), _dp(smin), C.c_uint32(match_num_thresh),
                                             C.c_double(k_huber), resid_in, resid_out, _dp(out)))
        return out[:, 42].copy(), out[:, :36].reshape(self.nseq, 6, 6).copy(), out[:, 36:42].copy()

    def download_resid(self, which):
        out = np.zeros((self.nseq, self.cap))
        self._ck(self.lib.edgehip_download_resid(self.ctx, which, _dp(out)))
        return out

    def lm_solve(self, A, b, svd_rule):
        """h = the 6x6 solve of an LM step for every system of A [n, 6, 6], b [n, 6]; svd_rule: the init phase's TooN::SVD<>::backsub."""
        A = np.ascontiguousarray(A, np.float64).reshape(-1, 36)
        b = np.ascontiguousarray(b, np.float64).reshape(-1, 6)
        h = np.zeros_like(b)
        self._ck(self.lib.edgehip_lm_solve(self.ctx, _dp(A), _dp(b), len(A), int(bool(svd_rule)), _dp(h)))
        return h

    def minimizer_rv(self, slot_new, slot_old):
        self._ck(self.lib.edgehip_minimizer_rv(self.ctx, slot_new, slot_old))

    def forward_match(self, slot_old, slot_new):
        self._ck(self.lib.edgehip_forward_match(self.ctx, slot_old, slot_new))

    def rotate_keylines(self, slot, R=None):
        if R is None:
            self._ck(self.lib.edgehip_rotate_keylines(self.ctx, slot, None))
        else:
            R = np.ascontiguousarray(np.broadcast_to(np.asarray(R, np.float64).reshape(-1, 9), (self.nseq, 9)))
            self._ck(self.lib.edgehip_rotate_keylines(self.ctx, slot, _dp(R)))

    def directed_matching(self, slot_new, slot_old):
        self._ck(self.lib.edgehip_directed_matching(self.ctx, slot_new, slot_old))

    def match_one_pass(self, slot_new, slot_old, fill=False):
        """edgehip_match_one_pass (test support only): the one-pass matching of a whole frame on uploaded lists; R0 = exp(state.W)."""
        self._ck(self.lib.edgehip_match_one_pass(self.ctx, slot_new, slot_old, int(bool(fill))))

    def regularize_ekf(self, slot, do_regularize=True, do_ekf=True):
        self._ck(self.lib.edgehip_regularize_ekf(self.ctx, slot, int(do_regularize), int(do_ekf)))

    def rescale(self, slot):
        self._ck(self.lib.edgehip_rescale(self.ctx, slot))

    # ---- whole frame ----
    def next_slot(self):
        return self.lib.edgehip_next_slot(self.ctx)

    def cur_slot(self):
        return self.lib.edgehip_cur_slot(self.ctx)

    def alloc_pinned_frames(self, count=None):
        """Page-locked uint8 array [count][h][w][3] for upload_rgb_pinned (free with free_pinned)."""
        count = self.nseq if count is None else count
        nbytes = count * self.h * self.w * 3
        ptr = C.c_void_p()
        self._ck(self.lib.edgehip_alloc_pinned(C.c_size_t(nbytes), C.byref(ptr)))
        buf = (C.c_uint8 * nbytes).from_address(ptr.value)
        arr = np.frombuffer(buf, np.uint8).reshape(count, self.h, self.w, 3)
        return arr, ptr

    def free_pinned(self, ptr):
        self._ck(self.lib.edgehip_free_pinned(ptr))

    def upload_rgb_pinned(self, slot, ptr, seq_first=0, count=None):
        self._ck(self.lib.edgehip_upload_rgb_pinned(self.ctx, slot, ptr, seq_first, self.nseq if count is None else count))

    def process_frame(self, t):
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.float64), (self.nseq,)))
        self._ck(self.lib.edgehip_process_frame(self.ctx, _dp(t)))

    def read_nav(self):
        nav = (Nav * self.nseq)()
        self._ck(self.lib.edgehip_read_nav(self.ctx, nav))
        return list(nav)

    # ---- IMU branch on the device ----
    def imu_enable(self, imu_params):
        self._ck(self.lib.edgehip_imu_enable(self.ctx, C.byref(imu_params)))

    def set_imu(self, records):
        """records: one ImuIntegrated per sequence, for the interval that ends with the next process_frame."""
        arr = (ImuIntegrated * self.nseq)(*records)
        self._ck(self.lib.edgehip_set_imu(self.ctx, arr))

    def read_nav_imu(self):
        out = (NavImu * self.nseq)()
        self._ck(self.lib.edgehip_read_nav_imu(self.ctx, out))
        return list(out)

    def reset(self):
        self._ck(self.lib.edgehip_reset(self.ctx))

    # ---- state / data ----
    def get_state(self, seq=0):
        s = SeqState()
        self._ck(self.lib.edgehip_get_state(self.ctx, seq, C.byref(s)))
        return s

    def set_state(self, seq, s):
        self._ck(self.lib.edgehip_set_state(self.ctx, seq, C.byref(s)))

    def get_framecount(self, seq, slot):
        v = C.c_uint32(0)
        self._ck(self.lib.edgehip_get_framecount(self.ctx, seq, slot, C.byref(v)))
        return v.value

    def set_framecount(self, seq, slot, fc):
        self._ck(self.lib.edgehip_set_framecount(self.ctx, seq, slot, C.c_uint32(fc)))

    def download_keylines(self, seq, slot, want_mask=True):
        kl = np.zeros(self.cap, KEYLINE_DTYPE)
        mask = np.zeros((self.h, self.w), np.int32) if want_mask else None
        kn = C.c_int32(0)
        self._ck(self.lib.edgehip_download_keylines(self.ctx, seq, slot, kl.ctypes.data_as(C.c_void_p),
                                                    None if mask is None else mask.ctypes.data_as(C.c_void_p),
                                                    C.byref(kn)))
        return kl[:kn.value].copy(), mask

    def download_keylines_batch(self, slot, seqs, registered=()):
        """AoS KeyLine lists of several sequences of one slot, one packing kernel (edgehip_download_keylines_batch).  `registered`:
        positions in `seqs` whose destination is page-locked first (edgehip_register_host: the copy lands in it directly)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        n = len(seqs)
        bufs = [np.zeros(self.cap, KEYLINE_DTYPE) for _ in range(n)]
        for j in registered:
            self._ck(self.lib.edgehip_register_host(C.c_void_p(bufs[j].ctypes.data), C.c_size_t(bufs[j].nbytes)))
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        kn = np.zeros(n, np.int32)
        try:
            self._ck(self.lib.edgehip_download_keylines_batch(self.ctx, slot, n, seqs.ctypes.data_as(C.c_void_p), ptrs, kn.ctypes.data_as(C.c_void_p)))
        finally:
            for j in registered:
                self._ck(self.lib.edgehip_unregister_host(C.c_void_p(bufs[j].ctypes.data)))
        return [b[:k].copy() for b, k in zip(bufs, kn)]

    def export_keylines(self, seqs):
        """edgehip_export_keylines: the OLD slot of the frame processed last, packed in-stream (no synchronisation) -> ticket."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        t = C.c_int(0)
        self._ck(self.lib.edgehip_export_keylines(self.ctx, len(seqs), seqs.ctypes.data_as(C.c_void_p), C.byref(t)))
        return (t.value, len(seqs))

    def export_fetch(self, ticket, kns, registered=True):
        """Enqueue the copies of kns[j] records per list (does not block); returns the destination arrays, valid after export_wait."""
        tid, n = ticket
        kns = np.ascontiguousarray(kns, dtype=np.int32)
        assert len(kns) == n
        bufs = [np.zeros(self.cap, KEYLINE_DTYPE) for _ in range(n)]
        if registered:
            for b in bufs:
                self._ck(self.lib.edgehip_register_host(C.c_void_p(b.ctypes.data), C.c_size_t(b.nbytes)))
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        self._ck(self.lib.edgehip_export_fetch(self.ctx, tid, kns.ctypes.data_as(C.c_void_p), ptrs))
        return {"bufs": bufs, "kns": kns, "registered": registered, "ticket": ticket}

    def export_wait(self, fetched):
        """Block until the ticket's copies have landed; returns the lists."""
        self._ck(self.lib.edgehip_export_wait(self.ctx, fetched["ticket"][0]))
        if fetched["registered"]:
            for b in fetched["bufs"]:
                self._ck(self.lib.edgehip_unregister_host(C.c_void_p(b.ctypes.data)))
        return [b[:k].copy() for b, k in zip(fetched["bufs"], fetched["kns"])]

    def export_drop(self, ticket):
        self._ck(self.lib.edgehip_export_wait(self.ctx, ticket[0]))

    # ---- dense depth fill (depth_filler) ----
    def depth_fill_enable(self, block=10, iter_num=10, thresh_rel_rho=1.0, thresh_match_num=5, bound_mode=0, discard=1, block_h=None):
        """edgehip_depth_fill_enable; block=None frees the grids.  Returns the grid size (gw, gh) or None."""
        if block is None:
            self._ck(self.lib.edgehip_depth_fill_enable(self.ctx, None))
            return None
        p = DepthFillParams(int(block), int(block if block_h is None else block_h), int(iter_num), float(thresh_rel_rho),
                            int(thresh_match_num), int(bound_mode), int(discard))
        self._ck(self.lib.edgehip_depth_fill_enable(self.ctx, C.byref(p)))
        return self.depth_fill_size()

    def depth_fill_size(self):
        gw, gh = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.edgehip_depth_fill_size(self.ctx, C.byref(gw), C.byref(gh)))
        return gw.value, gh.value

    def depth_fill(self, slot):
        """edgehip_depth_fill: the grids of every sequence from the KeyLines of `slot` (in-stream)."""
        self._ck(self.lib.edgehip_depth_fill(self.ctx, int(slot)))

    def download_depth_grid(self, seq):
        """-> (rho, s_rho, fixed) as (gh, gw) arrays (float64, float64, bool)."""
        gw, gh = self.depth_fill_size()
        rho, s_rho, fixed = np.empty((gh, gw)), np.empty((gh, gw)), np.empty((gh, gw), np.uint8)
        self._ck(self.lib.edgehip_download_depth_grid(self.ctx, int(seq), _dp(rho), _dp(s_rho), fixed.ctypes.data_as(C.c_void_p)))
        return rho, s_rho, fixed.astype(bool)

    def download_depth_grids(self, seqs):
        """edgehip_download_depth_grids_batch -> [(rho, s_rho, fixed)] in the order of seqs."""
        gw, gh = self.depth_fill_size()
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        n = len(seqs)
        out = [(np.empty((gh, gw)), np.empty((gh, gw)), np.empty((gh, gw), np.uint8)) for _ in range(n)]
        pr = (C.c_void_p * n)(*[o[0].ctypes.data for o in out])
        ps = (C.c_void_p * n)(*[o[1].ctypes.data for o in out])
        pf = (C.c_void_p * n)(*[o[2].ctypes.data for o in out])
        self._ck(self.lib.edgehip_download_depth_grids_batch(self.ctx, n, seqs.ctypes.data_as(C.c_void_p), pr, ps, pf))
        return [(r, s, f.astype(bool)) for r, s, f in out]

    # ---- the wire-format edge map (net_keyline) and the visualizer's fill from it ----
    def net_enable(self, kl_size):
        """edgehip_net_enable: room for kl_size 15-byte records per sequence; 0 (or None) frees the store."""
        self._ck(self.lib.edgehip_net_enable(self.ctx, int(kl_size or 0)))
        self.net_kl_size = int(kl_size or 0)

    def net_pack(self, slot, slot_pair=-1, k_prof=None):
        """edgehip_net_pack: copy_net_keyline + copy_net_keyline_nextid on the KeyLines of `slot` for every sequence (in-stream).
        k_prof: one scale per sequence (or a scalar), None for each sequence's K."""
        kp = None
        if k_prof is not None:
            kp = np.ascontiguousarray(np.broadcast_to(np.asarray(k_prof, np.float64), (self.nseq,))).copy()
        self._ck(self.lib.edgehip_net_pack(self.ctx, int(slot), int(slot_pair), _dp(kp) if kp is not None else None))

    def net_keylines(self, seq):
        """edgehip_download_net_keylines -> (records, header): a NET_KEYLINE_DTYPE array of header["kline_num"] records and a
        NET_HEADER_DTYPE scalar."""
        rec = np.zeros(self.net_kl_size, NET_KEYLINE_DTYPE)
        hdr = np.zeros(1, NET_HEADER_DTYPE)
        self._ck(self.lib.edgehip_download_net_keylines(self.ctx, int(seq), C.c_void_p(rec.ctypes.data), C.c_void_p(hdr.ctypes.data)))
        return rec[:max(0, min(int(hdr["kline_num"][0]), self.net_kl_size))].copy(), hdr[0]

    def net_keylines_batch(self, seqs):
        """edgehip_download_net_keylines_batch -> [(records, header)] in the order of seqs (one synchronisation)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        n = len(seqs)
        recs = [np.zeros(self.net_kl_size, NET_KEYLINE_DTYPE) for _ in range(n)]
        hdrs = [np.zeros(1, NET_HEADER_DTYPE) for _ in range(n)]
        pr = (C.c_void_p * n)(*[r.ctypes.data for r in recs])
        ph = (C.c_void_p * n)(*[h.ctypes.data for h in hdrs])
        self._ck(self.lib.edgehip_download_net_keylines_batch(self.ctx, n, seqs.ctypes.data_as(C.c_void_p), pr, ph))
        return [(r[:max(0, min(int(h["kline_num"][0]), self.net_kl_size))].copy(), h[0]) for r, h in zip(recs, hdrs)]

    def net_keylines_into(self, records=None, headers=None, first=0):
        """edgehip_net_keylines_device: the whole stores of sequences [first, first + count) into uint8 torch tensors on the context's
        device, records (count, kl_size, 15) and headers (count, 12) (either may be None), device to device."""
        t = records if records is not None else headers
        count = t.shape[0]
        for x, tail in ((records, (self.net_kl_size, 15)), (headers, (NET_HEADER_DTYPE.itemsize,))):
            if x is not None:
                assert x.dtype.itemsize == 1 and x.is_contiguous(), "uint8 contiguous tensors"
                assert tuple(x.shape) == (count,) + tail, (tuple(x.shape), (count,) + tail)
        self._ck(self.lib.edgehip_net_keylines_device(self.ctx, int(first), int(count),
                                                      C.c_void_p(records.data_ptr() if records is not None else None),
                                                      C.c_void_p(headers.data_ptr() if headers is not None else None)))

    def upload_net_keylines(self, seq, records):
        """edgehip_upload_net_keylines: `records` (NET_KEYLINE_DTYPE, or raw uint8 of shape (kn, 15)) become sequence seq's stored records."""
        rec = np.ascontiguousarray(records)
        if rec.dtype != NET_KEYLINE_DTYPE:
            rec = np.ascontiguousarray(rec, np.uint8).reshape(-1, 15)
        self._ck(self.lib.edgehip_upload_net_keylines(self.ctx, int(seq), C.c_void_p(rec.ctypes.data), len(rec)))

    # ---- the compressed edge map: fitted line segments (compress_edgemap) ----
    def edgemap_enable(self, cap_records):
        """edgehip_edgemap_enable: room for cap_records 5-byte records per sequence; 0 (or None) frees the store."""
        self._ck(self.lib.edgehip_edgemap_enable(self.ctx, int(cap_records or 0)))
        self.edgemap_cap = int(cap_records or 0)

    def edgemap_compress(self, slot, params, scale=None):
        """edgehip_edgemap_compress: compress_edgemap on the KeyLines of `slot` for every sequence (in-stream).  params: an EdgemapParams;
        scale: [nseq] or None for 1."""
        sc = None if scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float64), (self.nseq,)))
        self._ck(self.lib.edgehip_edgemap_compress(self.ctx, int(slot), C.byref(params), _dp(sc) if sc is not None else None))

    def download_edgemap(self, seq):
        """edgehip_download_edgemap -> (records: COMPRESSED_KL_DTYPE array of the sequence's count, status bits)."""
        return self.download_edgemaps([seq])[0]

    def download_edgemaps(self, seqs):
        """edgehip_download_edgemap_batch -> [(records, status)] in the order of seqs."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        n = len(seqs)
        recs = [np.zeros(self.edgemap_cap, COMPRESSED_KL_DTYPE) for _ in range(n)]
        counts, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        pr = (C.c_void_p * n)(*[r.ctypes.data for r in recs])
        self._ck(self.lib.edgehip_download_edgemap_batch(self.ctx, n, seqs.ctypes.data_as(C.c_void_p), pr, C.c_void_p(counts.ctypes.data),
                                                         C.c_void_p(status.ctypes.data)))
        return [(recs[j][:counts[j]].copy(), int(status[j])) for j in range(n)]

    def edgemap_into(self, records=None, counts=None, first=0):
        """edgehip_edgemap_device: the stores of sequences [first, first + count) into torch tensors on the context's GPU: records uint8
        (count, cap_records, 5), counts int32 (count,)."""
        count = (records if records is not None else counts).shape[0]
        self._ck(self.lib.edgehip_edgemap_device(self.ctx, int(first), int(count), C.c_void_p(records.data_ptr() if records is not None else None),
                                                 C.c_void_p(counts.data_ptr() if counts is not None else None)))

    def edgemap_ms(self):
        """edgehip_edgemap_ms -> (labelling_ms, sort_ms, walks_ms, placement_ms) of the last edgemap_compress under profile_enable."""
        ms = (C.c_float * 4)()
        self._ck(self.lib.edgehip_edgemap_ms(self.ctx, ms))
        return tuple(ms)

    # ---- the compressed edge map, received: segments, visibility, depth grid (edgemap_com_decoder) ----
    def upload_edgemap(self, seq, records, rho_scale=1.0):
        """edgehip_upload_edgemap: `records` (COMPRESSED_KL_DTYPE, or raw uint8 of shape (n, 5)) and their rho_scale become sequence
        seq's stored edge map."""
        rec = np.ascontiguousarray(records)
        if rec.dtype != COMPRESSED_KL_DTYPE:
            rec = np.ascontiguousarray(rec, np.uint8).reshape(-1, 5)
        self._ck(self.lib.edgehip_upload_edgemap(self.ctx, int(seq), C.c_void_p(rec.ctypes.data if len(rec) else None), len(rec),
                                                 C.c_float(rho_scale)))

    def edgemap_decode_enable(self, cap_segments, cap_items=None):
        """edgehip_edgemap_decode_enable: room for cap_segments segments and cap_items (segment, step) items per sequence.  cap_items
        has no default (a sequence with more steps than cap_items folds nothing); cap_segments 0 (or None) frees the decoder."""
        if cap_segments and cap_items is None:
            raise ValueError("edgemap_decode_enable: cap_items is required (the steps of a sequence's segments, about their length in pixels)")
        self._ck(self.lib.edgehip_edgemap_decode_enable(self.ctx, int(cap_segments or 0), int(cap_items or 0)))
        self.edgemap_cap_segments = int(cap_segments or 0)   # the size of download_edgemap_segments' buffers: the library has no query for it

    def edgemap_decode(self, x_scaling=0.0, y_scaling=0.0):
        """edgehip_edgemap_decode: Decode on every sequence's stored records (in-stream)."""
        self._ck(self.lib.edgehip_edgemap_decode(self.ctx, C.c_double(x_scaling), C.c_double(y_scaling)))

    def download_edgemap_segments(self, seqs):
        """edgehip_download_edgemap_segments(_batch): for a sequence -> (segments (n, 8) float32, flags (n,) uint8, status bits); for a
        list of sequences -> a list of those, in its order."""
        one = np.isscalar(seqs)
        ids = np.ascontiguousarray([seqs] if one else seqs, np.int32)
        cap = getattr(self, "edgemap_cap_segments", 0)
        if not cap:
            raise EdgeHipError("download_edgemap_segments: the decoder is not enabled through edgemap_decode_enable of this object")
        n = len(ids)
        segs = [np.zeros((cap, 8), np.float32) for _ in range(n)]
        flags = [np.zeros(cap, np.uint8) for _ in range(n)]
        ps = (C.c_void_p * n)(*[a.ctypes.data for a in segs])
        pf = (C.c_void_p * n)(*[a.ctypes.data for a in flags])
        counts, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._ck(self.lib.edgehip_download_edgemap_segments_batch(self.ctx, n, ids.ctypes.data_as(C.c_void_p), ps, pf,
                                                                  C.c_void_p(counts.ctypes.data), C.c_void_p(status.ctypes.data)))
        out = [(segs[j][:counts[j]].copy(), flags[j][:counts[j]].copy(), int(status[j])) for j in range(n)]
        return out[0] if one else out

    def edgemap_hide_visible(self, views):
        """edgehip_edgemap_hide_visible: views[seq] is None (the sequence is left alone) or (DPose (3, 3), DPos (3,), k_em, k_new).
        -> s_num per sequence (int32; -1 where left alone)."""
        B = self.nseq
        assert len(views) == B
        keep, pr, pp = [], (C.c_void_p * B)(), (C.c_void_p * B)()
        k_em, k_new = np.ones(B, np.float32), np.ones(B, np.float32)
        for s, v in enumerate(views):
            if v is None:
                continue
            r, p = np.ascontiguousarray(v[0], np.float64).reshape(9), np.ascontiguousarray(v[1], np.float64).reshape(3)
            keep += [r, p]
            pr[s], pp[s] = r.ctypes.data, p.ctypes.data
            k_em[s], k_new[s] = v[2], v[3]
        s_num = np.zeros(B, np.int32)
        self._ck(self.lib.edgehip_edgemap_hide_visible(self.ctx, pr, pp, C.c_void_p(k_em.ctypes.data), C.c_void_p(k_new.ctypes.data),
                                                       C.c_void_p(s_num.ctypes.data)))
        return s_num

    def depth_fill_segments(self, v_thresh, a_thresh_deg, use_visibility=False):
        """edgehip_depth_fill_segments: the grids of every sequence from its decoded segments (fillDepthMap, in-stream)."""
        self._ck(self.lib.edgehip_depth_fill_segments(self.ctx, C.c_double(v_thresh), C.c_double(a_thresh_deg), int(bool(use_visibility))))

    def edgemap_decode_ms(self):
        """edgehip_edgemap_decode_ms -> (decode_ms, hide_ms, items_ms, fill_ms) of the last such launches under profile_enable (-1: none)."""
        ms = (C.c_float * 4)()
        self._ck(self.lib.edgehip_edgemap_decode_ms(self.ctx, ms))
        return tuple(float(v) for v in ms)

    def depth_fill_net(self, p_off=(0.0, 0.0)):
        """edgehip_depth_fill_net: the grids of every sequence from its stored wire records (in-stream)."""
        self._ck(self.lib.edgehip_depth_fill_net(self.ctx, C.c_float(p_off[0]), C.c_float(p_off[1])))

    # ---- depth surface (computeDistance / calcSurfNormals / calcSurfArea / getImgRho*) ----
    # ---- the ROS nodelet's output: point cloud and EdgeMap records ----
    def ros_enable(self, what):
        """edgehip_ros_enable: the stores of `what` (ROS_POINTS | ROS_KEYLINES), cap records per sequence each; 0 (or None) frees them."""
        self._ck(self.lib.edgehip_ros_enable(self.ctx, int(what or 0)))
        self.ros_what = int(what or 0)

    def ros_pack(self, slot, k_prof=None):
        """edgehip_ros_pack: the nodelet's loop on the KeyLines of `slot` for every sequence (in-stream).  k_prof: [nseq] scales, or
        None = each sequence's seq_state.K."""
        kp = None if k_prof is None else np.ascontiguousarray(k_prof, dtype=np.float64)
        assert kp is None or kp.shape == (self.nseq,)
        self._ck(self.lib.edgehip_ros_pack(self.ctx, int(slot), _dp(kp) if kp is not None else None))

    def ros_edgemap(self, seq):
        """edgehip_download_ros_edgemap -> (points, keylines, kn): ROS_POINT_DTYPE / ROS_KEYLINE_DTYPE arrays of kn records (None for a
        store that is not enabled)."""
        return self.ros_edgemaps_batch([seq])[0]

    def ros_edgemaps_batch(self, seqs):
        """edgehip_download_ros_edgemaps_batch -> [(points, keylines, kn)] in the order of seqs."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        n = len(seqs)
        what = self.ros_what
        if not what:
            raise EdgeHipError("ros_edgemaps_batch: no store is enabled (ros_enable)")
        pts = [np.zeros(self.cap, ROS_POINT_DTYPE) if what & ROS_POINTS else None for _ in range(n)]
        kls = [np.zeros(self.cap, ROS_KEYLINE_DTYPE) if what & ROS_KEYLINES else None for _ in range(n)]
        pp = (C.c_void_p * n)(*[None if b is None else b.ctypes.data for b in pts])
        pk = (C.c_void_p * n)(*[None if b is None else b.ctypes.data for b in kls])
        kn = np.zeros(n, np.int32)
        self._ck(self.lib.edgehip_download_ros_edgemaps_batch(self.ctx, n, seqs.ctypes.data_as(C.c_void_p), pp, pk, kn.ctypes.data_as(C.c_void_p)))
        return [(None if p is None else p[:k].copy(), None if q is None else q[:k].copy(), int(k)) for p, q, k in zip(pts, kls, kn)]

    def ros_edgemap_into(self, points=None, keylines=None, kn=None, first=0):
        """edgehip_ros_edgemap_device: the whole stores of sequences [first, first + count) into torch tensors on the context's device —
        points uint8 (count, cap, 12), keylines uint8 (count, cap, 52), kn int32 (count,); any may be None."""
        given = [x for x in (points, keylines, kn) if x is not None]
        count = given[0].shape[0]
        for x, tail, item in ((points, (self.cap, 12), 1), (keylines, (self.cap, 52), 1), (kn, (), 4)):
            if x is not None:
                assert x.is_cuda and x.is_contiguous() and x.element_size() == item and tuple(x.shape) == (count,) + tail, tuple(x.shape)
        self._ck(self.lib.edgehip_ros_edgemap_device(self.ctx, int(first), int(count),
                                                     *[C.c_void_p(x.data_ptr()) if x is not None else None for x in (points, keylines, kn)]))

    def ros_edgemap_from(self, points=None, keylines=None, first=0):
        """edgehip_ros_edgemap_from_device (test support only: a sentinel behind the records): uint8 torch tensors (count, cap, 12) / (count, cap, 52) become the stores' bytes."""
        given = [x for x in (points, keylines) if x is not None]
        count = given[0].shape[0]
        for x, tail in ((points, (self.cap, 12)), (keylines, (self.cap, 52))):
            if x is not None:
                assert x.is_cuda and x.is_contiguous() and x.element_size() == 1 and tuple(x.shape) == (count,) + tail, tuple(x.shape)
        self._ck(self.lib.edgehip_ros_edgemap_from_device(self.ctx, int(first), int(count),
                                                          *[C.c_void_p(x.data_ptr()) if x is not None else None for x in (points, keylines)]))

    def ros_export(self, seqs, k_prof, what):
        """edgehip_ros_export: the OLD slot of the frame processed last, packed in-stream (no synchronisation) -> ticket."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        kp = np.ascontiguousarray(k_prof, dtype=np.float64)
        assert kp.shape == seqs.shape
        t = C.c_int(0)
        self._ck(self.lib.edgehip_ros_export(self.ctx, len(seqs), seqs.ctypes.data_as(C.c_void_p), _dp(kp), int(what), C.byref(t)))
        return (t.value, len(seqs), int(what))

    def ros_export_fetch(self, ticket, kns, registered=True):
        """edgehip_ros_export_fetch: enqueue the copies of kns[j] records per list (does not block); the arrays are valid after
        ros_export_wait."""
        tid, n, what = ticket
        kns = np.ascontiguousarray(kns, dtype=np.int32)
        assert len(kns) == n
        pts = [np.zeros(self.cap, ROS_POINT_DTYPE) if what & ROS_POINTS else None for _ in range(n)]
        kls = [np.zeros(self.cap, ROS_KEYLINE_DTYPE) if what & ROS_KEYLINES else None for _ in range(n)]
        bufs = [b for b in pts + kls if b is not None]
        if registered:
            for b in bufs:
                self._ck(self.lib.edgehip_register_host(C.c_void_p(b.ctypes.data), C.c_size_t(b.nbytes)))
        pp = (C.c_void_p * n)(*[None if b is None else b.ctypes.data for b in pts])
        pk = (C.c_void_p * n)(*[None if b is None else b.ctypes.data for b in kls])
        self._ck(self.lib.edgehip_ros_export_fetch(self.ctx, tid, kns.ctypes.data_as(C.c_void_p), pp, pk))
        return {"pts": pts, "kls": kls, "bufs": bufs, "kns": kns, "registered": registered, "ticket": ticket}

    def ros_export_wait(self, fetched):
        """edgehip_ros_export_wait.  With what ros_export_fetch returned: block until the copies have landed -> [(points, keylines)];
        with a bare ticket: release it unfetched."""
        if isinstance(fetched, tuple):
            self._ck(self.lib.edgehip_ros_export_wait(self.ctx, fetched[0]))
            return None
        self._ck(self.lib.edgehip_ros_export_wait(self.ctx, fetched["ticket"][0]))
        if fetched["registered"]:
            for b in fetched["bufs"]:
                self._ck(self.lib.edgehip_unregister_host(C.c_void_p(b.ctypes.data)))
        return [(None if p is None else p[:k].copy(), None if q is None else q[:k].copy())
                for p, q, k in zip(fetched["pts"], fetched["kls"], fetched["kns"])]

    def depth_surface_enable(self, surface=True, image_mode=0):
        """edgehip_depth_surface_enable; surface=None frees the products.  image_mode: 0 off, 1 getImgRho, 2 getImgRhoTriInterp."""
        if surface is None:
            self._ck(self.lib.edgehip_depth_surface_enable(self.ctx, None))
            return
        p = DepthSurfaceParams(int(bool(surface)), int(image_mode))
        self._ck(self.lib.edgehip_depth_surface_enable(self.ctx, C.byref(p)))

    def depth_surface(self):
        """edgehip_depth_surface: the enabled products of every sequence from the last fill's grids (in-stream)."""
        self._ck(self.lib.edgehip_depth_surface(self.ctx))

    def download_depth_surfaces(self, seqs):
        """edgehip_download_depth_surfaces_batch -> [dict(point (gh, gw, 3), normal (gh, gw, 3), area (gh, gw) float32,
        dist (gh, gw), min_dist float)] in the order of seqs."""
        gw, gh = self.depth_fill_size()
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        n = len(seqs)
        out = [dict(point=np.empty((gh, gw, 3)), normal=np.empty((gh, gw, 3)), area=np.empty((gh, gw), np.float32),
                    dist=np.empty((gh, gw)), min_dist=np.empty(1)) for _ in range(n)]
        ptrs = [(C.c_void_p * n)(*[o[k].ctypes.data for o in out]) for k in ("point", "normal", "area", "dist", "min_dist")]
        self._ck(self.lib.edgehip_download_depth_surfaces_batch(self.ctx, n, seqs.ctypes.data_as(C.c_void_p), *ptrs))
        for o in out:
            o["min_dist"] = float(o["min_dist"][0])
        return out

    def download_depth_surface(self, seq):
        """edgehip_download_depth_surface -> dict(point, normal, area, dist, min_dist) as download_depth_surfaces."""
        gw, gh = self.depth_fill_size()
        o = dict(point=np.empty((gh, gw, 3)), normal=np.empty((gh, gw, 3)), area=np.empty((gh, gw), np.float32),
                 dist=np.empty((gh, gw)), min_dist=np.empty(1))
        self._ck(self.lib.edgehip_download_depth_surface(self.ctx, int(seq), *[C.c_void_p(o[k].ctypes.data) for k in
                                                                               ("point", "normal", "area", "dist", "min_dist")]))
        o["min_dist"] = float(o["min_dist"][0])
        return o

    def download_depth_images(self, seqs):
        """edgehip_download_depth_images_batch -> [(rho, s_rho)] as (h, w) float32 arrays, in the order of seqs."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        n = len(seqs)
        out = [(np.empty((self.h, self.w), np.float32), np.empty((self.h, self.w), np.float32)) for _ in range(n)]
        pr = (C.c_void_p * n)(*[o[0].ctypes.data for o in out])
        ps = (C.c_void_p * n)(*[o[1].ctypes.data for o in out])
        self._ck(self.lib.edgehip_download_depth_images_batch(self.ctx, n, seqs.ctypes.data_as(C.c_void_p), pr, ps))
        return out

    def download_depth_image(self, seq):
        """edgehip_download_depth_image -> (rho, s_rho) as (h, w) float32 arrays."""
        rho, s_rho = np.empty((self.h, self.w), np.float32), np.empty((self.h, self.w), np.float32)
        self._ck(self.lib.edgehip_download_depth_image(self.ctx, int(seq), C.c_void_p(rho.ctypes.data), C.c_void_p(s_rho.ctypes.data)))
        return rho, s_rho

    def depth_image_into(self, rho, s_rho=None, first=0):
        """edgehip_depth_image_device: the images of sequences [first, first + len(rho)) into float32 torch tensors of shape
        (count, h, w) on the context's device (either may be None), device to device."""
        t = rho if rho is not None else s_rho
        count = t.shape[0]
        for x in (rho, s_rho):
            if x is not None:
                assert x.dtype.itemsize == 4 and x.is_floating_point() and x.is_contiguous(), "float32 contiguous tensors"
                assert tuple(x.shape) == (count, self.h, self.w), (tuple(x.shape), (count, self.h, self.w))
        self._ck(self.lib.edgehip_depth_image_device(self.ctx, int(first), int(count),
                                                     C.c_void_p(rho.data_ptr() if rho is not None else None),
                                                     C.c_void_p(s_rho.data_ptr() if s_rho is not None else None)))

    # ---- cross-view surface integration (surface_integrator.cpp: analizeSpaceSize, OcGrid::fillKFList / rayCutSurface) ----
    def surface_views_enable(self, capacity=64, n=(500, 500, 500)):
        """edgehip_surface_views_enable: `capacity` view slots and an nx x ny x nz voxel plane; capacity=None frees them."""
        if capacity is None:
            self._ck(self.lib.edgehip_surface_views_enable(self.ctx, None))
            return
        nx, ny, nz = (int(n),) * 3 if np.isscalar(n) else (int(v) for v in n)
        p = SurfaceViewsParams(int(capacity), nx, ny, nz)
        self._ck(self.lib.edgehip_surface_views_enable(self.ctx, C.byref(p)))

    @staticmethod
    def _pose(Pose, Pos):
        return np.ascontiguousarray(Pose, np.float64).reshape(9), np.ascontiguousarray(Pos, np.float64).reshape(3)

    def surface_view_capture(self, seq, view, Pose, Pos, K):
        """edgehip_surface_view_capture: sequence seq's grid of the last depth_fill into slot `view` (in-stream)."""
        Pose, Pos = self._pose(Pose, Pos)
        self._ck(self.lib.edgehip_surface_view_capture(self.ctx, int(seq), int(view), _dp(Pose), _dp(Pos), C.c_double(K)))

    def surface_view_upload(self, view, rho, s_rho, Pose, Pos, K):
        """edgehip_surface_view_upload: (gh, gw) float64 grids into slot `view`."""
        gw, gh = self.depth_fill_size()
        rho, s_rho = np.ascontiguousarray(rho, np.float64), np.ascontiguousarray(s_rho, np.float64)
        assert rho.shape == (gh, gw) and s_rho.shape == (gh, gw), (rho.shape, s_rho.shape, (gh, gw))
        Pose, Pos = self._pose(Pose, Pos)
        self._ck(self.lib.edgehip_surface_view_upload(self.ctx, int(view), _dp(rho), _dp(s_rho), _dp(Pose), _dp(Pos), C.c_double(K)))

    def surface_view_clear(self, view):
        self._ck(self.lib.edgehip_surface_view_clear(self.ctx, int(view)))

    def surface_space(self):
        """edgehip_surface_space -> (origin[3], size[3]) of analizeSpaceSize over the stored views."""
        origin, size = np.empty(3), np.empty(3)
        self._ck(self.lib.edgehip_surface_space(self.ctx, _dp(origin), _dp(size)))
        return origin, size

    def surface_integrate(self, origin, size, cast_views=None, accumulate=False):
        """edgehip_surface_integrate: rays of cast_views (None: every stored view), then the test of every stored view (in-stream)."""
        origin, size = np.ascontiguousarray(origin, np.float64).reshape(3), np.ascontiguousarray(size, np.float64).reshape(3)
        if cast_views is None:
            n, ptr = 0, None
        else:
            cast = np.ascontiguousarray(cast_views, dtype=np.int32).reshape(-1)
            n = len(cast)
            if n == 0:
                cast = np.zeros(1, np.int32)   # an empty list is not NULL ("every stored view")
            ptr = cast.ctypes.data_as(C.c_void_p)
        self._ck(self.lib.edgehip_surface_integrate(self.ctx, _dp(origin), _dp(size), n, ptr, int(bool(accumulate))))

    def surface_ray_cross(self, pairs=None, accumulate=False):
        """edgehip_surface_ray_cross: checkDFRayCrossExaustive for the ordered pairs [(target, hidder), ...] (None: every ordered pair of
        stored views), in-stream; the flags come back through download_surface_visibility."""
        if pairs is None:
            n, pt, ph = -1, None, None
        else:
            pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
            n = len(pr)
            t, h = (np.ascontiguousarray(pr[:, k]) if n else np.zeros(1, np.int32) for k in (0, 1))
            pt, ph = t.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p)
        self._ck(self.lib.edgehip_surface_ray_cross(self.ctx, n, pt, ph, int(bool(accumulate))))

    def download_surface_visibility(self, views):
        """edgehip_download_surface_visibility(_batch): one slot -> (gh, gw) bool array; a sequence of slots -> a list of them."""
        gw, gh = self.depth_fill_size()
        if np.isscalar(views):
            vis = np.empty((gh, gw), np.uint8)
            self._ck(self.lib.edgehip_download_surface_visibility(self.ctx, int(views), vis.ctypes.data_as(C.c_void_p)))
            return vis.astype(bool)
        views = np.ascontiguousarray(views, dtype=np.int32)
        n = len(views)
        out = [np.empty((gh, gw), np.uint8) for _ in range(n)]
        pv = (C.c_void_p * n)(*[o.ctypes.data for o in out])
        self._ck(self.lib.edgehip_download_surface_visibilities_batch(self.ctx, n, views.ctypes.data_as(C.c_void_p), pv))
        return [o.astype(bool) for o in out]

    def upload_keylines(self, seq, slot, kl, mask=None, retuned=0.0):
        kl = np.ascontiguousarray(kl, dtype=KEYLINE_DTYPE)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        self._ck(self.lib.edgehip_upload_keylines(self.ctx, seq, slot, kl.ctypes.data_as(C.c_void_p), len(kl),
                                                  None if m is None else m.ctypes.data_as(C.c_void_p),
                                                  C.c_float(retuned)))

    # ---- key-frame tracking (TrackKeyFrames) ----
    def keyframe_track_enable(self, enable=True, kf_save_percent=0.7, save_keyframes=True, in_frame_driver=True):
        """KFSavePercent and REBVO::saveKeyframes; enable=False frees the key frames and takes the steps out of process_frame;
        in_frame_driver=False keeps the store for the stage-level calls below and leaves process_frame as it is without the feature."""
        mode = 0 if not enable else (1 if in_frame_driver else 2)
        self._ck(self.lib.edgehip_keyframe_track_enable(self.ctx, mode, C.c_double(kf_save_percent), int(bool(save_keyframes))))
        self._kf_list_capacity = 0   # (the call frees the list with the key frames)

    @staticmethod
    def kf_pose(Pose=None, Pos=None, t=0.0, K=1.0):
        """A KfPose with the given pose (the other blocks zero: the tracking reads only Pose and Pos)."""
        q = KfPose()
        q.t, q.K = t, K
        q.Pose[:] = list(np.asarray(np.eye(3) if Pose is None else Pose, np.float64).reshape(9))
        q.Pos[:] = list(np.asarray(np.zeros(3) if Pos is None else Pos, np.float64).reshape(3))
        return q

    def keyframe_insert(self, slot, mask=None, poses=None):
        """keyframe(...) + resetForwardMatch + resetKFMatch from `slot` for the masked sequences (None: all); poses: one KfPose per
        sequence, or None for the newest nav record and seq_state.K."""
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(bool), np.uint8)
        assert m is None or m.shape == (self.nseq,)
        arr = None if poses is None else (KfPose * self.nseq)(*poses)
        self._ck(self.lib.edgehip_keyframe_insert(self.ctx, slot, None if m is None else m.ctypes.data_as(C.c_void_p), arr))

    def _kf_pose_args(self, Pose, Pos):
        if Pose is None and Pos is None:
            return None, None, None
        P = np.ascontiguousarray(np.broadcast_to(np.asarray(Pose, np.float64).reshape(-1, 9), (self.nseq, 9)))
        T = np.ascontiguousarray(np.broadcast_to(np.asarray(Pos, np.float64).reshape(-1, 3), (self.nseq, 3)))
        return _dp(P), _dp(T), (P, T)

    def keyframe_build_forward_match(self, slot_new):
        cnt = np.zeros(self.nseq, np.int32)
        self._ck(self.lib.edgehip_keyframe_build_forward_match(self.ctx, slot_new, cnt.ctypes.data_as(C.c_void_p)))
        return cnt

    def keyframe_forward_correct(self, slot_new, Pose=None, Pos=None, dist_thresh=10.0, dist_tolerance=0.0, augmentate=True):
        """Pose [nseq][3][3], Pos [nseq][3] (both None: Pose*R, Pos - Pose*R*V*K from seq_state) -> counts[nseq]."""
        cnt = np.zeros(self.nseq, np.int32)
        pp, pt, keep = self._kf_pose_args(Pose, Pos)
        self._ck(self.lib.edgehip_keyframe_forward_correct(self.ctx, slot_new, pp, pt, C.c_double(dist_thresh), C.c_double(dist_tolerance),
                                                           int(bool(augmentate)), cnt.ctypes.data_as(C.c_void_p)))
        return cnt

    def keyframe_back_correct(self, slot_new, Pose=None, Pos=None, dist_thresh=10.0, dist_tolerance=0.0, augmentate=True):
        cnt = np.zeros(self.nseq, np.int32)
        pp, pt, keep = self._kf_pose_args(Pose, Pos)
        self._ck(self.lib.edgehip_keyframe_back_correct(self.ctx, slot_new, pp, pt, C.c_double(dist_thresh), C.c_double(dist_tolerance),
                                                        int(bool(augmentate)), cnt.ctypes.data_as(C.c_void_p)))
        return cnt

    def read_keyframe_track(self):
        """The per-frame records as a structured array [nseq] (KF_TRACK_DTYPE)."""
        out = np.zeros(self.nseq, KF_TRACK_DTYPE)
        self._ck(self.lib.edgehip_read_keyframe_track(self.ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    def download_keyframe(self, seq):
        """-> (KeyLine records [kn], KfPose, kf_count) of the sequence's current key frame."""
        kl = np.zeros(self.cap, KEYLINE_DTYPE)
        kn, cnt, pose = C.c_int32(0), C.c_int32(0), KfPose()
        self._ck(self.lib.edgehip_download_keyframe(self.ctx, seq, kl.ctypes.data_as(C.c_void_p), C.byref(kn), C.byref(pose), C.byref(cnt)))
        return kl[:kn.value].copy(), pose, cnt.value

    def upload_keyframe(self, seq, kl, pose):
        kl = np.ascontiguousarray(kl, dtype=KEYLINE_DTYPE)
        self._ck(self.lib.edgehip_upload_keyframe(self.ctx, seq, kl.ctypes.data_as(C.c_void_p), len(kl), C.byref(pose)))

    def keyframe_set_save(self, save_keyframes):
        """REBVO::saveKeyframes at run time (startKeyFrames / endKeyFrames): from the next frame on; key frames and list stay."""
        self._ck(self.lib.edgehip_keyframe_set_save(self.ctx, int(bool(save_keyframes))))

    # ---- the key-frame list (REBVO::kf_list) ----
    def keyframe_list_enable(self, capacity):
        """A ring of `capacity` retired key frames per sequence (0 frees it); needs keyframe_track_enable."""
        self._ck(self.lib.edgehip_keyframe_list_enable(self.ctx, int(capacity)))
        self._kf_list_capacity = int(capacity)

    def keyframe_list_info(self):
        """-> structured array [nseq] (KF_LIST_INFO_DTYPE): kf_count, first, held, overwritten."""
        out = np.zeros(self.nseq, KF_LIST_INFO_DTYPE)
        self._ck(self.lib.edgehip_keyframe_list_info(self.ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    def download_keyframe_list(self, seq, ordinal):
        """seq, ordinal ints -> (KeyLine records [kn], KfPose) of that list entry; sequences of both -> a list of such pairs, through
        the batch call."""
        single = np.isscalar(seq)
        seqs = np.atleast_1d(np.asarray(seq, np.int32)).copy()
        ords = np.atleast_1d(np.asarray(ordinal, np.int32)).copy()
        assert seqs.shape == ords.shape and seqs.ndim == 1 and len(seqs) >= 1
        n = len(seqs)
        kls = [np.zeros(self.cap, KEYLINE_DTYPE) for _ in range(n)]
        ptrs = (C.c_void_p * n)(*[k.ctypes.data for k in kls])
        kn = np.zeros(n, np.int32)
        poses = (KfPose * n)()
        if single:
            self._ck(self.lib.edgehip_download_keyframe_list(self.ctx, int(seqs[0]), int(ords[0]), C.c_void_p(kls[0].ctypes.data), kn.ctypes.data_as(C.c_void_p), poses))
        else:
            self._ck(self.lib.edgehip_download_keyframe_list_batch(self.ctx, n, seqs.ctypes.data_as(C.c_void_p), ords.ctypes.data_as(C.c_void_p),
                                                                   ptrs, kn.ctypes.data_as(C.c_void_p), poses))
        out = [(kls[j][:kn[j]].copy(), KfPose.from_buffer_copy(poses[j])) for j in range(n)]
        return out[0] if single else out

    def keyframe_list_restore(self, slot, ordinals):
        """List entry ordinals[seq] of every sequence back into ring slot `slot` (-1: leave that sequence's slot alone)."""
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(ordinals, np.int32), (self.nseq,))).copy()
        self._ck(self.lib.edgehip_keyframe_list_restore(self.ctx, slot, o.ctypes.data_as(C.c_void_p)))

    # ---- key-frame covisibility (kfvo::countMatches, kfvo::kls_on_fov) ----
    @staticmethod
    def _covis_args(field_radius, field_min_mod, match_mod, match_ang, rho_tol, max_r):
        return KfCovisArgs(int(field_radius), float(field_min_mod), float(match_mod), float(match_ang), float(rho_tol), float(max_r))

    def keyframe_covisibility(self, field_radius, match_mod, match_ang, rho_tol, max_r, field_min_mod=0.0):
        """Every ordered pair of each sequence's key frames (list entries oldest first, then the current one) -> (counts, info):
        counts a structured array (nseq, M, M) of KF_PAIR_COUNT_DTYPE indexed [seq][to][from], M = list capacity + 1, -1 where the
        sequence lacks a position; info as keyframe_list_info() returns it, of the same moment."""
        m = getattr(self, "_kf_list_capacity", 0) + 1
        out = np.zeros((self.nseq, m, m), KF_PAIR_COUNT_DTYPE)
        info = np.zeros(self.nseq, KF_LIST_INFO_DTYPE)
        a = self._covis_args(field_radius, field_min_mod, match_mod, match_ang, rho_tol, max_r)
        self._ck(self.lib.edgehip_keyframe_covisibility(self.ctx, C.byref(a), out.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)))
        return out, info

    def keyframe_covisibility_slot(self, slot, field_radius, match_mod, match_ang, rho_tol, max_r, field_min_mod=0.0, poses=None):
        """Ring slot `slot`'s KeyLines as `from` (poses: one KfPose per sequence, or None for the newest nav record and seq_state.K)
        against every key frame of the same sequence -> (counts (nseq, M), info)."""
        m = getattr(self, "_kf_list_capacity", 0) + 1
        out = np.zeros((self.nseq, m), KF_PAIR_COUNT_DTYPE)
        info = np.zeros(self.nseq, KF_LIST_INFO_DTYPE)
        a = self._covis_args(field_radius, field_min_mod, match_mod, match_ang, rho_tol, max_r)
        arr = None if poses is None else (KfPose * self.nseq)(*poses)
        self._ck(self.lib.edgehip_keyframe_covisibility_slot(self.ctx, int(slot), arr, C.byref(a), out.ctypes.data_as(C.c_void_p),
                                                             info.ctypes.data_as(C.c_void_p)))
        return out, info

    def keyframe_covisibility_ms(self):
        """-> (field build ms, pair pass ms) of the last covisibility call, by HIP events."""
        f, p = C.c_double(0), C.c_double(0)
        self._ck(self.lib.edgehip_keyframe_covisibility_ms(self.ctx, C.byref(f), C.byref(p)))
        return f.value, p.value

    # ---- re-localisation against the key frames (kfvo::OptimizePosGT, optimizeScale) ----
    def keyframe_relocalize(self, slot, s_rho_q, field_radius, iter_max, rew_dis, rho_tol, field_min_mod=0.0, poses=None, to_mask=None):
        """Ring slot `slot`'s frame (poses: one KfPose per sequence, or None for the newest nav record and seq_state.K; s_rho_q: a
        scalar or one per sequence) against every key frame of the same sequence that to_mask (nseq, M) selects (None: all) ->
        (results (nseq, M) of KF_RELOC_DTYPE, info).  A position the sequence lacks or the mask deselects has every integer field -1."""
        m = getattr(self, "_kf_list_capacity", 0) + 1
        out = np.zeros((self.nseq, m), KF_RELOC_DTYPE)
        info = np.zeros(self.nseq, KF_LIST_INFO_DTYPE)
        a = KfRelocArgs(int(field_radius), float(field_min_mod), int(iter_max), float(rew_dis), float(rho_tol))
        q = np.ascontiguousarray(np.broadcast_to(np.asarray(s_rho_q, np.float64), (self.nseq,))).copy()
        arr = None if poses is None else (KfPose * self.nseq)(*poses)
        mk = None
        if to_mask is not None:
            mk = np.ascontiguousarray(np.broadcast_to(np.asarray(to_mask).astype(np.uint8), (self.nseq, m))).copy()
        self._ck(self.lib.edgehip_keyframe_relocalize(self.ctx, int(slot), arr, q.ctypes.data_as(C.c_void_p),
                                                      None if mk is None else mk.ctypes.data_as(C.c_void_p), C.byref(a),
                                                      out.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)))
        return out, info

    def keyframe_relocalize_links(self, seq, position):
        """-> m_id_f [kn] int32 of the last keyframe_relocalize call's pair (seq, position), or None for a pair it did not serve."""
        m = np.full(self.cap, -1, np.int32)
        kn = C.c_int32(-1)
        self._ck(self.lib.edgehip_keyframe_relocalize_links(self.ctx, int(seq), int(position), m.ctypes.data_as(C.c_void_p), C.byref(kn)))
        return None if kn.value < 0 else m[:kn.value].copy()

    def keyframe_relocalize_ms(self):
        """-> (prepare ms, solve ms) of the last keyframe_relocalize call, by HIP events."""
        f, p = C.c_double(0), C.c_double(0)
        self._ck(self.lib.edgehip_keyframe_relocalize_ms(self.ctx, C.byref(f), C.byref(p)))
        return f.value, p.value

    # ---- key-frame relative-pose constraint (kfvo::OptimizeRelContraint, mutualExclusionSimple) ----
    def keyframe_constraint(self, slot_new, direction, iter_max, k_huber, Pose=None, Pos=None, K=None):
        """Every sequence's current key frame against ring slot `slot_new` -> a dict of arrays: X (nseq, 6), W_X and R_X (nseq, 6, 6),
        ratio, E, E0, Kp, W_Kp (nseq,), links, inliers, evals, accepted, guard (nseq,) int32.  Pose (nseq, 3, 3), Pos (nseq, 3) and
        K (nseq,) are given together, or all None for Pose*R, Pos - Pose*R*V*K and K from seq_state."""
        out = np.zeros(self.nseq, KF_CONSTRAINT_DTYPE)
        a = KfConstraintArgs(int(direction), int(iter_max), float(k_huber))
        pp = pt = pk = None
        if Pose is not None or Pos is not None or K is not None:
            assert Pose is not None and Pos is not None and K is not None, "Pose, Pos and K are given together"
            P = np.ascontiguousarray(np.broadcast_to(np.asarray(Pose, np.float64).reshape(-1, 9), (self.nseq, 9)))
            T = np.ascontiguousarray(np.broadcast_to(np.asarray(Pos, np.float64).reshape(-1, 3), (self.nseq, 3)))
            S = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1), (self.nseq,)))
            pp, pt, pk = _dp(P), _dp(T), _dp(S)
        self._ck(self.lib.edgehip_keyframe_constraint(self.ctx, int(slot_new), pp, pt, pk, C.byref(a), out.ctypes.data_as(C.c_void_p)))
        res = {k: out[k].copy() for k in out.dtype.names if k != "pad"}
        res["W_X"] = res["W_X"].reshape(self.nseq, 6, 6)
        res["R_X"] = res["R_X"].reshape(self.nseq, 6, 6)
        return res

    def keyframe_mutual_exclusion(self, slot_new, dist_t, discard_non_mutual, kf_to_frame, want_counts=True):
        """mutualExclusionSimple between the key frames and `slot_new`: kf_to_frame edits the key frames' m_id_f, otherwise the slot's
        m_id_kf -> counts (nseq, 2) = (links seen, links kept), or None (and no synchronisation) when want_counts is False."""
        cnt = np.zeros((self.nseq, 2), np.int32) if want_counts else None
        self._ck(self.lib.edgehip_keyframe_mutual_exclusion(self.ctx, int(slot_new), C.c_double(dist_t), int(bool(discard_non_mutual)),
                                                            int(bool(kf_to_frame)), None if cnt is None else cnt.ctypes.data_as(C.c_void_p)))
        return cnt

    def keyframe_constraint_ms(self):
        """-> (gather ms, solve ms) of the last keyframe_constraint call, by HIP events."""
        g, s = C.c_double(0), C.c_double(0)
        self._ck(self.lib.edgehip_keyframe_constraint_ms(self.ctx, C.byref(g), C.byref(s)))
        return g.value, s.value

    # ---- key-frame depth along the links (kfvo::mapKFUsingIDK, translateDepth_F2KF / _KF2F / _New2Old) ----
    def _kf_depth_pose(self, Pose, Pos, K, with_K):
        given = [x is not None for x in ((Pose, Pos, K) if with_K else (Pose, Pos))]
        if not any(given):
            return None, None, None, None
        assert all(given), "Pose, Pos and K are given together" if with_K else "Pose and Pos are given together"
        P = np.ascontiguousarray(np.broadcast_to(np.asarray(Pose, np.float64).reshape(-1, 9), (self.nseq, 9)))
        T = np.ascontiguousarray(np.broadcast_to(np.asarray(Pos, np.float64).reshape(-1, 3), (self.nseq, 3)))
        S = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1), (self.nseq,))) if with_K else None
        return _dp(P), _dp(T), (None if S is None else _dp(S)), (P, T, S)

    @staticmethod
    def _kf_depth_result(out):
        return None if out is None else {k: out[k].copy() for k in out.dtype.names}

    def keyframe_map_depth(self, slot_new, reshape_q_abs, reshape_q_rel, location_uncertainty, Pose=None, Pos=None, want_result=True):
        """mapKFUsingIDK of every sequence's current key frame against ring slot `slot_new` -> a dict of arrays (nseq,): count, guard, K,
        rTr, rTr0 (the last three 0), or None (and no synchronisation) when want_result is False.  Pose (nseq, 3, 3) and Pos (nseq, 3)
        are given together, or both None for Pose*R and Pos - Pose*R*V*K from seq_state."""
        out = np.zeros(self.nseq, KF_DEPTH_DTYPE) if want_result else None
        pp, pt, _, keep = self._kf_depth_pose(Pose, Pos, None, False)
        self._ck(self.lib.edgehip_keyframe_map_depth(self.ctx, int(slot_new), pp, pt, C.c_double(reshape_q_abs), C.c_double(reshape_q_rel),
                                                     C.c_double(location_uncertainty), None if out is None else out.ctypes.data_as(C.c_void_p)))
        return self._kf_depth_result(out)

    def keyframe_translate_depth(self, slot_new, direction, optim_scale=False, Pose=None, Pos=None, K=None, want_result=True):
        """direction 0: translateDepth_F2KF (the slot's depth into the key frame, optim_scale first re-estimates the key frame's K);
        direction 1: translateDepth_KF2F (the key frame's depth into the SLOT's rho / s_rho) -> a dict of arrays (nseq,): count, guard,
        K (the kf.K used), rTr, rTr0, or None (and no synchronisation) when want_result is False.  Pose, Pos and K (nseq,) are given
        together, or all None for the defaults of keyframe_constraint."""
        out = np.zeros(self.nseq, KF_DEPTH_DTYPE) if want_result else None
        pp, pt, pk, keep = self._kf_depth_pose(Pose, Pos, K, True)
        self._ck(self.lib.edgehip_keyframe_translate_depth(self.ctx, int(slot_new), int(direction), pp, pt, pk, int(bool(optim_scale)),
                                                           None if out is None else out.ctypes.data_as(C.c_void_p)))
        return self._kf_depth_result(out)

    def keyframe_list_translate_depth(self, iters):
        """translateDepth_New2Old over every sequence's held list entries (oldest first) and its current key frame -> a dict of arrays
        (nseq,): count (links of the last iteration), guard, K, rTr, rTr0 (0)."""
        out = np.zeros(self.nseq, KF_DEPTH_DTYPE)
        self._ck(self.lib.edgehip_keyframe_list_translate_depth(self.ctx, int(iters), out.ctypes.data_as(C.c_void_p)))
        return self._kf_depth_result(out)

    def keyframe_depth_select(self, mask=None):
        """Restrict the three calls above to the sequences with mask[seq] true (None: every sequence again)."""
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(bool), np.uint8)
        assert m is None or m.shape == (self.nseq,)
        self._ck(self.lib.edgehip_keyframe_depth_select(self.ctx, None if m is None else m.ctypes.data_as(C.c_void_p)))

    def keyframe_depth_ms(self):
        """-> device ms of the last of the three calls above, by HIP events."""
        ms = C.c_double(0)
        self._ck(self.lib.edgehip_keyframe_depth_ms(self.ctx, C.byref(ms)))
        return ms.value

    # ---- the frame as a baseline JPEG (libjpeg's stream at the settings gd leaves it with) ----
    def jpeg_enable(self, quality=90, cap_bytes=None, comment=None):
        """edgehip_jpeg_enable: one region of cap_bytes per sequence (None: edgehip_jpeg_bound of the context's frame, which no stream
        exceeds; 0 frees the store), the tables of `quality`, `comment` (bytes or str) as COM segment."""
        if isinstance(comment, str):
            comment = comment.encode()
        if cap_bytes is None:
            cap_bytes = jpeg_bound(self.w, self.h, len(comment or b""))
        self._ck(self.lib.edgehip_jpeg_enable(self.ctx, int(quality), C.c_uint32(int(cap_bytes)), comment))
        self.jpeg_cap = int(cap_bytes)

    def jpeg_encode(self, slot):
        """edgehip_jpeg_encode: every (selected) sequence's frame of `slot` into its region (in-stream)."""
        self._ck(self.lib.edgehip_jpeg_encode(self.ctx, int(slot)))

    def jpeg_select(self, mask=None):
        """Restrict jpeg_encode to the sequences with mask[seq] true (None: every sequence again)."""
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(bool), np.uint8)
        assert m is None or m.shape == (self.nseq,)
        self._ck(self.lib.edgehip_jpeg_select(self.ctx, None if m is None else m.ctypes.data_as(C.c_void_p)))

    def jpeg_download(self, seq, with_record=False):
        """edgehip_download_jpeg -> the stream as a uint8 array (its first cap_bytes bytes when it overflowed); with_record: (stream,
        true size, overflow flag)."""
        return self.jpeg_download_batch([seq], with_record)[0]

    def jpeg_download_batch(self, seqs, with_record=False):
        """edgehip_download_jpeg_batch -> the streams in the order of seqs."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        n = len(seqs)
        bufs = [np.zeros(self.jpeg_cap, np.uint8) for _ in range(n)]
        rec = np.zeros((n, 2), np.uint32)
        pd = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        self._ck(self.lib.edgehip_download_jpeg_batch(self.ctx, n, seqs.ctypes.data_as(C.c_void_p), pd, C.c_uint32(self.jpeg_cap),
                                                      rec.ctypes.data_as(C.c_void_p)))
        out = [b[:min(int(r[0]), self.jpeg_cap)].copy() for b, r in zip(bufs, rec)]
        return [(o, int(r[0]), bool(r[1])) for o, r in zip(out, rec)] if with_record else out

    def jpeg_export(self, slot, seqs):
        """edgehip_jpeg_export: the frames of `seqs` in `slot` encoded in-stream into a ring entry -> ticket."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        t = C.c_int(0)
        self._ck(self.lib.edgehip_jpeg_export(self.ctx, int(slot), len(seqs), seqs.ctypes.data_as(C.c_void_p), C.byref(t)))
        return (t.value, len(seqs))

    def jpeg_export_fetch(self, ticket):
        """edgehip_jpeg_export_sizes + _fetch: waits for the ticket's encoder only, enqueues the copies (does not wait for them) ->
        (streams, records (n, 2) uint32); the streams are valid after jpeg_export_wait."""
        tk, n = ticket
        rec = np.zeros((n, 2), np.uint32)
        self._ck(self.lib.edgehip_jpeg_export_sizes(self.ctx, tk, rec.ctypes.data_as(C.c_void_p)))
        bufs = [np.zeros(min(int(r[0]), self.jpeg_cap), np.uint8) for r in rec]
        pd = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        self._ck(self.lib.edgehip_jpeg_export_fetch(self.ctx, tk, pd))
        return bufs, rec

    def jpeg_export_wait(self, ticket):
        self._ck(self.lib.edgehip_jpeg_export_wait(self.ctx, ticket[0]))

    def jpeg_device(self, bytes_out=None, sizes_out=None, first=0):
        """edgehip_jpeg_device: the regions of sequences [first, first + count) into torch tensors on the context's device, bytes_out
        uint8 (count, stride) with stride = cap_bytes rounded up to 16, sizes_out int32 / uint32 (count, 2) (either may be None)."""
        t = bytes_out if bytes_out is not None else sizes_out
        count = t.shape[0]
        if bytes_out is not None:
            assert bytes_out.dtype.itemsize == 1 and bytes_out.is_contiguous() and tuple(bytes_out.shape) == (count, (self.jpeg_cap + 15) & ~15)
        if sizes_out is not None:
            assert sizes_out.dtype.itemsize == 4 and sizes_out.is_contiguous() and tuple(sizes_out.shape) == (count, 2)
        self._ck(self.lib.edgehip_jpeg_device(self.ctx, int(first), int(count),
                                              C.c_void_p(bytes_out.data_ptr() if bytes_out is not None else None),
                                              C.c_void_p(sizes_out.data_ptr() if sizes_out is not None else None)))

    def jpeg_encode_images(self, images, quality=90, cap=None):
        """edgehip_jpeg_encode_images: `images` (count, h, w, 3) uint8 — a numpy array, or a torch tensor on the context's device —
        through the encoder's kernel -> [(stream, true size, overflow flag)].  cap: bytes per image (a multiple of 16; None: the bound)."""
        import torch
        dev = torch.device("cuda", self.device)
        t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images, np.uint8)).to(dev)
        assert t.dtype == torch.uint8 and t.dim() == 4 and t.shape[3] == 3 and t.is_contiguous() and t.device == dev
        count, h, w = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
        cap = (jpeg_bound(w, h) + 15) & ~15 if cap is None else int(cap)
        out = torch.zeros((count, cap), dtype=torch.uint8, device=dev)
        rec = torch.zeros((count, 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)   # the tensors were made on torch's stream, the encoder runs on the context's
        self._ck(self.lib.edgehip_jpeg_encode_images(self.ctx, C.c_void_p(t.data_ptr()), w, h, count, int(quality), C.c_void_p(out.data_ptr()),
                                                     C.c_uint32(cap), C.c_void_p(rec.data_ptr())))
        out, rec = out.cpu().numpy(), rec.cpu().numpy()
        return [(o[:min(int(r[0]), cap)].copy(), int(r[0]), bool(r[1])) for o, r in zip(out, rec)]

    # ---- baseline JPEG frames decoded on the device (MJPEG ingest) ----
    jpeg_probe = staticmethod(jpeg_probe)

    def jpeg_decode_enable(self, max_streams=None, cap_bytes=None):
        """edgehip_jpeg_decode_enable: room for max_streams (None: nseq) compressed frames of cap_bytes each per upload_jpeg
        (None: w * h bytes; 0 frees it)."""
        cap = self.w * self.h if cap_bytes is None else int(cap_bytes)
        self._ck(self.lib.edgehip_jpeg_decode_enable(self.ctx, int(self.nseq if max_streams is None else max_streams), C.c_uint32(cap)))

    def upload_jpeg(self, slot, streams, seq_first=0, fmt=FRAME_RGB24):
        """edgehip_upload_jpeg: one JPEG per sequence from seq_first on, decoded into the slot's own storage (in-stream).  Raises
        EdgeHipError with .reasons (per stream) when a stream is not decodable on the device: nothing was enqueued then."""
        keep, data, size = _stream_args(streams)
        reasons = np.zeros(len(keep), np.int32)
        rc = self.lib.edgehip_upload_jpeg(self.ctx, int(slot), data, size, int(seq_first), len(keep), int(fmt), reasons.ctypes.data_as(C.c_void_p))
        if rc != 0:
            err = EdgeHipError(f"edgehip error {rc}: {self.lib.edgehip_last_error().decode()}")
            err.code, err.reasons = rc, reasons.tolist()
            raise err

    def jpeg_decode_status(self, slot):
        """edgehip_read_jpeg_decode_status -> int32 [nseq]: how the entropy walk of the slot's last upload_jpeg ended per sequence."""
        st = np.zeros(self.nseq, np.int32)
        self._ck(self.lib.edgehip_read_jpeg_decode_status(self.ctx, int(slot), st.ctypes.data_as(C.c_void_p)))
        return st

    def jpeg_decode_ms(self):
        """edgehip_jpeg_decode_ms -> (entropy walk, inverse DCT, pixels) device milliseconds and the bytes moved of the last upload_jpeg,
        which must have been made under profile_enable()."""
        ms, moved = (C.c_float * 3)(), C.c_uint64(0)
        self._ck(self.lib.edgehip_jpeg_decode_ms(self.ctx, ms, C.byref(moved)))
        return tuple(float(v) for v in ms) + (int(moved.value),)

    def jpeg_decode_images(self, streams, w, h, out=None, offset=0):
        """edgehip_jpeg_decode_images: streams of one size -> (count, h, w, 3) uint8.  out: a torch uint8 tensor on the context's
        device that takes the images from byte `offset` on (returned as it is, whole).  Raises EdgeHipError with .reasons."""
        import torch
        dev = torch.device("cuda", self.device)
        keep, data, size = _stream_args(streams)
        nb = len(keep) * int(w) * int(h) * 3
        t = torch.zeros(nb, dtype=torch.uint8, device=dev) if out is None else out
        assert t.dtype == torch.uint8 and t.is_contiguous() and t.device == dev and t.numel() >= offset + nb
        torch.cuda.synchronize(dev)   # the tensor was made on torch's stream, the decoder runs on the context's
        reasons = np.zeros(len(keep), np.int32)
        rc = self.lib.edgehip_jpeg_decode_images(self.ctx, data, size, len(keep), int(w), int(h), C.c_void_p(t.data_ptr() + int(offset)),
                                                 reasons.ctypes.data_as(C.c_void_p))
        if rc != 0:
            err = EdgeHipError(f"edgehip error {rc}: {self.lib.edgehip_last_error().decode()}")
            err.code, err.reasons = rc, reasons.tolist()
            raise err
        return t.cpu().numpy().reshape(len(keep), int(h), int(w), 3) if out is None else t

    def download_frame(self, seq, slot):
        """edgehip_download_frame: the slot's own frame storage of `seq` -> (h, w, 3) RGB24 or (h, w) 8-bit mono, whichever it holds."""
        out = np.zeros(self.h * self.w * 3, np.uint8)
        fmt = C.c_int(0)
        self._ck(self.lib.edgehip_download_frame(self.ctx, int(seq), int(slot), C.c_void_p(out.ctypes.data), C.byref(fmt)))
        return out[:self.h * self.w].reshape(self.h, self.w).copy() if fmt.value == FRAME_GREY8 else out.reshape(self.h, self.w, 3)

    def download_plane(self, seq, which):
        idx = {"img0": 0, "img1": 1, "dog": 2, "dx": 3, "dy": 4}[which]
        out = np.zeros((self.h, self.w), np.float32)
        self._ck(self.lib.edgehip_download_plane(self.ctx, seq, idx, out.ctypes.data_as(C.c_void_p)))
        return out

    def download_field(self, seq):
        out = np.zeros((self.h, self.w, 2), np.int32)
        self._ck(self.lib.edgehip_download_field(self.ctx, seq, out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- measurement ----
    def profile_enable(self, on=True):
        self._ck(self.lib.edgehip_profile_enable(self.ctx, int(on)))

    def profile_select(self, names=None):
        n = self.lib.edgehip_profile_count()
        mask = 0
        for i in range(n):
            if names is None or self.lib.edgehip_profile_name(i).decode() in names:
                mask |= 1 << i
        self._ck(self.lib.edgehip_profile_select(self.ctx, C.c_uint64(mask)))

    def profile_read(self):
        n = self.lib.edgehip_profile_count()
        ms = np.zeros(n)
        calls = np.zeros(n, np.int64)
        self._ck(self.lib.edgehip_profile_read(self.ctx, _dp(ms), calls.ctypes.data_as(C.c_void_p)))
        return {self.lib.edgehip_profile_name(i).decode(): (float(ms[i]), int(calls[i])) for i in range(n)}
