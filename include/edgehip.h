/* edgehip.h — C ABI of libedgehip.so: REBVO's per-frame edge pipeline as hand-written HIP for gfx950.
 *
 * This is the drop-in boundary.  Every entry point replaces one call that the reference's
 * REBVO::FirstThr / REBVO::SecondThread make into mtracklib; the file:line each one replaces is cited at
 * its declaration (paths relative to the reference tree).  Plain pointers and sizes only — no C++ or
 * torch types — so the same library binds from C++ (rebvo_amd/host), ctypes (rebvo_amd/edgehip.py) or
 * any other FFI.
 *
 * Model.  One context = `nseq` independent image sequences that advance in lock-step on ONE GPU (the
 * sequence index is the batch dimension of every kernel launch), each with a ring of `nslots` frame
 * slots — the device-side counterpart of the reference's PipeBuffer ring (src/rebvo/rebvo.cpp:297-312).
 * All KeyLine lists, masks, auxiliary fields and the tracker/mapper state live in HBM as
 * structure-of-arrays; the 168-byte AoS `KeyLine` is materialised only by edgehip_download_keylines()
 * for callback consumers and parity tests.
 *
 * Calls enqueue work on the context's HIP stream and return immediately unless documented as
 * synchronising.  Every function returns 0 on success or a negative edgehip_status; the message of the
 * last failure on the calling thread is available from edgehip_last_error().  Nothing here ever falls
 * back to a CPU implementation: if no gfx950 device is usable, edgehip_create() fails.
 */
#ifndef EDGEHIP_H
#define EDGEHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDGEHIP_ABI_VERSION 2
#define EDGEHIP_KEYLINE_MAX 50000 /* KEYLINE_MAX, include/mtracklib/edge_finder.h:43 */

typedef enum edgehip_status {
    EDGEHIP_OK = 0,
    EDGEHIP_ERR_ARG = -1,     /* bad argument (slot/sequence out of range, null pointer, size mismatch) */
    EDGEHIP_ERR_DEVICE = -2,  /* no usable gfx950 device / HIP runtime error */
    EDGEHIP_ERR_MEMORY = -3,  /* hipMalloc / hipHostMalloc failed */
    EDGEHIP_ERR_STATE = -4    /* call sequence error (e.g. track before two frames were detected) */
} edgehip_status;

typedef struct edgehip_ctx edgehip_ctx;

/* The REBVOParameters fields (include/rebvo/rebvo.h:64-235) that reach the hot path.  Same meaning and
 * units as the reference's config keys (app/rebvorun/GlobalConfig_EuRoC). */
typedef struct edgehip_params {
    int32_t w, h;                 /* ImageWidth, ImageHeight */
    double ppx, ppy, zfx, zfy;    /* PPx, PPy, ZfX, ZfY (stored as float like REBVOParameters does) */
    double kc[5];                 /* KcR2 KcR4 KcR6 KcP1 KcP2 */
    double sigma0, ksigma;        /* Sigma0, KSigma */
    int32_t plane_fit_size;       /* DetectorPlaneFitSize: 1, 2 or 3 = a 3x3, 5x5 or 7x7 plane-fit window (edge_finder.cpp:110-137) */
    double pos_neg_thresh, dog_thresh;
    int32_t max_points, reference_points, track_points;
    double detector_thresh, auto_gain, max_thresh, min_thresh;
    int32_t search_range, qcut_nbins;
    double qcut_quantile;
    int32_t tracker_iter_num, tracker_init_type, tracker_init_iter_num;
    double tracker_match_thresh, match_thresh_module, match_thresh_angle;
    uint32_t match_num_thresh;
    int32_t do_rescaling;
    double reweight_distance, regularize_thresh;
    double loc_unc_match, reshape_q_abs, reshape_q_rel, loc_unc;
    int32_t global_match_threshold;
    int32_t debug_planes;         /* !=0: also store img0/img1/dog/dx/dy planes (parity tests) */
    double config_fps;
    /* UseUndistort: resample every input frame through the radial-tangential model `kc` before RGB->grey,
     * i.e. image_undistort::undistort<true> of rebvo_first_t.cpp:231 (include/VideoLib/image_undistort.h:
     * 66-79, 105-122; map as built by src/VideoLib/image_undistort.cpp:29-95), fused into the first
     * stage-A kernel: the bilinear map (4 taps, 16.16 integer weights) is built once at create time. */
    int32_t use_undistort;
    /* REBVO/StereoAvaiable: allocate the stereo KeyLine fields (stereo_m_id, stereo_rho, stereo_s_rho), and run
     * directed_matching in its stereo mode (the match copies rho0/s_rho0 instead of rho/s_rho and leaves rho_nr alone,
     * edge_tracker.cpp:343-351).  The pair image's edge map lives in a ring slot of its own (see
     * edgehip_directed_matching_stereo). */
    int32_t stereo_available;
} edgehip_params;

/* Byte-for-byte the reference's rebvo::KeyLine (include/mtracklib/edge_finder.h:45-91), 168 B. */
typedef struct edgehip_keyline {
    int32_t p_inx;
    float m_m[2], u_m[2], n_m, score, c_p[2];
    double rho, s_rho, rho_nr, s_rho_nr, rho0, s_rho0;
    float p_m[2], p_m_0[2];
    int32_t m_id, m_id_f, m_id_kf, m_num;
    float m_m0[2];
    double n_m0;
    int32_t p_id, n_id, net_id, stereo_m_id;
    double stereo_rho, stereo_s_rho;
} edgehip_keyline;

/* Per-sequence tracker/mapper state: the locals of FirstThr (rebvo_first_t.cpp:92-94) and SecondThread
 * (rebvo_second_t.cpp:54-66) that persist from frame to frame, kept in HBM so that a whole frame can be
 * enqueued without a host round trip. */
typedef struct edgehip_seq_state {
    double tresh;               /* detector threshold (P-controller state) */
    double V[3], W[3];          /* velocity / rotation estimate carried to the next frame */
    double P_V[9], P_W[9];      /* RVel, RW0 of the last Minimizer_RV */
    double R[9];                /* back-rotation of the last frame pair */
    double Pose[9], Pos[3];     /* integrated pose */
    double Kp, P_Kp, K;
    double s_rho_q;             /* EstimateQuantile result of the last frame pair */
    double score, rel_error, rel_error_score;
    double t_prev, dt;
    float retuned_thresh;       /* edge_finder::reTunedThresh of the newest slot */
    int32_t l_kl_num;           /* KeyLines on the last edge map (P-controller input) */
    int32_t frame;              /* frames detected so far */
    int32_t klm_fwd;            /* KeyLines of the new edge map that received a forward match.  (edge_tracker::FordwardMatch returns the
                                   number of assignments it made, the ones it later overwrote on a double match included; SecondThread
                                   overwrites that value with directed_matching's before anything reads it, rebvo_second_t.cpp:354 / 410.) */
    int32_t klm_num, kf_matchs; /* directed_matching: matched KeyLines, key-frame matches among them */
    int32_t estimation_ok;
    int32_t minimizer_evals;    /* TryVelRot evaluations spent on the last frame pair */
} edgehip_seq_state;

/* What SecondThread leaves in PipeBuffer/NavData per frame (rebvo_second_t.cpp:550-606). */
typedef struct edgehip_nav {
    double t, dt;
    double V[3], W[3], P_V[9], P_W[9];
    double Rot[9], RotLie[3], Vel[3], Pose[9], PoseLie[3], Pos[3];
    double Kp, RKp, s_rho_q, tresh, score, rel_error, rel_error_score;   /* tresh: FirstThr's threshold state behind the frame's detection(s) —
                                                                           with a stereo rig, behind the pair image's (rebvo_first_t.cpp:266-290) */
    float retuned_thresh;
    int32_t kn, klm_fwd, klm_num, kf_matchs, estimation_ok, frame, minimizer_evals;
} edgehip_nav;

/* ---- IMU branch on the device (ImuMode > 0 for whole batches) -------------------------------------------------------
 * The &IMU parameters REBVO::SecondThread uses (include/rebvo/rebvo.h:172-199; GlobalConfig_EuRoC:107-140). */
typedef struct edgehip_imu_params {
    double giro_meas_std, giro_bias_std;       /* GiroMeasStdDev, GiroBiasStdDev */
    int32_t init_bias, init_bias_frame_num;    /* InitBias, InitBiasFrameNum */
    double bias_init_guess[3];                 /* BiasHintX/Y/Z */
    double acel_meas_std, g_module, g_module_uncer, g_uncert, vbias_std;   /* AcelMeasStdDev, g_module, g_module_uncer, g_uncert, VBiasStdDev */
    double scale_std_mult, scale_std_max, scale_std_init;                  /* ScaleStdDevMult, ScaleStdDevMax, ScaleStdDevInit */
} edgehip_imu_params;
/* rebvo::IntegratedImuData (include/UtilLib/imugrabber.h:57-69): what ImuGrabber::GrabAndIntegrate hands the tracker
 * for the interval between two frames. */
typedef struct edgehip_imu_integrated {
    int32_t n, pad;
    double dt, Rot[9], giro[3], acel[3], comp[3], dgiro[3], cacel[3];
} edgehip_imu_integrated;
/* What the IMU branch adds to the per-frame record: NavData's IMU fields (rebvo.h:292-308) and the IMUState members the
 * reference logs (rebvo_second_t.cpp:550-606). */
typedef struct edgehip_nav_imu {
    double Rot[9], RotLie[3], RotGiro[3], Vel[3], Pose[9], PoseLie[3], Pos[3], g[3];
    double scale, dt, K, Kp, RKp, s_rho_q;
    double Vg[3], Bg[3], dVv[3], dWv[3], Vgv[3], Vgva[3], Av[3], As[3], X[7], b_est[3], u_est[3];
    int32_t kn, klm_num, estimation_ok, init;
} edgehip_nav_imu;

/* ---- lifetime -------------------------------------------------------------------------------------- */
/* Replaces the per-slot `new sspace / new edge_tracker / new global_tracker` of REBVO::construct
 * (src/rebvo/rebvo.cpp:297-312).  `device` is the HIP device ordinal. */
int edgehip_create(const edgehip_params *params, int nseq, int nslots, int device, edgehip_ctx **out);
int edgehip_destroy(edgehip_ctx *ctx);
const char *edgehip_last_error(void);
int edgehip_abi_version(void);
/* 1 if the library was built with `make EXPERIMENTS=1`: it then also holds the alternative kernels that measured slower than the
 * defaults and reads their EDGEHIP_* switches (timing experiments; the tests of those paths need such a build). */
int edgehip_experiments(void);
/* Block the caller until everything enqueued so far has finished. */
int edgehip_sync(edgehip_ctx *ctx);
/* The hipStream_t the tracker / mapper kernels (and, for whole batches, everything) are launched on, as an opaque pointer (for event
 * timing by the caller).  For batches of fewer sequences than the device has CUs the detection of a frame (stage A) runs on a second
 * stream of the context, beside the tracking and mapping of the frame before, unless EDGEHIP_OVERLAP=0 is set when the context is
 * created; edgehip_sync and the read-back calls wait for both. */
void *edgehip_stream(edgehip_ctx *ctx);
/* Device box-filter widths chosen for (sigma0, ksigma), as iigauss::iigauss does
 * (src/mtracklib/iigauss.cpp:43-81): out[0..2] filter0, out[3..5] filter1. */
int edgehip_box_widths(edgehip_ctx *ctx, int out[6]);

/* ---- frame input ----------------------------------------------------------------------------------- */
/* Copy RGB24 frames (host memory, [count][h][w][3]) into slot `slot` of sequences [seq_first,
 * seq_first+count): the `(*pbuf.imgc) = data` of rebvo_first_t.cpp:250.  Asynchronous through a pinned
 * staging buffer; the source may be reused when the call returns. */
int edgehip_upload_rgb(edgehip_ctx *ctx, int slot, const uint8_t *rgb24, int seq_first, int count);
/* Same, from device memory ([nseq][h][w][3], all sequences), device-to-device on the context stream. */
int edgehip_upload_rgb_device(edgehip_ctx *ctx, int slot, const void *rgb24_dev);
/* Host frames without the staging copy: the source is page-locked memory from edgehip_alloc_pinned (count frames for
 * sequences seq_first .. seq_first+count-1) and is read by an asynchronous copy — leave it untouched until the next
 * call that synchronises (edgehip_sync, edgehip_read_nav, ...) or write the next frames into a second buffer.
 * The copy is enqueued on a dedicated upload stream: it runs under stage A and stages B/C of the frames before, waits
 * by itself for the frame that last used the slot, and stage A of the slot waits for it. */
int edgehip_alloc_pinned(size_t bytes, void **out);
int edgehip_free_pinned(void *p);
int edgehip_upload_rgb_pinned(edgehip_ctx *ctx, int slot, const uint8_t *rgb24_pinned, int seq_first, int count);
/* Block the caller until the page-locked sources of every *_pinned upload enqueued so far have been read (the copies on the upload
 * stream are done) — the point at which a camera ring may hand the buffers back to the application
 * (cam_pipe.ReleaseBuffer, src/VideoLib/customcam.cpp:70-76).  The frames' processing is NOT waited for. */
int edgehip_upload_sync(edgehip_ctx *ctx);
/* The same for the *_pinned uploads into ONE slot: copies into other slots enqueued behind them keep running.  A camera ring whose
 * frame k+1 is already going up behind frame k hands frame k's buffers back with this (rebvo_amd/host/src/batch_group.cpp). */
int edgehip_upload_wait(edgehip_ctx *ctx, int slot);

/* Bench/replay helper: frame pool resident in HBM ([pool_frames][h][w][3]); sequence s takes frame
 * idx[s] (host array, nseq entries).  One gather kernel on the context stream. */
int edgehip_upload_rgb_indexed(edgehip_ctx *ctx, int slot, const void *pool_dev, int pool_frames, const int32_t *idx);
/* The same selection without the copy: stage A of `slot` reads sequence s's frame directly at
 * pool_dev + idx[s] * w*h*3 (what ConvertRGB2BW does with the camera buffer, rebvo_first_t.cpp:259).  The pool must
 * stay valid and unchanged until that stage A has run, and must extend at least 16 bytes past its last frame (pixels
 * are fetched as aligned 8-byte words).  Any edgehip_upload_rgb* call on the slot returns it to its own storage. */
int edgehip_bind_rgb_indexed(edgehip_ctx *ctx, int slot, const void *pool_dev, int pool_frames, const int32_t *idx);
/* 8-bit mono frames, 1 byte per pixel: what a mono camera or the EuRoC data set delivers.  The reference's DataSetCam expands
 * such an image to RGB24 with r = g = b (src/VideoLib/datasetcam.cpp:109-171) because Image<float>::ConvertRGB2BW
 * (include/VideoLib/image.h:197-203) wants RGB24; b + g + r is then 3 v, and that is what the first load of stage A computes
 * from the 8-bit frame directly — bit-identical results at a third of the bytes over PCIe and out of HBM.  Same three forms
 * as the RGB24 uploads: pageable host memory (staged), page-locked host memory (asynchronous, on the upload stream), frames of
 * a device-resident pool read in place.  A slot holds whichever format was uploaded or bound to it last. */
int edgehip_upload_grey8(edgehip_ctx *ctx, int slot, const uint8_t *grey8, int seq_first, int count);
int edgehip_upload_grey8_pinned(edgehip_ctx *ctx, int slot, const uint8_t *grey8_pinned, int seq_first, int count);
int edgehip_bind_grey8_indexed(edgehip_ctx *ctx, int slot, const void *pool_dev, int pool_frames, const int32_t *idx);

/* ---- stage A: scale space + KeyLine extraction ----------------------------------------------------- */
/* Image<float>::ConvertRGB2BW + sspace::build + edge_finder::detect + reEstimateThresh for every
 * sequence's slot `slot` (rebvo_first_t.cpp:259-272; sspace.cpp:52-85; edge_finder.cpp:67-405).
 * Reads and updates seq_state.tresh / l_kl_num exactly as detect()'s UpdateThresh does. */
int edgehip_stage_a(edgehip_ctx *ctx, int slot);
/* Number of KeyLines per sequence in `slot` (edge_finder::KNum).  Synchronises.  kn_out[nseq]. */
int edgehip_get_kn(edgehip_ctx *ctx, int slot, int32_t *kn_out);

/* ---- stage B: tracker ------------------------------------------------------------------------------ */
/* edge_tracker::EstimateQuantile(RHO_MIN,RHO_MAX,pct,nbins) on slot (rebvo_second_t.cpp:172;
 * edge_tracker.cpp:1148-1186).  Result in seq_state.s_rho_q. */
int edgehip_quantile(edgehip_ctx *ctx, int slot, double s_rho_min, double s_rho_max, double pct, int nbins);
/* global_tracker::build_field (rebvo_second_t.cpp:177; global_tracker.cpp:61-105).  min_mod < 0 takes
 * each sequence's retuned threshold of that slot (what the reference passes: new_buf.ef->getThresh()). */
int edgehip_build_field(edgehip_ctx *ctx, int slot, int radius, float min_mod);
/* One global_tracker::TryVelRot<double,ReWeight,ProcJF,false> evaluation (global_tracker.cpp:289-543) of
 * the old slot's KeyLines against the new slot's field, at state X[nseq][6].  Residual buffers are
 * device-resident and named by index 0..2 (Res0/Res1/Rest of Minimizer_RV, :611-612); resid_in < 0 means
 * all-zero.  out[nseq][43] = JtJ(36, row-major, sign-fixed and symmetrised) | JtF(6) | score.
 * Parity: every per-KeyLine value (projection, match, residual, Huber weight k/|r|, q_rho, the seven quotients by q_rho) is formed
 * by the reference's own sequence of IEEE operations (:363-463; ne10wrapper.h:414-424), so the residual memory is bit-identical;
 * the 28 sums are added in another (fixed) pair-wise tree than ne10wrapper.h:333-362 and agree to ~4e-16 relative.
 * Synchronises. */
int edgehip_try_velrot(edgehip_ctx *ctx, int slot_new, int slot_old, const double *X, int reweight, int procjf,
                       double match_thresh, const double *s_rho_min, uint32_t match_num_thresh, double k_huber,
                       int resid_in, int resid_out, double *out);
/* Copy a residual buffer to the host (resid[nseq][cap] with cap = max_points).  Synchronises. */
int edgehip_download_resid(edgehip_ctx *ctx, int which, double *resid);
/* global_tracker::Minimizer_RV<double,false> (rebvo_second_t.cpp:346; global_tracker.cpp:580-819): the
 * whole Levenberg-Marquardt loop runs on the device (evaluate kernels + a one-wave solve kernel between
 * them, no host round trip).  Reads seq_state.V/W/s_rho_q, writes V, W, P_V, P_W, score, rel_error*. */
int edgehip_minimizer_rv(edgehip_ctx *ctx, int slot_new, int slot_old);
/* Which instantiation of the tracker edgehip_minimizer_rv / edgehip_process_frame run: 64 (default) = global_tracker::Minimizer_RV<double>,
 * what the reference runs on x86 (rebvo_second_t.cpp:346); 32 = Minimizer_RV<float> with TryVelRot<float, ...> (global_tracker.cpp:824), what
 * the reference runs when it is built with USE_NE10 (rebvo_second_t.cpp:339-343: NEON only does float).  Everything the reference declares
 * as T (P0, the transformed points, residuals, gradients, Jacobian rows, the 28 sums, JtJ / JtF / h / X) is then computed and rounded in
 * float; the uncertainty gate, q_rho, the 6x6 solves and the Levenberg-Marquardt scalars stay double, as there.  Results follow the
 * reference's float instantiation to float accuracy (the 28 float sums are added in another tree than PairWiseVAdd<float>):
 * tests/test_tracker_f32_gpu.py states the tolerance.  The depth filter, the matcher and the detector are not affected.  ImuMode 0 without
 * a stereo rig only, in either order: 32 is refused (EDGEHIP_ERR_STATE) after edgehip_imu_enable / edgehip_set_stereo_rig, and those two
 * are refused while the precision is 32 (nothing changes; set 64 first). */
int edgehip_set_tracker_precision(edgehip_ctx *ctx, int bits);
/* The 6x6 solve between two evaluations, n independent systems (A [n][36] row-major, b [n][6], h [n][6], host pointers):
 * svd_rule = 0: h = TooN::Cholesky<6>(A).backsub(b) (global_tracker.cpp:767-768); svd_rule = 1: h = TooN::SVD<>(A).backsub(b) with
 * its condition_no = 1e9 cut-off (global_tracker.cpp:660-661, 711-712; TooN/SVD.h:37, 179).  Exposed so that the parity tests can
 * feed the device ill-conditioned systems on either side of the cut-off; edgehip_minimizer_rv runs the same device function.
 * Synchronises. */
int edgehip_lm_solve(edgehip_ctx *ctx, const double *A, const double *b, int n, int svd_rule, double *h);

/* kfvo::Minimizer_RV_KF<double,false> with kfvo::TryVelRot<double,true,true,false> and global_tracker::Calc_f_J_Complete
 * (src/mtracklib/kfvo.cpp:1679-1825, 1389-1668; global_tracker.cpp:116-165) — the key-frame tracker of SURVEY section 8 row
 * f4: the KeyLines of slot_cur (the current frame, `klist`) against the field of slot_kf's KeyLines (the key frame's
 * global_tracker), relative pose X = [translation, rotation] starting from X0, scale ratio Kr.  Reached in the reference
 * through kfvo::OptimizePosGT (kfvo.cpp:58-113), which has no caller upstream; built to the letter of the scope row and
 * checked against the reference's own function.  The field of slot_kf is (re)built inside the call; KeyLine m_id_f of
 * slot_cur is left as the last evaluation wrote it, mnum counts its non-negative entries (kfvo.cpp:76-82).  req/res are
 * host arrays of nseq entries.  Synchronises. */
typedef struct edgehip_kf_request {
    double X0[6];        /* BRelPos, BRelRotW (kfvo.cpp:63-69) */
    double Kr;           /* K / mkf.K */
    double max_s_rho;    /* s_rho_q */
} edgehip_kf_request;
typedef struct edgehip_kf_result {
    double X[6];
    double RRV[36];      /* Cholesky<6>(JtJ).get_inverse() */
    double score_ratio;  /* F / F0, the function's return value */
    double F, F0;
    int32_t evals, mnum;
} edgehip_kf_result;
int edgehip_minimizer_rv_kf(edgehip_ctx *ctx, int slot_kf, int slot_cur, const edgehip_kf_request *req, double match_mod,
                            double match_ang, double rho_tol, int iter_max, double reweight_distance, uint32_t match_num_thresh,
                            edgehip_kf_result *res);

/* global_tracker::Minimizer_V<double> (IMU branch, rebvo_second_t.cpp:223; global_tracker.cpp:1037-1093 with
 * TryVel :830-934 and Calc_f_J :178-219): translation-only Levenberg-Marquardt of the old slot's KeyLines (already
 * rotated by the gyro estimate) against the new slot's field.  V[nseq][3] in/out, s_rho_min[nseq], min_mod < 0
 * takes each sequence's retuned threshold of the OLD slot (old_buf.ef->getThresh()); RVel[nseq][9] and F[nseq]
 * may be NULL.  FrameCount is read, not incremented (as in the reference).  Synchronises. */
int edgehip_minimizer_v(edgehip_ctx *ctx, int slot_new, int slot_old, double *V, const double *s_rho_min, float min_mod,
                        double match_thresh, int iter_max, uint32_t match_num_thresh, double reweight_distance,
                        double *RVel, double *F);

/* ---- stage C: matching + mapping ------------------------------------------------------------------- */
/* edge_tracker::FordwardMatch (rebvo_second_t.cpp:354; edge_tracker.cpp:380-436). */
int edgehip_forward_match(edgehip_ctx *ctx, int slot_old, int slot_new);
/* edge_tracker::rotate_keylines (rebvo_second_t.cpp:369; edge_tracker.cpp:42-76).  R == NULL rotates
 * each sequence by exp(seq_state.W) and stores the back-rotation in seq_state.R (:360-361). */
int edgehip_rotate_keylines(edgehip_ctx *ctx, int slot, const double *R /* [nseq][9] or NULL */);
/* edge_tracker::directed_matching (rebvo_second_t.cpp:410; edge_tracker.cpp:302-374, 158-295) with
 * V, P_V, R taken from seq_state; the match count lands in seq_state.klm_num / kf_matchs. */
int edgehip_directed_matching(edgehip_ctx *ctx, int slot_new, int slot_old);
/* TEST SUPPORT ONLY, not part of the product surface: the matching of a frame that matches in one pass (no stereo pair, no IMU
 * branch), on uploaded lists.  Enqueues exactly what edgehip_process_frame enqueues there: FordwardMatch's arbitration keys of slot_old
 * (the keys the tracker's last evaluation posts in a frame), rotate_keylines(exp(seq_state.W)) out of place together with the
 * arbitration (seq_state.R receives the back-rotation, :360-361), then directed_matching with FordwardMatch's copy inside, with V, P_V
 * from seq_state.  fill != 0: the ten matching fields of slot_new are taken as unwritten (a detector that left them to this call) and
 * every KeyLine gets them: the match's, the forward match's, or a fresh KeyLine's (edge_finder.cpp:176-196).  Counts land in
 * seq_state.klm_fwd / klm_num / kf_matchs (added to what is there).  slot_old keeps its turned values beside its arrays until the next
 * stage-level call or download reads it.  EDGEHIP_ERR_STATE in a context that does not match in one pass (stereo_available). */
int edgehip_match_one_pass(edgehip_ctx *ctx, int slot_new, int slot_old, int fill);
/* Regularize_1_iter + UpdateInverseDepthKalman fused (rebvo_second_t.cpp:453, 460;
 * edge_tracker.cpp:87-148, 695-724, 954-1055).  do_regularize/do_ekf select either half (tests). */
int edgehip_regularize_ekf(edgehip_ctx *ctx, int slot, int do_regularize, int do_ekf);
/* edge_tracker::ExtRotVel (IMU branch, rebvo_second_t.cpp:237; edge_tracker.cpp:1207-1296): linear 6-DoF
 * roto-translation increment from the forward matches of `slot` (the new edge map after edgehip_forward_match),
 * given the translation estimate vel[nseq][3].  X[nseq][6]; Wx[nseq][36] = Phi^T Phi and Rx[nseq][36] = its
 * pseudo inverse may be NULL; ok[nseq] (may be NULL) is the function's return value (false on a NaN result).
 * The per-KeyLine rows and the 27 sums run on the device, the 6x6 SVD solve on the host.  Synchronises. */
int edgehip_ext_rot_vel(edgehip_ctx *ctx, int slot, const double *vel, double loc_unc, double hub_reweight, double *X,
                        double *Wx, double *Rx, int32_t *ok);
/* EstimateReScalingOpt (rebvo_second_t.cpp:487; edge_tracker.cpp:1104-1140) -> seq_state.Kp, P_Kp.
 * Parity: the five dependent weighted sums are block reductions in a fixed order (the reference adds KeyLine by KeyLine) and
 * the per-KeyLine divisions are reciprocal + Newton steps (an ulp or two each), so Kp — and every rho that DoReScaling
 * multiplies by it — follows the reference to about 1e-10 relative, not bit for bit (tests/test_stage_c_gpu.py: 1e-10). */
int edgehip_rescale(edgehip_ctx *ctx, int slot);

/* ---- stereo depth (REBVO/StereoAvaiable, experimental upstream) ------------- */
/* Intrinsics of the camera whose frames go into `slot` when they differ from the context's (the pair camera of a
 * stereo rig, cam_stereo of rebvo.cpp:202-216): stage A of that slot forms p_m with this principal point, and the
 * stereo search projects with this focal length.  zfm is taken as (float)((zfx + zfy) / 2), like cam_model. */
int edgehip_set_slot_camera(edgehip_ctx *ctx, int slot, double ppx, double ppy, double zfx, double zfy);
/* edge_tracker::directed_matching_stereo (rebvo_second_t.cpp:471; edge_tracker.cpp:580-618 with search_match_stereo
 * :453-571 and getDepthFromStereo :622-668): every KeyLine of `slot` walks, in the pair slot's edge mask, the segment
 * its depth interval [rho - s_rho, rho + s_rho] projects to through p1 = R p0 + t, keeps a match only when it is
 * unique (or all candidates lie within loc_unc of each other) and triangulates stereo_rho / stereo_s_rho from it.
 * t[3], R[9] are shared by all sequences; nmatch[nseq] (may be NULL) returns the function's result per sequence.
 * q_abs / q_rel are accepted and unused, as in the reference.  Needs params.stereo_available.  Synchronises. */
int edgehip_directed_matching_stereo(edgehip_ctx *ctx, int slot, int slot_pair, const double *t, const double *R,
                                     double min_thr_mod, double min_thr_ang, double max_radius, double loc_unc,
                                     double q_abs, double q_rel, double loc_unc_model, int32_t *nmatch);
/* edge_tracker::fuseStereoDepth (rebvo_second_t.cpp:484; edge_tracker.cpp:670-688): rho0/s_rho0 = rho/s_rho, then the
 * information-weighted mean with the stereo depth where a stereo match exists. */
int edgehip_fuse_stereo_depth(edgehip_ctx *ctx, int slot);
/* Stereo inside edgehip_process_frame (what SecondThread does with StereoAvaiable, rebvo_second_t.cpp:410, 465-486):
 * the last ring slot becomes the pair slot (the frame ring then cycles through the others); the caller uploads the pair
 * image into it before every edgehip_process_frame, which then also runs stage A on it (after the main image, sharing
 * the detector threshold state like rebvo_first_t.cpp:283-289) and, after the depth EKF, directed_matching_stereo with
 * (t, R, max_radius) and the context's matching thresholds, fuseStereoDepth, and Kp = 1 in place of
 * EstimateReScalingOpt.  Set edgehip_set_slot_camera for the pair slot first when the cameras differ.
 * slot_pair < 0 switches the rig off.  edgehip_get_stereo_matches: stereo_match_num of the last frame.  Synchronises. */
int edgehip_set_stereo_rig(edgehip_ctx *ctx, int slot_pair, const double *t, const double *R, double max_radius);
int edgehip_get_stereo_matches(edgehip_ctx *ctx, int32_t *nmatch);

/* ---- whole frame ------------------------------------------------------------------------------------ */
/* Everything FirstThr + SecondThread (ImuMode==0) do for one new frame of every sequence, on the
 * context's current ring slot, enqueued back to back without host synchronisation: stage A on the new
 * slot, then (from the second frame on) quantile, build_field, Minimizer_RV, FordwardMatch, rotate,
 * directed_matching, Regularize, EKF, rescale and the pose integration of rebvo_second_t.cpp:550-551.
 * The frame must have been uploaded into edgehip_next_slot() first.  t[nseq] = frame time stamps.
 * Uploads and stage A are enqueued on a second HIP stream; with EDGEHIP_OVERLAP=1 in the environment at
 * edgehip_create() time, stage A of this frame only waits for the B/C work that still reads the slot it overwrites
 * and so runs under the tracking/mapping of the previous frame (the reference's T0 || T1 pipelining).
 * With EDGEHIP_GRAPH=1 the launches of a frame are captured into HIP graphs (one per ring-slot / FrameCount-row
 * combination) the first time they occur and replayed afterwards. */
int edgehip_process_frame(edgehip_ctx *ctx, const double *t);
int edgehip_next_slot(edgehip_ctx *ctx);
int edgehip_cur_slot(edgehip_ctx *ctx);
/* Per-sequence record of the last processed frame.  Synchronises.  nav[nseq]. */
int edgehip_read_nav(edgehip_ctx *ctx, edgehip_nav *nav);
/* ImuMode > 0 for every sequence of the context (rebvo_second_t.cpp:54-94 set-up, :182-336 tracker + filters, :519-544
 * pose): from the next frame on edgehip_process_frame takes the IMU branch — gyro pre-rotation, Minimizer_V, FordwardMatch,
 * ExtRotVel, BiasCorrect, rotate, the mapper, the scale filter and the gravity-aligned pose — entirely on the device, no
 * host synchronisation, one thread per sequence for the 3..11-dimensional filters.  Call before the first frame. */
int edgehip_imu_enable(edgehip_ctx *ctx, const edgehip_imu_params *imu);
/* The integrated IMU data of the interval that ends with the NEXT edgehip_process_frame, one record per sequence
 * (ImuGrabber::GrabAndIntegrate stays with the caller: it is I/O).  Asynchronous; the records are copied before return. */
int edgehip_set_imu(edgehip_ctx *ctx, const edgehip_imu_integrated *per_seq);
/* The IMU part of the newest frame's record, one per sequence (synchronises like edgehip_read_nav). */
int edgehip_read_nav_imu(edgehip_ctx *ctx, edgehip_nav_imu *out);
/* Keep the last `len` per-frame records of every sequence in HBM (ring indexed by frame number) so that a
 * replay can run many frames without reading back; edgehip_read_nav_log copies records of frames
 * [first, first+count) as out[count][nseq]; the frames must have been enqueued (EDGEHIP_ERR_STATE before the first one).
 * Threading: a context is driven by ONE thread at a time — with this exception: edgehip_read_nav_log may be called from a
 * second thread while the first keeps enqueueing frames (the nav gather of a multi-GPU replay does).  It waits, on a stream
 * of its own, for the newest frame it is asked for — not for frames enqueued behind it, so a caller may keep frames in flight
 * and read the records one or two frames late — and never touches the context's frame streams (which may be capturing a
 * frame graph).  edgehip_set_nav_log itself belongs to the driving thread, with no reader active. */
int edgehip_set_nav_log(edgehip_ctx *ctx, int len);
int edgehip_read_nav_log(edgehip_ctx *ctx, int first, int count, edgehip_nav *out);
/* The same records into DEVICE memory of the context's GPU (out_dev[count][nseq] edgehip_nav, e.g. a tensor the caller's RCCL
 * communicator sends from): the multi-GPU nav gather of SURVEY.md section 8(e) takes its payload from HBM to the wire without a
 * host bounce (rebvo_amd/shard.py NavMover).  Same waiting, threading and range rules; the copy is complete on return. */
int edgehip_read_nav_log_device(edgehip_ctx *ctx, int first, int count, void *out_dev);
/* ImuMode > 0: the IMU part of the logged records (what edgehip_read_nav_imu returns for the newest frame), frames [first, first+count)
 * as out[count][nseq] — same ring, same waiting and threading rules as edgehip_read_nav_log.  A caller that keeps frames in flight
 * (a batch group of ImuMode = 1 / 2 objects, rebvo_amd/host/src/batch_group.cpp) reads both halves of frame k while k+1 and k+2 run. */
int edgehip_read_nav_imu_log(edgehip_ctx *ctx, int first, int count, edgehip_nav_imu *out);
/* With a stereo rig (edgehip_set_stereo_rig): stereo_match_num (rebvo_second_t.cpp:471-477, what edgehip_get_stereo_matches returns for the
 * newest frame) of the logged frames [first, first+count) as out[count][nseq] — same ring, same waiting and threading rules as
 * edgehip_read_nav_log; 0 for a sequence's first frame.  A batch group of StereoAvaiable objects reads it with frames in flight. */
int edgehip_read_stereo_matches_log(edgehip_ctx *ctx, int first, int count, int32_t *out);
/* Restart every sequence from scratch: state as after edgehip_create (thresholds, priors, pose, frame
 * counters) and an empty ring.  Not something the reference does at run time (it would re-construct REBVO). */
int edgehip_reset(edgehip_ctx *ctx);
/* REBVO::Reset() as SecondThread executes it after a frame (rebvo_second_t.cpp:609-620): depth reset of the
 * newest edge map (rho = RhoInit, s_rho = RHO_MAX for every KeyLine), Pose = I, Pos = V = W = 0.  Everything
 * else (detector threshold, K, frame counters) carries on.  seq < 0 applies it to all sequences. */
int edgehip_depth_reset(edgehip_ctx *ctx, int seq);
/* The same on an explicit ring slot, for callers that drive the stages one by one (the host's IMU branch) instead of
 * through edgehip_process_frame. */
int edgehip_depth_reset_slot(edgehip_ctx *ctx, int seq, int slot);

/* ---- state / data exchange (callback consumers, parity tests) ---------------------------------------- */
int edgehip_get_state(edgehip_ctx *ctx, int seq, edgehip_seq_state *out);       /* synchronises */
int edgehip_set_state(edgehip_ctx *ctx, int seq, const edgehip_seq_state *in);
int edgehip_get_framecount(edgehip_ctx *ctx, int seq, int slot, uint32_t *fc);  /* global_tracker::FrameCount */
int edgehip_set_framecount(edgehip_ctx *ctx, int seq, int slot, uint32_t fc);
/* AoS KeyLine list + img_mask_kl of one sequence/slot, as the output callback sees them
 * (PipeBuffer::ef, include/rebvo/rebvo.h:312-351).  kl has room for max_points entries; mask (h*w int32)
 * may be NULL.  Synchronises.  Returns kn through *kn_out.
 * The OLD slot of a frame edgehip_process_frame() has run holds what old_buf.ef holds after rotate_keylines (rebvo_second_t.cpp:369):
 * the frame driver keeps the turned p_m / m_m / rho / s_rho next to the slot's arrays for its own matching kernel and brings them in
 * when anybody else — this call, any stage-level entry point — asks for the slot. */
int edgehip_download_keylines(edgehip_ctx *ctx, int seq, int slot, edgehip_keyline *kl, int32_t *mask,
                              int32_t *kn_out);
/* The same lists for several sequences of one slot in ONE packing kernel and one copy per list (the output callbacks of a batch of cameras,
 * rebvo_amd/host/src/batch_group.cpp): seqs[n] sequence indices, kl[n] destinations of max_points entries each, kn_out[n].  Record for record what
 * edgehip_download_keylines returns (no mask).  Synchronises. */
int edgehip_download_keylines_batch(edgehip_ctx *ctx, int slot, int n, const int32_t *seqs, edgehip_keyline *const *kl, int32_t *kn_out);
/* Output callbacks at full pipeline depth (round 6; the consumer: setOutputCallback, include/rebvo/rebvo.h:595-609, called by
 * REBVO::ThirdThread, src/rebvo/rebvo_third_t.cpp:174 — every real user of the surface has one, ros/src/rebvo_ros/src/rebvo_nodelet.cpp:146-242).
 * A callback gets frame k-1's edge map as frame k's tracking left it: the OLD slot of the frame processed last.
 *   edgehip_export_keylines  right after edgehip_process_frame(k): packs that slot's KeyLines of sequences seqs[n] as AoS records into a
 *                            device-side staging ring, in-stream behind the frame (no synchronisation; the ring slot itself is free for
 *                            the frame after next).  Returns a ticket; at most four may be outstanding.
 *   edgehip_export_fetch     once the caller knows the lists' lengths (kn[j] = edgehip_nav::kn of frame k-1 for seqs[j]): enqueues the copies
 *                            of exactly kn[j] records into dst[j] on a stream of their own (page-locked destinations — edgehip_register_host —
 *                            are written by DMA under the frames that follow; pageable ones work, slower).  Does not block.
 *   edgehip_export_wait      blocks until the ticket's copies have landed and releases the ticket (never fetched: waits for the pack itself, as edgehip_ros_export_wait does).
 * Record for record what edgehip_download_keylines_batch returns for the same slot at the same point. */
int edgehip_export_keylines(edgehip_ctx *ctx, int n, const int32_t *seqs, int *ticket_out);
int edgehip_export_fetch(edgehip_ctx *ctx, int ticket, const int32_t *kn, edgehip_keyline *const *dst);
int edgehip_export_wait(edgehip_ctx *ctx, int ticket);
/* Page-lock host memory the caller owns, in place (hipHostRegister), so that edgehip_download_keylines_batch copies straight into
 * it: a destination inside a registered range skips the library's staging buffer and the host memcpy behind it (2.4 MB per list of
 * 14 k KeyLines).  What a batch group does with the KeyLine arrays of the members that have an output callback
 * (PipeBuffer::ef of setOutputCallback, include/rebvo/rebvo.h:595-609).  Unregister before the memory is freed. */
int edgehip_register_host(void *p, size_t bytes);
int edgehip_unregister_host(void *p);
/* Inject a KeyLine list (+ mask) into a slot: stage-isolated parity tests. */
int edgehip_upload_keylines(edgehip_ctx *ctx, int seq, int slot, const edgehip_keyline *kl, int32_t kn,
                            const int32_t *mask, float retuned_thresh);
/* Planes of the scale space (debug_planes must be set): which = 0 img0, 1 img1, 2 dog, 3 dx, 4 dy.
 * out[h*w] float.  Synchronises. */
int edgehip_download_plane(edgehip_ctx *ctx, int seq, int which, float *out);
/* Auxiliary field of the tracker in the reference's {dist, ikl} form (global_tracker.h:33-36); out[h*w*2].
 * The tracker only ever reads ikl, so the device keeps a 2-byte KeyLine-index plane; dist is stored as well (and
 * returned here) when params.debug_planes is set, otherwise it is reported as -1 (0 where the pixel is empty). */
int edgehip_download_field(edgehip_ctx *ctx, int seq, int32_t *out);
/* The undistortion map edgehip_create() builds for `params` (host-only, needs no device), in the reference's
 * undistMapPoint form (image_undistort.h:41-47): inx[h*w*4] valid taps first, -1 beyond `num`; iw[h*w*4]. */
int edgehip_build_undistort_map(const edgehip_params *params, int32_t *inx, int32_t *iw);
/* Debug: the undistorted RGB24 frame that stage A consumed for sequence `seq` in `slot`, recomputed on the
 * device with the same integer arithmetic (what PipeBuffer::imgc holds after rebvo_first_t.cpp:231). */
int edgehip_download_undistorted(edgehip_ctx *ctx, int seq, int slot, uint8_t *rgb24);

/* ---- dense depth fill (the visualizer's depth_filler) ----------------------------------------------------------------
 * The inverse-depth grid that depth_filler interpolates from a KeyLine list (src/visualizer/depth_filler.cpp), in the order the
 * reference's callers run it — ResetData, FillEdgeData, InitCoarseFine, Integrate(IterNum).  FillEdgeData has two overloads with
 * different gates.  The key-frame path fills from the tracker's list per key frame, FillEdgeData(edge_tracker&, ThreshRelRho,
 * ThreshMatchNum, discart) (src/mtracklib/keyframe.cpp:171-184, app/kf_visualizer/main.cpp:106): that is edgehip_depth_fill.  The
 * visualizer fills per received frame from the quantised wire records, FillEdgeData(net_keyline*, kn, p_off, ...)
 * (src/visualizer/visualizer.cpp:303, 436-440): that is edgehip_depth_fill_net, below.  Grid gw x gh = (w / block_w) x (h / block_h), cell
 * (x, y) at y * gw + x.  rho, s_rho and fixed equal the reference's bit for bit (fp64 throughout, the reference's order of
 * operations; tests/depth_fill_port.py restates it) — except the sign and payload of a NaN the arithmetic creates (inf - inf,
 * 0 * inf): the GPU's default NaN is positive, x86 SSE's negative.  NaNs a KeyLine carries in pass through unchanged.  Two departures, both where the reference has no defined result or writes
 * through its argument:
 *   - a KeyLine whose cell index y * gw + x lands past the grid is dropped.  (With w % block_w != 0 a KeyLine in the partial
 *     column gets x == gw and lands in the first cell of the next row, as in the reference; on the last row the reference writes
 *     past its buffer.)
 *   - FillEdgeData sets kl.rho = kl.rho0 in the tracker's list for a negative rho it accepts (discard = 0); the fill only reads. */
typedef enum edgehip_bound_mode {
    EDGEHIP_BOUND_NONE = 0,      /* depth_filler::BOUND_NONE: every cell takes the coarse-fine / neighbour mean (both callers use this) */
    EDGEHIP_BOUND_CORNERS = 1,   /* BOUND_CORNERS: the four corner cells keep s_rho = 2 RHO_MAX */
    EDGEHIP_BOUND_FULL = 2       /* BOUND_FULL: every border cell keeps s_rho = 2 RHO_MAX */
} edgehip_bound_mode;
typedef struct edgehip_depth_fill_params {
    int32_t block_w, block_h;    /* &DepthFiller PixelBlockSize (app/kf_visualizer/main.cpp:56; the visualizer fixes 10, visualizer.cpp:303) */
    int32_t iter_num;            /* IterNum: Integrate1Step sweeps (main.cpp:59, visualizer.cpp:561); 0 = coarse-fine only */
    double thresh_rel_rho;       /* ThreshRelRho: KeyLines with s_rho / rho > this are skipped (main.cpp:57, visualizer.cpp:559) */
    int32_t thresh_match_num;    /* ThreshMatchNum: m_num below this counts as unmatched (main.cpp:58, visualizer.cpp:560) */
    int32_t bound_mode;          /* edgehip_bound_mode (depth_filler's bound_modes) */
    int32_t discard;             /* FillEdgeData's discart: != 0 skips unmatched KeyLines, 0 folds them with weight 1 / RHO_MAX^2 */
} edgehip_depth_fill_params;
/* Replaces the construction `depth_filler(cam, {bw, bh}, bound_mode)` (depth_filler.cpp:30-39) for every sequence of the context:
 * allocates the grids and scratch (about 17 B per cell and 8 B per KeyLine of capacity, per sequence).  params == NULL frees them.
 * EDGEHIP_ERR_ARG for a block size < 1, iter_num < 0, a grid smaller than 1x1 or an unknown bound_mode. */
int edgehip_depth_fill_enable(edgehip_ctx *ctx, const edgehip_depth_fill_params *params);
/* depth_filler::gridSize (depth_filler.h:95-97).  EDGEHIP_ERR_STATE if the fill is not enabled. */
int edgehip_depth_fill_size(edgehip_ctx *ctx, int32_t *gw, int32_t *gh);
/* ResetData + FillEdgeData + InitCoarseFine + Integrate (depth_filler.cpp:41-56, 113-163, 233-355) on the KeyLines of `slot`, for every
 * sequence, in-stream (no synchronisation).  Reads exactly what edgehip_download_keylines returns for the slot — for the OLD slot of
 * a processed frame, its turned rho / s_rho (see there) — and writes nothing but the grids.  EDGEHIP_ERR_STATE if not enabled. */
int edgehip_depth_fill(edgehip_ctx *ctx, int slot);
/* The grid of sequence `seq` from the last edgehip_depth_fill: rho[gh*gw], s_rho[gh*gw] (depth_filler::data[].rho / .s_rho) and
 * fixed[gh*gw] (1 where KeyLines landed: df_point::fixed), row-major.  Any of the three may be NULL.  Synchronises. */
int edgehip_download_depth_grid(edgehip_ctx *ctx, int seq, double *rho, double *s_rho, uint8_t *fixed);
/* The same for n sequences seqs[n] in one call (the output callbacks of a batch group): rho[j], s_rho[j], fixed[j] per request, any
 * array or entry may be NULL.  Synchronises once. */
int edgehip_download_depth_grids_batch(edgehip_ctx *ctx, int n, const int32_t *seqs, double *const *rho, double *const *s_rho,
                                       uint8_t *const *fixed);

/* ---- the wire-format edge map (net_keyline) and the visualizer's fill from it ---------------------------------------------
 * The reference publishes every frame's edge map as 15-byte net_keyline records (include/CommLib/net_keypoint.h:35-62), packed by
 * copy_net_keyline + copy_net_keyline_nextid (src/CommLib/net_keypoint.cpp:29-108) in its third thread
 * (src/rebvo/rebvo_third_t.cpp:189-203); its visualizer builds the dense depth from those records (visualizer.cpp:427-440).  Here the
 * records are packed on the device from the SoA KeyLines, for every sequence in one launch: 15 B per KeyLine leave the device instead
 * of the 168-byte record. */
#pragma pack(push, 1)
typedef struct edgehip_net_keyline {   /* rebvo::net_keyline, byte for byte */
    uint16_t qx, qy;        /* round(c_p) */
    uint16_t rho, s_rho;    /* max(clamp_ushort(NET_RHO_SCALING * v / k_prof), 1), NET_RHO_SCALING = 10000 */
    int32_t n_kl;           /* record index of the next KeyLine on the edge, -1: none */
    uint8_t m_num;          /* clamp_uchar(m_num) */
    uint8_t flow_x, flow_y; /* extra.flow: matched displacement * 10 + 127, or the stereo disparity + 127 (the `gradient` arm is never written upstream) */
} edgehip_net_keyline;
#pragma pack(pop)
#ifdef __cplusplus
static_assert(sizeof(edgehip_net_keyline) == 15, "net_keyline is 15 bytes on the wire");
#else
_Static_assert(sizeof(edgehip_net_keyline) == 15, "net_keyline is 15 bytes on the wire");
#endif
/* The three fields of net_packet_hdr (net_keypoint.h:64-78) that describe the records (rebvo_third_t.cpp:192, 200, 202). */
typedef struct edgehip_net_header {
    int32_t kline_num;      /* records packed: min(kn, kl_size) */
    int32_t km_num;         /* NumMatches(): directed_matching's count of the frame processed last (edgehip_seq_state::klm_num when the
                               records were packed; the device keeps no count per slot) */
    float k;                /* the k_prof the records were scaled with, as float (net_hdr->k = pbuf.K) */
} edgehip_net_header;
/* Allocates the record store: nseq x kl_size records back to back (nseq * kl_size * 15 B, rounded up to 16) and nseq headers, all
 * zero.  kl_size is the reference's KEYLINE_MAX argument (rebvo_third_t.cpp:193, 197); it need not equal max_points.  kl_size == 0
 * frees the store.  EDGEHIP_ERR_ARG for kl_size < 0 or > EDGEHIP_KEYLINE_MAX; EDGEHIP_ERR_MEMORY when the allocation fails (the store
 * is then off; the context stays usable). */
int edgehip_net_enable(edgehip_ctx *ctx, int kl_size);
/* copy_net_keyline(*ef, pair, to, kl_size, k_prof) followed by copy_net_keyline_nextid(*ef, to, kl_size)
 * (net_keypoint.cpp:29-75, 79-108; rebvo_third_t.cpp:192-202) on the KeyLines of `slot`, for every sequence, in-stream (no
 * synchronisation).  KeyLine j is packed iff j < min(kn, kl_size), into record j.  slot_pair >= 0: the slot of the stereo pair's edge
 * map (needs params.stereo_available); extra.flow is then the disparity to KeyLine stereo_m_id of that slot (:45-58).  k_prof: host
 * array [nseq] of the scale each sequence's depths are divided by, or NULL for each sequence's edgehip_seq_state::K.  Fields are formed
 * by the reference's own operations (float / double as written there, clamp_ushort and clamp_uchar taking a float), so the records
 * equal the reference's byte for byte.  Departures, where the reference has no defined result:
 *   - n_kl of a KeyLine whose n_id was not packed in this call (n_id >= kline_num) is -1; the reference copies that KeyLine's
 *     net_id, which is stale from an earlier call.
 *   - a stereo_m_id past the KeyLine capacity counts as no match (flow 127, 127); the reference indexes the pair list with it.
 *   - converting a NaN (or a value past the integer range) to an integer has no defined result in C++; the kernel's conversions
 *     behave as an x86-64 build of the reference does for finite values and are otherwise unspecified.
 * Only the first kline_num * 15 bytes of a sequence's records are written.  EDGEHIP_ERR_STATE when the store is off, or with a pair
 * slot on a context without the stereo fields; EDGEHIP_ERR_ARG for a slot out of range or slot_pair == slot. */
int edgehip_net_pack(edgehip_ctx *ctx, int slot, int slot_pair /* -1: none */, const double *k_prof /* [nseq] or NULL */);
/* The records of sequence `seq` and their header: records has room for kl_size entries, of which header->kline_num are copied.
 * Either may be NULL.  Synchronises. */
int edgehip_download_net_keylines(edgehip_ctx *ctx, int seq, edgehip_net_keyline *records, edgehip_net_header *header);
/* The same for n sequences seqs[n] (records[j], headers[j] per request; any array or entry may be NULL).  Synchronises once. */
int edgehip_download_net_keylines_batch(edgehip_ctx *ctx, int n, const int32_t *seqs, edgehip_net_keyline *const *records,
                                        edgehip_net_header *const *headers);
/* The stores of sequences [first, first+count) into DEVICE memory of the context's GPU, records_dev[count][kl_size] records (15 B each,
 * back to back) and headers_dev[count] (either may be NULL; e.g. torch uint8 tensors), without a host bounce — like
 * edgehip_depth_image_device.  The copy is complete on return. */
int edgehip_net_keylines_device(edgehip_ctx *ctx, int first, int count, void *records_dev, void *headers_dev);
/* The receiving side (visualizer.cpp:427-428): kn records that came from elsewhere become sequence `seq`'s stored records, header
 * {kn, 0, 1}.  0 <= kn <= kl_size; the bytes behind them are left alone.  The array is free on return. */
int edgehip_upload_net_keylines(edgehip_ctx *ctx, int seq, const edgehip_net_keyline *records, int32_t kn);
/* d_filler[0].ResetData(); FillEdgeData(net_kl, net_kln, p_off, DF_ThreshRelRho, DF_ThreshMatchNum); InitCoarseFine();
 * Integrate(DF_IterNum) (visualizer.cpp:436-439; depth_filler.cpp:41-56, 59-104, 233-355) on every sequence's stored records,
 * in-stream, with the parameters of edgehip_depth_fill_enable (discard included; the visualizer's call leaves it at true).  Per
 * record: rho and s_rho divided by NET_RHO_SCALING; skipped when s_rho / rho > thresh_rel_rho; m_num < thresh_match_num skips it
 * (discard) or sets s_rho = RHO_MAX; cell GetIndex((qx + p_off_x) / block_w, (qy + p_off_y) / block_h) in float, converted as
 * edgehip_depth_fill converts (an index past the grid is dropped).  No p_id / n_id / rho <= 0 gate and no rho0: that is the other
 * overload.  Writes the same grids as edgehip_depth_fill — edgehip_depth_surface, the grid downloads and
 * edgehip_surface_view_capture work on the result unchanged — and shares no other state with it.  EDGEHIP_ERR_STATE when either the
 * fill or the record store is off. */
int edgehip_depth_fill_net(edgehip_ctx *ctx, float p_off_x, float p_off_y);

/* ---- the compressed edge map: KeyLine chains as fitted line segments -------------------------------------------------------
 * edgemap_com_sender::compress_edgemap (src/CommLib/edgemap_com.cpp:162-326) with LineFitting::RobustFit3DLine<float>
 * (src/UtilLib/linefitting.cpp:12-43, 111-204) under it, for every sequence of a slot: each chain of n_id links is walked from its head
 * (p_id < 0), cut where the edge direction turns or the depth ratio jumps, a 3D line is fitted to each piece by weighted least squares,
 * and the two end points of each piece leave as 5-byte compressed_kl records (include/CommLib/edgemap_com.h:45-51); a negative rho
 * closes a polyline.  A few thousand bytes per frame instead of 168 (or 15) bytes per KeyLine.
 *
 * The walk is order dependent (heads in ascending index against a shared mask).  Walks touch only KeyLines reachable from their head, so
 * walks in different weakly connected components of the n_id graph commute: the device labels the components, sorts the heads' keys
 * (component, index) and runs one lane per component, its heads serially — exact on any link graph (merging chains, cycles, self-links).
 * Records are numbered in head order over the whole list: a counting walk per head, a scan over the counts in index order, then the
 * walk again with the fits.  The walk and the fit are the code of rebvo_amd/csrc/edgemap_fit.h, shared with the serial host restatement
 * rebvo_compress_edgemap (rebvo_amd/host/include/rebvo/edgemap_com.h), whose records the device's equal byte for byte.
 *
 * The fit list (the reference's fit_list[max_line_len]) is stored nowhere: it always is the n_id path of f_inx KeyLines from the last
 * cut, and the fit walks that path again (four passes of dependent loads, served by the L2).  One lane runs a whole component: a
 * link graph that is one giant component (every chain merging into one) runs on a single lane of its sequence's workgroup.  No LDS or scratch is sized by
 * max_line_len, so max_line_len has no upper limit.
 * sin / cos of the fitted direction come from square roots and divisions instead of atan2, sin and cos (edgemap_fit.h): the same IEEE
 * operations on host and device, but possibly another last bit of the double than glibc's before tx, ty and zfo are narrowed to float.
 * Out of domain (the reference's integer conversions are undefined there): NaN or infinite rho / s_rho, s_rho <= 0. */
#pragma pack(push, 1)
typedef struct edgehip_compressed_kl {   /* rebvo::compressed_kl, byte for byte */
    uint8_t x, y;           /* clamp_uchar(x * x_scaling), clamp_uchar(y * y_scaling) */
    int16_t rho;            /* clamp_short(max(rho * (32767/20) / scale, (32767/20) * 1e-3)); negative: the polyline ends here */
    uint8_t s_rho;          /* clamp_uchar(fit_sigma * (255/20)) */
} edgehip_compressed_kl;
#pragma pack(pop)
#ifdef __cplusplus
static_assert(sizeof(edgehip_compressed_kl) == 5, "compressed_kl is 5 bytes on the wire");
#else
_Static_assert(sizeof(edgehip_compressed_kl) == 5, "compressed_kl is 5 bytes on the wire");
#endif
typedef struct edgehip_edgemap_params {   /* compress_edgemap's arguments (edgemap_com.cpp:168) */
    int32_t min_line_len;   /* >= 0 */
    int32_t max_line_len;   /* >= 1 (the reference declares fit_list[max_line_len] and writes entry 0) */
    int32_t match_n_t;      /* m_num below it: s_rho counts as 1e10 */
    int32_t pad;
    double max_angle;       /* radians; cos(max_angle) is taken once on the host */
    double rho_rel_max;
    double x_scaling, y_scaling;   /* 0 means the reference's COMPRESSED_X_SCALING 0.5 / COMPRESSED_Y_SCALING 1 (edgemap_com.h:42-43), whose
                                      byte coordinates cover 510 x 255 pixels and clamp beyond; other values are this library's only
                                      extension, for its own decoder */
} edgehip_edgemap_params;
#define EDGEHIP_EDGEMAP_BAD_LINK 1    /* status: a p_id / n_id outside [-1, kn) was read as -1 */
#define EDGEHIP_EDGEMAP_OVERFLOW 2    /* status: more than cap_records records: count 0 (the reference's `return kl_num=0`) */
#define EDGEHIP_EDGEMAP_STEP_GUARD 4  /* status: a walk ran into its bound of kn + 1 steps (no link graph does) */
/* Allocates the store: nseq x cap_records records back to back (5 B each), a count and a status per sequence, and the scratch of the
 * component pass (8 B per KeyLine and per record).  With min_line_len >= 1, cap_records = 2 * max_points cannot overflow.  0 frees
 * everything.  A context that never calls this allocates and launches nothing; edgehip_process_frame never enqueues any of it.
 * EDGEHIP_ERR_ARG for cap_records < 0; EDGEHIP_ERR_MEMORY when the allocation fails (the store is then off). */
int edgehip_edgemap_enable(edgehip_ctx *ctx, int cap_records);
/* compress_edgemap on the KeyLines of `slot` for every sequence, in-stream (no synchronisation); the slot is only read.  scale: host
 * array [nseq] (the reference passes nav.K), or NULL for 1.  Camera: the context's principal point and zfm.  EDGEHIP_ERR_ARG for a
 * slot out of range, min_line_len < 0, max_line_len < 1 or a negative scaling; EDGEHIP_ERR_STATE when the store is off. */
int edgehip_edgemap_compress(edgehip_ctx *ctx, int slot, const edgehip_edgemap_params *params, const double *scale /* [nseq] or NULL */);
/* The records of sequence `seq` (room for cap_records, *count are copied), their number and the status bits.  Any may be NULL.
 * Synchronises. */
int edgehip_download_edgemap(edgehip_ctx *ctx, int seq, edgehip_compressed_kl *records, int32_t *count, int32_t *status);
/* The same for n sequences seqs[n]: records[j] (array or entries may be NULL), counts[n], status[n] (may be NULL).  Synchronises once
 * for the counts and once for the records. */
int edgehip_download_edgemap_batch(edgehip_ctx *ctx, int n, const int32_t *seqs, edgehip_compressed_kl *const *records, int32_t *counts,
                                   int32_t *status);
/* The stores of sequences [first, first+count) into DEVICE memory: records_dev[count][cap_records] records (5 B each, back to back) and
 * counts_dev[count] int32 (either may be NULL), without a host bounce — like edgehip_net_keylines_device.  Complete on return. */
int edgehip_edgemap_device(edgehip_ctx *ctx, int first, int count, void *records_dev, void *counts_dev);
/* The records for output callbacks at full pipeline depth, through one more instance of the KeyLine export's staging ring (like
 * edgehip_ros_export): edgehip_edgemap_compress on the OLD slot of the newest frame pair, in-stream, with scale[j] for sequence seqs[j]
 * (1 for the others), then the lists of the n requested sequences, their counts and status words into a ring entry; nothing
 * synchronises.  *ticket_out names the entry.  EDGEHIP_ERR_STATE before two frames or with the store off. */
int edgehip_edgemap_export(edgehip_ctx *ctx, int n, const int32_t *seqs, const double *scale, const edgehip_edgemap_params *params, int *ticket_out);
/* Enqueues the copies of a ticket on the ring's stream: up to max_records[j] records of list j to records_dst[j] (array or entries may
 * be NULL) and pairs_dst[n][2] = (count, status) per list.  The count is known only on the device, so the caller bounds the copy: with
 * min_line_len >= 1 a list has at most 2 * kn records.  The destinations are valid after edgehip_edgemap_export_wait. */
int edgehip_edgemap_export_fetch(edgehip_ctx *ctx, int ticket, const int32_t *max_records, edgehip_compressed_kl *const *records_dst,
                                 int32_t *pairs_dst);
/* Blocks until the ticket's copies have landed (or, never fetched, its kernels have run) and frees the entry. */
int edgehip_edgemap_export_wait(edgehip_ctx *ctx, int ticket);
/* Measurement (tools/edgemap_compress_timing.py): device time of the last edgehip_edgemap_compress made under
 * edgehip_profile_enable(ctx, 1), by HIP events: ms[0] component labelling, ms[1] the heads' keys and their sort (such a call runs
 * the two as launches of their own, the labels crossing in HBM; otherwise they are one launch), ms[2] the walks (counting pass, scan,
 * fitting pass), ms[3] the placement of the records.  EDGEHIP_ERR_STATE otherwise.  Waits for them. */
int edgehip_edgemap_ms(edgehip_ctx *ctx, float ms[4]);

/* ---- the compressed edge map, received: segments, visibility, depth grid ---------------------------------------------------
 * edgemap_com_decoder (include/CommLib/edgemap_com.h:226-252, src/CommLib/edgemap_com.cpp:42-160, 431-528) over the record store of
 * edgehip_edgemap_enable, for every sequence in one launch per step.  The store takes records from edgehip_edgemap_compress (which
 * also leaves the scale it used as the store's rho_scale, the double narrowed to float as the reference's rho_scale=scale narrows it)
 * or from edgehip_upload_edgemap.  The rules are rebvo_amd/csrc/edgemap_seg.h, shared with the serial host restatements decode,
 * hide_visible and fill_depth_map of rebvo/edgemap_com.h, whose results the device's equal bit for bit.
 *
 * Departures from the reference, all of them:
 *   - getPair's cursor walk is evaluated as a rule local to a record (it starts a segment iff it is not the last record, its rho is
 *     not 0, and it is not a negative record behind a positive one); every list gives the segments the walk gives, in its order.
 *   - A list with more than cap_segments segments is cut in order and flagged (the reference's bound is KEYLINE_MAX), and the fill
 *     folds the decoded segments: fillDepthMap reads the records through getPair again, which differs only for a list that was cut.
 *   - fillDepthMap updates a cell once per step of a segment, in segment and then step order; here those (segment, step) items are
 *     numbered by a scan and brought to their cells by the stable ordered scatter of the fill, so a cell sees the same updates in the
 *     same order.  A sequence with more than cap_items items folds none (the reference has no bound) and is flagged.
 *   - use_visibility != 0 skips hidden segments in the fill.  The reference's fillDepthMap ignores visi_mask; 0 is its behaviour.
 *   - x_scaling / y_scaling other than the reference's 0.5 and 1 (edgehip_edgemap_params).
 *   - (int) of a step's position converts as an x86-64 build converts it; a direction of infinite length (only with scalings that
 *     overflow a float) is a sequence over cap_items rather than an endless loop.
 * Not built: GetLowerKL (it sums a histogram it never zeroes) and dfillerHideVisible (per-cell visibility of two fillers). */
#define EDGEHIP_EDGEMAP_SEGMENT_OVERFLOW 1   /* decoder status: more than cap_segments segments; the first cap_segments are kept */
#define EDGEHIP_EDGEMAP_ITEM_OVERFLOW 2      /* decoder status: the last edgehip_depth_fill_segments met more than cap_items steps: none folded */
/* `count` records (and the rho_scale of their header) become sequence seq's stored edge map: the counterpart of
 * edgehip_upload_net_keylines.  EDGEHIP_ERR_ARG for count outside [0, cap_records] or a rho_scale that is not finite, is <= 0 or is so
 * small (below about 5e-36) that getPair's divisor (32767 / 20) / rho_scale is no finite float; EDGEHIP_ERR_STATE when the store is
 * off.  Synchronises.
 * Domain of everything below: a store whose rho_scale passes this test.  Then the local decode rule equals getPair's walk on every
 * list, every decoded rho is a positive finite float and every s_rho at least 1e-3, and no record list puts a NaN into the grid.
 * edgehip_edgemap_compress / _export store the scale they are given unchecked (they always accepted any double): a NaN, infinite, zero,
 * negative or vanishing scale there is out of domain for the decoder (NaN or +-0 rho; no gate compares true on a NaN, so it folds). */
int edgehip_upload_edgemap(edgehip_ctx *ctx, int seq, const edgehip_compressed_kl *records, int32_t count, float rho_scale);
/* Allocates the decoder: per sequence cap_segments segments (8 floats and a visibility byte; 44 B more for the fill's direction and
 * offset) and cap_items (segment, step) items (8 B each).  cap_segments 0 frees it.  A context that never calls this allocates and
 * launches nothing; edgehip_process_frame never enqueues any of it.  EDGEHIP_ERR_ARG outside [0, 2^24]. */
int edgehip_edgemap_decode_enable(edgehip_ctx *ctx, int cap_segments, int cap_items);
/* edgemap_com_decoder::Decode on every sequence's stored records, in-stream: segments in record order, every visibility flag 1.
 * x_scaling / y_scaling as the sender's (0: the reference's 0.5 and 1).  EDGEHIP_ERR_STATE when the decoder or the store is off. */
int edgehip_edgemap_decode(edgehip_ctx *ctx, double x_scaling, double y_scaling);
/* Segments (k0, k1: x, y, rho, s_rho; room for cap_segments x 8 floats), visibility flags (cap_segments bytes), their number and the
 * decoder's status bits of sequence `seq`.  Any may be NULL.  Synchronises. */
int edgehip_download_edgemap_segments(edgehip_ctx *ctx, int seq, float *segments, uint8_t *flags, int32_t *count, int32_t *status);
int edgehip_download_edgemap_segments_batch(edgehip_ctx *ctx, int n, const int32_t *seqs, float *const *segments, uint8_t *const *flags,
                                            int32_t *counts, int32_t *status);
/* edgemap_com_decoder::HideVisible on every sequence whose rows are not NULL: dpose[seq] (9 doubles, row-major) and dpos[seq] (3) are
 * GetDPose() / GetDPos() after UpdatePos (rebvo::edgemap::update_pos computes them on the host), k_em[seq] the stored map's K and
 * k_new[seq] the new view's.  A segment whose k0 or k1, moved by TransformPos, lands inside the context's frame with rho > 0 loses
 * its flag; a flag that is 0 stays 0.  s_num_out[nseq] (may be NULL): segments that were visible and stay visible, -1 for a sequence
 * left alone.  Synchronises. */
int edgehip_edgemap_hide_visible(edgehip_ctx *ctx, const double *const *dpose, const double *const *dpos, const float *k_em, const float *k_new,
                                 int32_t *s_num_out);
/* The third source of the depth fill: ResetData, edgemap_com_decoder::fillDepthMap(df, cam, v_thresh, a_thresh) on the decoded
 * segments, InitCoarseFine, Integrate(iter_num), in-stream, with the block size, iter_num and bound_mode of edgehip_depth_fill_enable
 * and the context's camera.  Writes the same grids as edgehip_depth_fill and shares no other state with it.  use_visibility: see the
 * departures above.  EDGEHIP_ERR_STATE when the fill or the decoder is off or nothing was decoded. */
int edgehip_depth_fill_segments(edgehip_ctx *ctx, double v_thresh, double a_thresh_deg, int use_visibility);
/* Measurement (tools/edgemap_decode_timing.py): device time of the last decode, hide, item and fill launch made under
 * edgehip_profile_enable(ctx, 1), by HIP events; -1 for a stage not run so.  Waits for them. */
int edgehip_edgemap_decode_ms(edgehip_ctx *ctx, float ms[4]);

/* ---- depth surface (what depth_filler's callers take from the grid) --------------------------------------------------------
 * From the grids of the last edgehip_depth_fill, for every sequence, in the camera frame and bit for bit as depth_filler computes them
 * (tests/depth_surface_port.py restates it), except the sign and payload of a NaN the arithmetic creates:
 *   per cell (surface != 0), cell (x, y) at y * gw + x:
 *     point[3]  get3DPos(x, y) (include/visualizer/depth_filler.h:115-122, gl_viewer.cpp / surface_integrator.cpp:48, 93)
 *     dist      computeDistance(Zeros) (depth_filler.cpp:170-180, visualizer.cpp:436-440, keyframe.cpp:181): |point|
 *     min_dist  one per sequence: current_min_dist / GetMinDist() of the same call (1e20 when every dist is NaN)
 *     normal[3] calcSurfNormals (depth_filler.cpp:358-373): the value its raster loop leaves — a cell's own computation for x <= gw-2,
 *               y <= gh-2, else that of (x-1, y-1)
 *     area      calcSurfArea (depth_filler.cpp:377-389), float as df_point::area
 *   One departure, where the reference has no defined result: the cells calcSurfNormals never writes ((gw-1, 0), (0, gh-1), every
 *   cell of a grid 1 cell wide or high) and calcSurfArea never writes (the last row and column) hold NaN; the reference leaves them
 *   uninitialised.
 *   per pixel (image_mode), at every integer pixel (px, py) of the w x h image, rho[py][px] and s_rho[py][px] as float (both
 *   functions compute in float: exact): getImgRho(px, py, &s_rho) (depth_filler.h:246-280, gl_viewer.cpp:562-602) or
 *   getImgRhoTriInterp(px, py, &s_rho) (depth_filler.h:203-244, its s_rho formula as written). */
typedef enum edgehip_depth_image_mode {
    EDGEHIP_DEPTH_IMAGE_OFF = 0,
    EDGEHIP_DEPTH_IMAGE_BILINEAR = 1,   /* getImgRho */
    EDGEHIP_DEPTH_IMAGE_TRIANGLE = 2    /* getImgRhoTriInterp */
} edgehip_depth_image_mode;
typedef struct edgehip_depth_surface_params {
    int32_t surface;      /* != 0: per-cell point / normal / area / dist / min_dist */
    int32_t image_mode;   /* edgehip_depth_image_mode */
} edgehip_depth_surface_params;
/* Allocates the products for every sequence: 60 B per cell (+ 8 B per sequence) for the surface, w * h * 8 B for the image.
 * params == NULL, or both products off, frees them.  EDGEHIP_ERR_STATE while the fill is off, EDGEHIP_ERR_ARG for an unknown
 * image_mode, EDGEHIP_ERR_MEMORY when the allocation fails (the products are then off; the context stays usable).  Disabling the
 * fill, or enabling it with other block sizes, frees them too. */
int edgehip_depth_surface_enable(edgehip_ctx *ctx, const edgehip_depth_surface_params *params);
/* computeDistance(Zeros) + calcSurfNormals + calcSurfArea and / or the image, from the grids of the last edgehip_depth_fill, for
 * every sequence, in-stream (no synchronisation).  EDGEHIP_ERR_STATE when not enabled or before the first fill since the fill's
 * enable. */
int edgehip_depth_surface(edgehip_ctx *ctx);
/* The per-cell products of sequence `seq`: point[3 gh gw], normal[3 gh gw], area[gh gw], dist[gh gw], min_dist[1].  Any may be NULL.
 * Synchronises.  EDGEHIP_ERR_STATE when the surface is not enabled. */
int edgehip_download_depth_surface(edgehip_ctx *ctx, int seq, double *point, double *normal, float *area, double *dist, double *min_dist);
/* The same for n sequences seqs[n] (point[j], ... per request; any array or entry may be NULL).  Synchronises once. */
int edgehip_download_depth_surfaces_batch(edgehip_ctx *ctx, int n, const int32_t *seqs, double *const *point, double *const *normal,
                                          float *const *area, double *const *dist, double *const *min_dist);
/* The depth image of sequence `seq`: rho[h w], s_rho[h w] (row-major; either may be NULL).  Synchronises.  EDGEHIP_ERR_STATE when
 * the image is not enabled. */
int edgehip_download_depth_image(edgehip_ctx *ctx, int seq, float *rho, float *s_rho);
/* The same for n sequences seqs[n] in one call.  Synchronises once. */
int edgehip_download_depth_images_batch(edgehip_ctx *ctx, int n, const int32_t *seqs, float *const *rho, float *const *s_rho);
/* The images of sequences [first, first+count) into DEVICE memory of the context's GPU, rho_dev[count][h][w] and s_rho_dev[count][h][w]
 * (either may be NULL; e.g. torch tensors), without a host bounce — like edgehip_read_nav_log_device.  The copy is complete on return. */
int edgehip_depth_image_device(edgehip_ctx *ctx, int first, int count, float *rho_dev, float *s_rho_dev);

/* ---- cross-view surface integration (the key-frame viewer's OcGrid ray cut) ---------------------------------------------
 * Which cells of several filled grids are occluded: a cell is hidden when it lies in free space that another view's rays have crossed
 * (src/visualizer/surface_integrator.cpp, driven by app/kf_visualizer/main.cpp:110-116, 192, 201).  A "view" is what the reference
 * takes from a keyframe there: its depth_filler grid (rho, s_rho), Pose (3x3, row-major), Pos and scale K, with
 * Local2WorldScaled(p) = Pose * p * K + Pos (include/mtracklib/keyframe.h:101-103); camera and block size are the context's.
 * The reference registers every cell in the voxels its surface samples fall in (OcGrid::fillKFList, :167-229), then marches a ray per
 * cell of each casting view from the camera centre to the cell's point at rho + s_rho in steps of the smallest voxel edge, and clears
 * the `visibility` of every registered cell of ANOTHER view in each voxel it steps through (rayCutSurface / hideAll, :235-266,
 * :153-163).  Visibility only falls, so the result does not depend on the order: cell c of view A ends hidden iff some voxel holds
 * both a fill sample of c and a ray step of a casting view B != A.  The device keeps one 4-byte word per voxel (which views' rays
 * crossed it: none, exactly one and which, or several) instead of the reference's per-voxel pointer lists, marks the rays, then walks
 * every cell's samples in the reference's order and arithmetic (float accumulators with double increments; getImg3DPos's float
 * bilinear rho, depth_filler.h:133-163; fp64 elsewhere) and looks them up.  Every flag equals the reference's
 * (tests/surface_integrate_port.py restates it).  Up to 1024 views.  Departures, all where the reference has no defined result:
 *   - a fill sample or ray step outside the box is dropped: outside = a quotient (p - origin)[i] / block[i] that is negative, not
 *     finite or >= n on any axis.  (The reference converts negative doubles to u_int and indexes with the wrapped value, and lets
 *     p - origin == size through.)  A ray stops at the first step from which every later step is outside as well.
 *   - a cell whose rho / K is not finite or not positive contributes no fill samples (it stays visible; its ray is still cast).  The
 *     reference's sample loop does not end when its step is 0; neither does it when an accumulator stops advancing (a step below half
 *     an ulp of the pixel coordinate): the walk ends there.
 *   - a ray whose length / step is not finite, or is past the int range, takes no steps (the x86 conversion gives INT_MIN there: the
 *     same).  rho + s_rho == 0 is such a ray.
 *   - the box needs a finite origin and a finite, positive size (EDGEHIP_ERR_ARG otherwise).
 *   - fillKFList's "blocks filled" counter is not produced. */
typedef struct edgehip_surface_views_params {
    int32_t capacity;       /* view slots, 1..1024 */
    int32_t nx, ny, nz;     /* OcGrid's grid_size (main.cpp:113 uses 500, 500, 500) */
} edgehip_surface_views_params;
/* Allocates the view store (per slot: the two grids, the pose, one visibility byte per cell: 17 B per cell) and the voxel plane
 * (4 B per voxel: 500 MB at 500^3).  params == NULL frees them.  EDGEHIP_ERR_STATE while the depth fill is off, EDGEHIP_ERR_ARG for a
 * capacity outside [1, 1024] or a dimension < 1, EDGEHIP_ERR_MEMORY when the allocation fails (the store is then off; the context
 * stays usable).  Disabling the fill, or enabling it with other block sizes, frees the store too. */
int edgehip_surface_views_enable(edgehip_ctx *ctx, const edgehip_surface_views_params *params);
/* Sequence `seq`'s grid of the last edgehip_depth_fill into slot `view`, with the pose the caller tracks for it (what edgehip_nav
 * reports: Pose[9] row-major, Pos[3], K), in-stream: keyframe + initDepthFiller (keyframe.cpp:171-184) as the integrator sees them.
 * Sets the view's visibility to 1 (depth_filler::ResetVisibility, depth_filler.cpp:190-194).  EDGEHIP_ERR_STATE before the first fill. */
int edgehip_surface_view_capture(edgehip_ctx *ctx, int seq, int view, const double *Pose, const double *Pos, double K);
/* The same from host arrays rho[gh*gw], s_rho[gh*gw] (key frames loaded from a file, keyframe::loadKeyframesFromFile, main.cpp:82;
 * stage-isolated tests).  The arrays are free on return. */
int edgehip_surface_view_upload(edgehip_ctx *ctx, int view, const double *rho, const double *s_rho, const double *Pose, const double *Pos,
                                double K);
/* Empties slot `view`: like a key frame without a depth filler (depthFillerAval() false, :42, :173, :237) it casts no rays, is not
 * tested and does not count in edgehip_surface_space. */
int edgehip_surface_view_clear(edgehip_ctx *ctx, int view);
/* SurfaceInt::analizeSpaceSize over the stored views (surface_integrator.cpp:32-68): origin[3] = the minimum and size[3] = maximum -
 * minimum of Local2WorldScaled(get3DPos(x, y)) over every cell, bit for bit (the maxima start at 1e-20 as there), except the sign of a
 * zero.  Synchronises. */
int edgehip_surface_space(edgehip_ctx *ctx, double *origin, double *size);
/* OcGrid(origin, size, {nx, ny, nz}) + fillKFList + rayCutSurface (surface_integrator.cpp:120-132, 167-229, 235-266), in-stream: clears
 * the voxel plane, marks the rays of cast_views[n_cast] (NULL: every stored view, main.cpp:192; empty slots in the list are skipped),
 * then tests every cell of every stored view.  accumulate == 0 sets every visibility to 1 first (ResetVisibility); accumulate != 0
 * keeps earlier hides (main.cpp:201's single-view cut after :192).  origin and size are the caller's: edgehip_surface_space's result
 * for the reference's box (main.cpp:110-113), or a padded one that keeps the camera centres inside. */
int edgehip_surface_integrate(edgehip_ctx *ctx, const double *origin, const double *size, int n_cast, const int32_t *cast_views,
                              int accumulate);
/* SurfaceInt::checkDFRayCrossExaustive(target, hidder) (surface_integrator.cpp:70-116) for n_pairs ordered pairs (targets[j], hidders[j]),
 * in-stream, in one launch: the same question as the OcGrid cut without the box, the resolution or the voxel plane.  A cell of the
 * target is hidden when some ray of the hidder (from its camera centre through one of its cells, both taken into the target's frame
 * by keyframe::transformTo, keyframe.h:105-109) passes the cell's point closer than its bubble, norm(bw, bh) / zfm * K / rho (:79, :95,
 * :98-100), and the cell lies on the ray in front of the hidder's surface: 0 < distance along the ray < dist (:101-102).  Every target
 * cell is tested against every hidder ray, in the reference's fp64 operations and their order, so every flag equals the reference's
 * (tests/surface_ray_cross_port.py restates it).  As there, `dist` is what keyframe::initDepthFiller leaves in the grid through
 * computeDistance(Zeros) (keyframe.cpp:181, depth_filler.cpp:170-182): norm(get3DPos(x, y)), NOT multiplied by the hidder's K, while the
 * distance along the ray is in scaled units.  Cells with a rho that is zero, negative or not finite, and rays without length, take the
 * branch IEEE comparison gives them (false for a NaN), as in the reference.  Visibility only falls, so the reference's early exits
 * change nothing and the pairs may run in any order.
 *   targets == hidders == NULL with n_pairs < 0: every ordered pair t != h of stored views.  With lists, a pair that names an empty
 *   slot is skipped (depthFillerAval() false, :73).  EDGEHIP_ERR_ARG for an id outside [0, capacity) and — the one departure — for a
 *   pair with t == h: the reference's answer there is decided by the rounding of each cell's distance to its own ray.  EDGEHIP_ERR_STATE
 *   before edgehip_surface_views_enable.  On an error nothing is changed.
 *   accumulate == 0 sets every visibility to 1 first (ResetVisibility); accumulate != 0 keeps earlier hides, those of
 *   edgehip_surface_integrate included.  The flags come back through the visibility downloads below.
 * The voxel plane is not touched: nx = ny = nz = 1 in edgehip_surface_views_enable is a valid way to have the store for this check alone. */
int edgehip_surface_ray_cross(edgehip_ctx *ctx, int n_pairs, const int32_t *targets, const int32_t *hidders, int accumulate);
/* df_point::visibility of the cells of `view`: vis[gh*gw], 1 = visible, row-major.  Synchronises.  EDGEHIP_ERR_STATE for an empty slot. */
int edgehip_download_surface_visibility(edgehip_ctx *ctx, int view, uint8_t *vis);
/* The same for n slots views[n] (vis[j] per request; an entry may be NULL).  Synchronises once. */
int edgehip_download_surface_visibilities_batch(edgehip_ctx *ctx, int n, const int32_t *views, uint8_t *const *vis);

/* ---- the ROS nodelet's per-frame output: point cloud and EdgeMap records ---------------------------------------------------
 * The one output callback that ships with the reference is the ROS nodelet's, RebvoNodelet::edgeMapPubCb
 * (ros/src/rebvo_ros/src/rebvo_nodelet.cpp:146-217).  Per KeyLine its loop (:176-212) builds one xyz float point of the rebvo_pcl cloud,
 * cam.unprojectHomCordVec(makeVector(kl.p_m.x, kl.p_m.y, kl.rho / K)) (:203-208; include/UtilLib/cam_model.h:163-169), and one Keyline
 * record of the EdgeMap message (:179-198; ros/src/rebvo_ros/msg/Keyline.msg).  Here both are packed on the device from the SoA
 * KeyLines, for every sequence in one launch: 12 B and / or 52 B per KeyLine leave the device instead of the 168-byte record.
 *   point:   q = rho / K; x = (float)(p_m.x / q / zfm), y = (float)(p_m.y / q / zfm), z = (float)(1.0 / q) — fp64 quotients in the
 *            reference's order, each correctly rounded, zfm the slot camera's (edgehip_set_slot_camera's rule), the narrowing to float
 *            round-to-nearest-even with float denormals kept.  Bit for bit the reference's, except the sign and payload of a NaN the
 *            divisions create (0 / 0, inf / inf: the GPU's default NaN is positive, x86 SSE's negative); a NaN rho passes through as a NaN.
 *   record:  the fields below; rho is NOT divided by K, as in the nodelet.  The two int16 fields keep the low 16 bits of p_id / n_id,
 *            what the nodelet's assignment does on x86-64.
 * edgehip_ros_keyline is the little-endian ROS wire body of one element of `Keyline[] Keylines` (fixed-size fields in message order,
 * no padding), so n records are the serialised array's body element for element; edgehip_ros_point is one point of a PointCloud2 with
 * the fields "xyz" (point_step 12). */
typedef struct edgehip_ros_point { float x, y, z; } edgehip_ros_point;
#pragma pack(push, 1)
typedef struct edgehip_ros_keyline {   /* rebvo/Keyline.msg, field for field */
    float KlGrad[2];        /* m_m */
    float KlImgPos[2];      /* c_p */
    double invDepth;        /* rho */
    double invDepthS;       /* s_rho */
    float KlFocPos[2];      /* p_m */
    int32_t KlMatchID;      /* m_id */
    int32_t ConsMatch;      /* m_num */
    int16_t KlPrevMatchID;  /* (int16_t)p_id */
    int16_t KlNextMatchID;  /* (int16_t)n_id */
} edgehip_ros_keyline;
#pragma pack(pop)
#ifdef __cplusplus
static_assert(sizeof(edgehip_ros_point) == 12, "a PointCloud2 xyz point is 12 bytes");
static_assert(sizeof(edgehip_ros_keyline) == 52, "a Keyline.msg record is 52 bytes on the wire");
#else
_Static_assert(sizeof(edgehip_ros_point) == 12, "a PointCloud2 xyz point is 12 bytes");
_Static_assert(sizeof(edgehip_ros_keyline) == 52, "a Keyline.msg record is 52 bytes on the wire");
#endif
#define EDGEHIP_ROS_POINTS 1
#define EDGEHIP_ROS_KEYLINES 2
/* Allocates the chosen stores, zeroed: nseq x max_points records of each kind, back to back (a sequence's records start at
 * seq * max_points * 12 resp. * 52 bytes), and nseq counts.  what == 0 frees them.  EDGEHIP_ERR_ARG for other bits than the two above;
 * EDGEHIP_ERR_MEMORY when the allocation fails (the stores are then off; the context stays usable). */
int edgehip_ros_enable(edgehip_ctx *ctx, int what);
/* The loop of rebvo_nodelet.cpp:176-212 on the KeyLines of `slot`, for every sequence, in-stream (no synchronisation): KeyLine j goes
 * to record j of each enabled store, j < kn, and kn to the sequence's count.  Reads exactly what edgehip_download_keylines returns for
 * the slot — for the OLD slot of a processed frame, its turned p_m / m_m / rho / s_rho (see there).  k_prof: host array [nseq] of the K
 * each sequence's rho is divided by (edgeMapRebvo.K, :204), or NULL for each sequence's edgehip_seq_state::K.  Only the kn records of a
 * sequence are written.  EDGEHIP_ERR_STATE when the stores are off, EDGEHIP_ERR_ARG for a slot out of range. */
int edgehip_ros_pack(edgehip_ctx *ctx, int slot, const double *k_prof /* [nseq] or NULL */);
/* The records of sequence `seq` from the last edgehip_ros_pack: points / keylines have room for max_points entries, of which *kn_out are
 * copied.  Any destination may be NULL (as is one whose store is not enabled).  Synchronises. */
int edgehip_download_ros_edgemap(edgehip_ctx *ctx, int seq, edgehip_ros_point *points, edgehip_ros_keyline *keylines, int32_t *kn_out);
/* The same for n sequences seqs[n] (points[j], keylines[j], kn_out[j] per request; any array or entry may be NULL).  Synchronises once. */
int edgehip_download_ros_edgemaps_batch(edgehip_ctx *ctx, int n, const int32_t *seqs, edgehip_ros_point *const *points,
                                        edgehip_ros_keyline *const *keylines, int32_t *kn_out);
/* The whole stores of sequences [first, first+count) into DEVICE memory of the context's GPU: points_dev[count][max_points] (12 B each),
 * keylines_dev[count][max_points] (52 B each, back to back), kn_dev[count] int32 (any may be NULL; a store that is not enabled is
 * EDGEHIP_ERR_STATE), without a host bounce — like edgehip_net_keylines_device.  The copy is complete on return. */
int edgehip_ros_edgemap_device(edgehip_ctx *ctx, int first, int count, void *points_dev, void *keylines_dev, void *kn_dev);
/* TEST SUPPORT ONLY, not part of the product surface: the other direction, same shapes and rules (no counts) — device memory becomes the
 * stores' bytes of sequences [first, first+count), so that a test can put a sentinel behind the records and see that a pack leaves it
 * alone.  The next edgehip_ros_pack overwrites what it covers; nothing in the library reads the stores back. */
int edgehip_ros_edgemap_from_device(edgehip_ctx *ctx, int first, int count, const void *points_dev, const void *keylines_dev);
/* The same products for output callbacks at full pipeline depth, with the semantics of edgehip_export_keylines / _fetch / _wait (above)
 * and a staging ring of their own: the OLD slot of the frame processed last, packed in-stream for sequences seqs[n] with k_prof[n] (required:
 * the callback of frame k-1 divides by pbuf.K of frame k-1, which the device no longer holds), what = EDGEHIP_ROS_POINTS |
 * EDGEHIP_ROS_KEYLINES (needs no edgehip_ros_enable); at most four tickets outstanding.  The staging grows with n and with the record kinds asked
 * for, which it can only do while no ticket is outstanding (EDGEHIP_ERR_STATE otherwise: ask for the largest request first).  Fetch enqueues the copies of exactly kn[j] records
 * into points_dst[j] / keylines_dst[j] (either array or any entry may be NULL; page-locked destinations are written by DMA) on a copy
 * stream.  Wait blocks until they have landed and releases the ticket; for a ticket that was never fetched it waits for the pack itself, so
 * that the staging entry is not reused under a kernel that has yet to write it. */
int edgehip_ros_export(edgehip_ctx *ctx, int n, const int32_t *seqs, const double *k_prof, int what, int *ticket_out);
int edgehip_ros_export_fetch(edgehip_ctx *ctx, int ticket, const int32_t *kn, edgehip_ros_point *const *points_dst,
                             edgehip_ros_keyline *const *keylines_dst);
int edgehip_ros_export_wait(edgehip_ctx *ctx, int ticket);

/* ---- key-frame tracking (TrackKeyFrames) ------------------------------------------------------------------------------------
 * What SecondThread does with REBVO/TrackKeyFrames = 1 (rebvo_second_t.cpp:156-162, 429-444, 587-598): it keeps a current key frame —
 * a copy of an edge map with its pose (keyframe.cpp:28-43) — and, after every frame pair whose matching succeeded, repairs the matches
 * between that key frame and the newest edge map in both directions with kfvo::buildForwardMatch, forwardCorrectAugmentate and
 * correctAugmentate (src/mtracklib/kfvo.cpp:739-771, 969-1142, 804-966); a new key frame is taken when the repaired back-match count drops
 * below min(TrackPoints, KNum) * KFSavePercent.  Here every sequence has ONE key frame in HBM, the reference's kf_list.back(); older key
 * frames go into the key-frame list below when it is enabled, and are otherwise the caller's to take when `inserted` is set.  Only
 * m_id_f of the key frame, m_id_kf of the frame lists and the counts change: nothing feeds back into the odometry, with one exception that
 * only a caller can trigger: edgehip_keyframe_translate_depth with direction = 1 (below) writes a frame slot's rho / s_rho.  Every id and count equals the reference's (integers; the distances behind them are fp64
 * in the reference's order of operations; tests/keyframe_track_port.py restates the rule).
 * Preconditions: every p_m finite; m_id, m_id_f, m_id_kf negative or in range of the list they index.  Out-of-range links end a chain;
 * every chain walk is capped at the length of the list it walks (on finite p_m it ends before), a capped walk sets `guard`.
 * Not for a context with the device IMU branch (EDGEHIP_ERR_STATE). */
/* keyframe's pose block (keyframe.h: t, K, Rot, RotLie, Vel, Pose, PoseLie, Pos). */
typedef struct edgehip_kf_pose {
    double t, K;
    double Rot[9], RotLie[3], Vel[3], Pose[9], PoseLie[3], Pos[3];
} edgehip_kf_pose;
/* Per-frame record of the key-frame tracking, beside edgehip_nav (read by edgehip_read_keyframe_track). */
typedef struct edgehip_kf_track {
    int32_t fow_m0, fow_m;     /* num_kf_fow_m after buildForwardMatch / after forwardCorrectAugmentate (0 when the steps did not run) */
    int32_t back_m0, back_m;   /* num_kf_back_m as directed_matching left it / after correctAugmentate (equal when the steps did not run) */
    int32_t inserted;          /* this frame took a new key frame (either rule) */
    int32_t kf_count;          /* kf_list.size() */
    int32_t guard;             /* != 0: a chain walk hit its cap (bit 0) or met a match outside its list (bit 1): a precondition was broken */
    int32_t kf_kn;             /* KeyLines of the current key frame */
} edgehip_kf_track;
/* enable = 1: allocates every sequence's key frame (all KeyLine fields, about 140 B per KeyLine of capacity) and the scratch of the
 * repair (20 B per KeyLine), empty (kf_count = 0), and switches the feature on inside edgehip_process_frame — the first-key-frame rule on
 * the old slot before a frame pair is processed (:156-162), the three steps behind directed_matching for sequences with klm_num >=
 * MatchThreshold with (dist_thesh, dist_tolerance, augmentate) = (10, 0, true) (:429-444), the insertion from the new slot at the frame's
 * end when save_keyframes != 0 and the criterion holds (:591-596); edgehip_nav::kf_matchs / edgehip_seq_state::kf_matchs then carry the
 * repaired back count, as num_kf_back_m does upstream.  kf_save_percent = REBVO/KFSavePercent, save_keyframes = REBVO::saveKeyframes.
 * enable = 2: the same store for the entry points below alone; edgehip_process_frame leaves the key frames to the caller.
 * enable = 0 frees everything (the default state: edgehip_process_frame enqueues exactly what it does without the feature). */
int edgehip_keyframe_track_enable(edgehip_ctx *ctx, int enable, double kf_save_percent, int save_keyframes);
/* keyframe(...) + kfvo::resetForwardMatch + kfvo::resetKFMatch (kfvo.cpp:774-787) from ring slot `slot` for the sequences with mask[seq]
 * != 0 (mask == NULL: all): the key frame becomes a copy of the slot's KeyLines with m_id_f = i, rho0 = rho, s_rho0 = s_rho, and the
 * slot's m_id_kf = i; kf_count goes up by one.  pose[nseq] (entries of unmasked sequences are ignored), or NULL for the newest nav
 * record's t, Rot, RotLie, Vel, Pose, PoseLie, Pos and edgehip_seq_state::K.  In-stream, no synchronisation. */
int edgehip_keyframe_insert(edgehip_ctx *ctx, int slot, const uint8_t *mask, const edgehip_kf_pose *pose);
/* kfvo::buildForwardMatch(kf, new, old): the key frame's m_id_f, which index the list slot_new's KeyLines were matched against (their
 * m_id), re-pointed into slot_new.  counts[nseq] (may be NULL: no synchronisation) = the function's return value. */
int edgehip_keyframe_build_forward_match(edgehip_ctx *ctx, int slot_new, int32_t *counts);
/* kfvo::forwardCorrectAugmentate / kfvo::correctAugmentate(kf, new, Pose, Pos, dist_thresh, dist_tolerance, augmentate) for every
 * sequence: Pose[nseq][9], Pos[nseq][3], or both NULL for Pose * R and Pos - Pose * R * V * K from edgehip_seq_state (what the frame
 * driver has at that point, rebvo_second_t.cpp:435-436).  counts as above. */
int edgehip_keyframe_forward_correct(edgehip_ctx *ctx, int slot_new, const double *Pose, const double *Pos, double dist_thresh,
                                     double dist_tolerance, int augmentate, int32_t *counts);
int edgehip_keyframe_back_correct(edgehip_ctx *ctx, int slot_new, const double *Pose, const double *Pos, double dist_thresh,
                                  double dist_tolerance, int augmentate, int32_t *counts);
/* The records of the last processed frame (the stage-level entry points above write their counts into the same fields).  out[nseq].
 * Synchronises. */
int edgehip_read_keyframe_track(edgehip_ctx *ctx, edgehip_kf_track *out);
/* The current key frame of sequence `seq`: kl has room for max_points records (may be NULL), pose and kf_count may be NULL.
 * Synchronises. */
int edgehip_download_keyframe(edgehip_ctx *ctx, int seq, edgehip_keyline *kl, int32_t *kn_out, edgehip_kf_pose *pose, int32_t *kf_count);
/* Replace it (kf_count goes up by one; the records are taken as they are, no reset).  Synchronises. */
int edgehip_upload_keyframe(edgehip_ctx *ctx, int seq, const edgehip_keyline *kl, int32_t kn, const edgehip_kf_pose *pose);
/* REBVO::saveKeyframes at run time: the criterion of :591-596 inserts only while the flag is set (the first-key-frame rule does not ask
 * it).  Takes effect from the next enqueued frame; the key frames and the list below stay as they are (edgehip_keyframe_track_enable
 * sets the flag too, but frees both).  EDGEHIP_ERR_STATE without key-frame tracking. */
int edgehip_keyframe_set_save(edgehip_ctx *ctx, int save_keyframes);

/* ---- the key-frame list (REBVO::kf_list) -------------------------------------------------------------------------------------
 * Every key frame a sequence replaces — through the frame driver's two rules, edgehip_keyframe_insert or edgehip_upload_keyframe —
 * is kept on the device as it was at that moment: its pose block and its KeyLines as the 168-byte records edgehip_download_keyframe
 * would have returned (score 0, net_id -1, bytes 36..39 zero, the stereo triple (-1, 1.0, 20.0) unless the context keeps it), which
 * are the records keyframe::dumpToBinaryFile writes.  The key frames of a sequence are numbered from 0 in the order it took them
 * (the ordinal); the current one is kf_count - 1 and is NOT in the list, it retires when the next one replaces it.  Retiring is
 * in-stream, inside the captured frame, with no synchronisation; a frame that replaces nothing pays one launch of empty workgroups.
 * Each sequence has a ring of `capacity` entries: ordinal j lives in position j % capacity, and a retirement into a full ring
 * overwrites the oldest entry (first moves up, overwritten counts it).
 * Memory: (168 B x max_points, rounded up to 16) x capacity x nseq for the records — 2.75 GB per unit of capacity at 1024 sequences of
 * 16000 KeyLines — and 264 B x capacity x nseq for the headers. */
typedef struct edgehip_kf_list_info {
    int32_t kf_count;      /* key frames taken so far (edgehip_kf_track::kf_count) */
    int32_t first, held;   /* the list holds the ordinals [first, first + held); first + held == kf_count - 1 once a key frame exists */
    int32_t overwritten;   /* entries the ring has dropped since the list was enabled or reset */
} edgehip_kf_list_info;
/* Allocates the rings, empty (a sequence that has key frames already starts its list at the current one's ordinal).  capacity == 0
 * frees the list alone; edgehip_keyframe_track_enable (any mode) frees it with the key frames; edgehip_reset empties it.
 * EDGEHIP_ERR_STATE without key-frame tracking (capacity > 0), EDGEHIP_ERR_MEMORY when the allocation fails: the list is then off and
 * the context stays usable. */
int edgehip_keyframe_list_enable(edgehip_ctx *ctx, int capacity);
/* info[nseq].  Synchronises. */
int edgehip_keyframe_list_info(edgehip_ctx *ctx, edgehip_kf_list_info *info);
/* Entry `ordinal` of sequence `seq`: kl has room for max_points records (may be NULL), of which *kn_out are copied — a straight copy,
 * the list holds them as records; pose may be NULL.  EDGEHIP_ERR_ARG for an ordinal the list does not hold (overwritten, current, or
 * future); nothing is written then.  Synchronises. */
int edgehip_download_keyframe_list(edgehip_ctx *ctx, int seq, int ordinal, edgehip_keyline *kl, int32_t *kn_out, edgehip_kf_pose *pose);
/* The same for n requests (seqs[j], ordinals[j]) -> kl[j] (array or entries may be NULL), kn_out[j], pose[j] (arrays may be NULL).
 * Two synchronisations however many requests: one for the headers, which say how many records to copy, one for the records. */
int edgehip_download_keyframe_list_batch(edgehip_ctx *ctx, int n, const int32_t *seqs, const int32_t *ordinals, edgehip_keyline *const *kl,
                                         int32_t *kn_out, edgehip_kf_pose *pose);
/* List entry ordinals[seq] of every sequence back into ring slot `slot` as KeyLines (-1: that sequence's slot is left alone): the slot
 * is then what edgehip_upload_keylines(ctx, seq, slot, records, kn, NULL, 0) of the entry's records leaves — edgehip_depth_fill,
 * edgehip_surface_view_capture and edgehip_minimizer_rv_kf run on an older key frame without a host copy.  The ordinals are checked on
 * the host against a synchronising read of the lists' counts, so the call synchronises first; the copy itself is enqueued and not
 * waited for.  EDGEHIP_ERR_ARG for an ordinal a list does not hold: nothing changes. */
int edgehip_keyframe_list_restore(edgehip_ctx *ctx, int slot, const int32_t *ordinals /* [nseq] */);

/* ---- key-frame covisibility (kfvo::countMatches, kfvo::kls_on_fov) ------------------------------------------------------------
 * Which key frames of a sequence see the same edges: the candidate selection for loop closing, for re-localising against the list and
 * for choosing the views of edgehip_surface_integrate.  For an ordered pair (to, from) every KeyLine of `from` is re-projected into
 * `to` (keyframe::reProjectTo, include/mtracklib/keyframe.h:110-114; cam_model.h:146-169), looked up in the distance field
 * global_tracker::build_field(to's edges, field_radius, field_min_mod) leaves (global_tracker.cpp:61-105; image.h:121-126), which is
 * what keyframe::loadFromBinaryFile rebuilds (keyframe.cpp:119-123), and put to the tracker's match test
 * (global_tracker::Calc_f_J_Complete<float>, global_tracker.cpp:115-165):
 *     kl_on_fov, kl_match   kfvo::countMatches(kf_to, kf_from, kl_on_fov, kl_match, match_mod, match_ang, rho_tol, max_r)
 *                           (src/mtracklib/kfvo.cpp:18-55), every integer the reference's
 *     kls_on_fov            kfvo::kls_on_fov(kf_from, kf_to.Pose, kf_to.Pos) (kfvo.cpp:688-712)
 *     guard                 `from` KeyLines whose re-projected image coordinate is not finite; the reference indexes its field out of
 *                           bounds with them, here they are outside the image.  Non-zero: a precondition was broken (rho finite and
 *                           non-zero, finite poses), as with edgehip_kf_track::guard.
 * Read-only: no key frame, list entry or ring slot changes (countMatches also leaves the last pair's match in kf_from's m_id_f; that is
 * not reproduced).  Scratch is allocated by the first call and freed with the key frames: nseq x min(M, 8) x w x h x 4 B of field planes
 * and 52 B x max_points x nseq x (M + 1) of compact KeyLines. */
typedef struct edgehip_kf_pair_count { int32_t kl_on_fov, kl_match, kls_on_fov, guard; } edgehip_kf_pair_count;
typedef struct edgehip_kf_covis_args {
    int32_t field_radius;          /* build_field's radius: SearchRange, the max_r the key-frame file stores */
    float   field_min_mod;         /* <= 0: every KeyLine (the file loader's field) */
    float   match_mod, match_ang, rho_tol, max_r;   /* countMatches' arguments */
} edgehip_kf_covis_args;
/* all ordered pairs of a sequence's key frames: positions 0..held-1 are the list's ordinals first..first+held-1, position held is the
 * current key frame; M = capacity + 1 (1 without a list).  out[nseq][M][M], index [seq][to][from], diagonal included; pairs with a
 * position the sequence does not have are all -1.  info[nseq] (may be NULL) is the edgehip_keyframe_list_info of the same moment.
 * Synchronises.  EDGEHIP_ERR_STATE without key-frame tracking; EDGEHIP_ERR_ARG for NULL args or out, field_radius < 1 or > 4094 (the
 * field's packed key has 12 bits for |t|) and max_points > 2^20 (20 bits for the KeyLine index); EDGEHIP_ERR_MEMORY when the scratch
 * cannot be allocated: the context stays usable. */
int edgehip_keyframe_covisibility(edgehip_ctx *ctx, const edgehip_kf_covis_args *args, edgehip_kf_pair_count *out, edgehip_kf_list_info *info);
/* the query form: ring slot `slot`'s KeyLines as `from` (pose[nseq], or NULL for what edgehip_keyframe_insert takes by default)
 * against every key frame of the same sequence as `to`: out[nseq][M]. */
int edgehip_keyframe_covisibility_slot(edgehip_ctx *ctx, int slot, const edgehip_kf_pose *pose, const edgehip_kf_covis_args *args,
                                       edgehip_kf_pair_count *out, edgehip_kf_list_info *info);
/* Device time of the last of the two calls above, by HIP events: the field build (with the one read of the key frames) and the pair pass. */
int edgehip_keyframe_covisibility_ms(edgehip_ctx *ctx, double *field_ms, double *pair_ms);

/* ---- re-localisation against the key frames (kfvo::OptimizePosGT with kfvo::optimizeScale) ---------------------------------------
 * The pose and scale of ring slot `slot`'s frame relative to every selected key frame of the same sequence — the positions of
 * edgehip_keyframe_covisibility — for the whole batch in one call (src/mtracklib/kfvo.cpp:58-112, 222-260).  Per
 * sequence and position t, with the query's (Pose, Pos, K) and key frame t's (Pose_t, Pos_t, K_t), KeyLines and field
 * build_field(edges_t, field_radius, field_min_mod):
 *     BRelRot = Pose_t.T() * Pose, BRelPos = Pose_t.T() * (Pos - Pos_t) / K, W0 = SO3<>(BRelRot).ln()           (:62-68)
 *     Minimizer_RV_KF<double>(BRelPos, W0, ..., Kr = K / K_t, 5, 30 pi / 180, rho_tol, iter_max, rew_dis, s_rho_q, 0, X, RRV)   (:74)
 *         — the arithmetic of edgehip_minimizer_rv_kf, run over the (sequence, position) pairs as its batch
 *     mnum = #{m_id_f >= 0}                                                                                      (:76-82)
 *     Kp = optimizeScale(kf_t, et, exp(W), BRelPos'): over the query KeyLines with m_id_f >= 0 and q1[2] > 0,
 *          rTr0 += q1[2]^2 / v, rTr += q1[2] rho_b / v, v = s_rho^2 + s_rho_b^2; Kp = (rTr0 > 0 && rTr > 0) ? rTr0 / rTr : 1   (:222-260)
 *     K = K_t * Kp, Pose = SO3<>(Pose_t) * exp(W), Pos = (SO3<>(Pose_t) * BRelPos') * K + Pos_t                  (:93-96)
 * The two sums of optimizeScale are added in a fixed order of the device's own (per lane in KeyLine order with stride 256, then
 * across lanes), not the reference's running sum: the same bits alone, in any batch and under any to_mask.  An empty query list
 * returns score_ratio = 0, mnum = 0, Kp = 1, X = [BRelPos, W0], RRV = 0 (the reference leaves X and RRV unset there) and Pose / Pos
 * from the unchanged W0 / BRelPos.  guard: query KeyLines whose transformed point q1 is not finite, plus one when Pose or Pose_t
 * holds a NaN (broken preconditions, as with edgehip_kf_pair_count::guard).
 * Read-only: no key frame, list entry or ring slot changes.  The reference writes the links into the query's m_id_f, where M pairs
 * would overwrite each other; here every pair has its own link array, read by edgehip_keyframe_relocalize_links.
 * Scratch is allocated by the first call and freed with the key frames.  Positions are served P = min(M, 8) at a time, so with
 * T = ceil(w / 64) * ceil(h / 64) field tiles it is
 *     nseq x P x (max_points x (72 + 4 T) B + ceil(w / 8) x ceil(h / 4) x 64 B + ceil(max_points / 256) x 256 B + 5.1 kB)
 *   + nseq x M x (max_points x 4 B + 0.6 kB)                                  (the links and the results of every position)
 * — the key frame's compact KeyLines 48 B, three residual buffers 24 B and the field's bins 4 T B per KeyLine of a pair; its index plane;
 * carries and partial sums per block of 256 KeyLines; the minimiser's state.  752x480 (T = 96), 16 000 KeyLines: 7.4 MB per pair. */
typedef struct edgehip_kf_reloc_args {
    int32_t field_radius; float field_min_mod;   /* as edgehip_kf_covis_args; the radius is build_field's: 1 .. 255 */
    int32_t iter_max; double rew_dis, rho_tol;
} edgehip_kf_reloc_args;
typedef struct edgehip_kf_reloc {
    double X[6], RRV[36], score_ratio, F, F0, Kp, K, Pose[9], Pos[3];
    int32_t mnum, evals, accepted, guard;
} edgehip_kf_reloc;
/* pose[nseq], or NULL for what edgehip_keyframe_insert takes by default; s_rho_q[nseq]; to_mask[nseq][M] (non-zero: serve the position),
 * or NULL for all; out[nseq][M]; info[nseq] (may be NULL) as in edgehip_keyframe_covisibility_slot.  A position the sequence does not
 * have, or that to_mask deselects, comes back with every integer field -1 (and zeros).  Synchronises.  EDGEHIP_ERR_STATE without
 * key-frame tracking; EDGEHIP_ERR_ARG for NULL args, s_rho_q or out, a slot out of range, field_radius outside 1 .. 255, iter_max < 0
 * or max_points > 65535; EDGEHIP_ERR_MEMORY when the scratch cannot be allocated: the context stays usable. */
int edgehip_keyframe_relocalize(edgehip_ctx *ctx, int slot, const edgehip_kf_pose *pose, const double *s_rho_q, const uint8_t *to_mask,
                                const edgehip_kf_reloc_args *args, edgehip_kf_reloc *out, edgehip_kf_list_info *info);
/* The links of the last call's pair (seq, position): m_id_f[kn] (room for max_points; may be NULL), the query KeyLine's partner in key
 * frame `position` or -1; kn_out = -1 (and nothing written) for a pair the last call did not serve.  Synchronises. */
int edgehip_keyframe_relocalize_links(edgehip_ctx *ctx, int seq, int position, int32_t *m_id_f, int32_t *kn_out);
/* Device time of the last edgehip_keyframe_relocalize, by HIP events: prepare (descriptors, the one read of the key frames, set-up,
 * fields) and solve (the minimisation's launch chain, the count, the scale and the finish). */
int edgehip_keyframe_relocalize_ms(edgehip_ctx *ctx, double *prepare_ms, double *solve_ms);

/* ---- key-frame relative-pose constraint (kfvo::OptimizeRelContraint) ------------------------------------------------------------
 * The metric use of the links the tracking above maintains: from the key frame's m_id_f (direction 0) or the frame list's m_id_kf
 * (direction 1) alone, with no distance field, kfvo::OptimizeRelContraint (src/mtracklib/kfvo.cpp:527-604; its evaluation
 * OptimizeRelConstraint1Iter, :344-420) makes a 6-DoF relative pose X = [BRelPos, ln(BRelRot)], its information matrix W_X = JtJ, its
 * covariance R_X = Cholesky<6>(JtJ).get_inverse() and, for direction 1, the scale ratio of optimizeScaleF2KF (:263-302) with its weight:
 * the fields relPosPose, WrelPosPose, K, WK of the OdometryMeas the reference's pose_graph keeps per key frame
 * (include/mtracklib/pose_graph.h:31-47).  Upstream defines the function and never calls it.  Every sequence's current key frame is
 * constrained against ring slot slot_new in one call; all arithmetic is fp64 in the reference's order per KeyLine, the sums over
 * KeyLines run in a fixed order of the device's own (tests/keyframe_constraint_port.py restates the rules).
 *     direction 1   walks the slot's KeyLines, partner = key frame's KeyLine m_id_kf; start pose BRelRot = kf.Pose^T * Pose,
 *                   BRelPos = kf.Pose^T * (Pos - kf.Pos) / K (:538-541)
 *     direction 0   walks the key frame's KeyLines, partner = the slot's KeyLine m_id_f; BRelRot = Pose^T * kf.Pose,
 *                   BRelPos = Pose^T * (kf.Pos - Pos) / kf.K (:542-544)
 * The reference has no defined result for a sequence without links (it aborts in SO3::coerce) or with a NaN on a linked KeyLine; here
 *     guard bit 0   the sequence stopped stepping at a non-finite dX or JtJ; X is the last accepted pose (the start pose if none)
 *     guard bit 1   the last evaluation counted fewer than 6 links (the reference's arithmetic still runs; the result means nothing)
 *     guard bit 2   a link outside the list it indexes was taken as unmatched (the reference reads out of bounds)
 * and none of them stops the other sequences of the batch.  A sequence without a key frame has no links. */
typedef struct edgehip_kf_constraint_args { int32_t direction, iter_max; double k_huber; } edgehip_kf_constraint_args;
typedef struct edgehip_kf_constraint {
    double X[6], W_X[36], R_X[36];
    double ratio, E, E0;          /* E/E0 (the return value), and both terms */
    double Kp, W_Kp;              /* optimizeScaleF2KF; 0, 0 for direction 0 */
    int32_t links, inliers;       /* match_num of the LAST evaluation */
    int32_t evals, accepted, guard, pad;
} edgehip_kf_constraint;
/* Pose[nseq][9], Pos[nseq][3], K[nseq], or all three NULL for what edgehip_keyframe_forward_correct takes by default and
 * edgehip_seq_state::K.  out[nseq].  Read-only on the key frames and the slot.  Synchronises.  EDGEHIP_ERR_STATE without key-frame
 * tracking; EDGEHIP_ERR_ARG for NULL args or out, iter_max < 0, a direction that is not 0 or 1, a slot out of range, or some but not
 * all of Pose, Pos, K; EDGEHIP_ERR_MEMORY when the scratch (92 B x max_points x nseq, allocated by the first call and freed with the
 * key frames) cannot be allocated: the context stays usable. */
int edgehip_keyframe_constraint(edgehip_ctx *ctx, int slot_new, const double *Pose, const double *Pos, const double *K,
                                const edgehip_kf_constraint_args *args, edgehip_kf_constraint *out);
/* kfvo::mutualExclusionSimple(kf, slot_new, dist_t, discard_non_mutual, kf_to_frame) (kfvo.cpp:423-522): the pruning pass in front of
 * the constraint.  kf_to_frame = 1 edits the key frame's m_id_f (a link whose partner does not link back is dropped when
 * discard_non_mutual; one whose partner links back to a KeyLine further than dist_t away, by the Euclidean distance of the float p_m,
 * is dropped), kf_to_frame = 0 the slot's m_id_kf (the distance is |difference . u_m| in float); nothing else changes.  In-stream like
 * the correct steps; counts[nseq][2] (may be NULL: no synchronisation) = (links seen, links kept).  A link outside the list it indexes
 * is left alone and not counted; a back link outside the walked list is seen, not kept, and left alone (the reference reads out of
 * bounds in both cases).  EDGEHIP_ERR_STATE and EDGEHIP_ERR_ARG for the slot as above; the call allocates nothing (its counts live
 * with the key frames). */
int edgehip_keyframe_mutual_exclusion(edgehip_ctx *ctx, int slot_new, double dist_t, int discard_non_mutual, int kf_to_frame, int32_t *counts);
/* Device time of the last edgehip_keyframe_constraint, by HIP events: the link gather and the solve. */
int edgehip_keyframe_constraint_ms(edgehip_ctx *ctx, double *gather_ms, double *solve_ms);

/* ---- key-frame depth along the links (kfvo::mapKFUsingIDK, translateDepth_F2KF / _KF2F / _New2Old) -----------------------------------
 * The other half of key-frame mapping: the links the tracking above maintains MOVE depth.  Upstream defines these functions and never
 * calls them; nothing here runs inside edgehip_process_frame.  All arithmetic is fp64 in the reference's order of operations per
 * KeyLine (p_m, u_m: the records' floats widened); relative poses are formed as TooN forms them (row dot products from 0 in index
 * order), on the device, the same way for every sequence (tests/keyframe_depth_port.py restates the rules).  Every rho /
 * s_rho written equals the reference's bit for bit (NaN as a class).
 *   result      out[nseq]: count = links used, guard, and for translate_depth K = the kf.K the rewrite used (0 for a sequence without a
 *               key frame), rTr, rTr0 = optimizeScaleBack's sums (0 without optim_scale).
 *   guard bit 2   a link outside the list it indexes was taken as unmatched (the reference reads out of bounds), as above
 *   guard bit 0   optimizeScaleBack made a non-finite K: kf.K is left as it was and the rewrite runs with the old K
 * A sequence without a key frame has no links: count 0, nothing written; no guard stops the other sequences.
 * Pose[nseq][9], Pos[nseq][3] (and K[nseq] where the call has it) are given together, or all NULL for what edgehip_keyframe_constraint
 * takes by default.  EDGEHIP_ERR_STATE without key-frame tracking; EDGEHIP_ERR_ARG for a slot out of range or some but not all of the
 * pose arguments; EDGEHIP_ERR_MEMORY when the scratch (137 B x nseq, allocated by the first of these calls, freed with the key frames)
 * cannot be allocated: the context stays usable. */
typedef struct edgehip_kf_depth {
    int32_t count, guard;
    double K, rTr, rTr0;
} edgehip_kf_depth;
/* kfvo::mapKFUsingIDK(kf, slot_new, Pose, Pos, ReshapeQAbsolute, ReshapeQRelative, LocationUncertainty) (src/mtracklib/kfvo.cpp:1147-1184):
 * FRelRot = Pose^T * kf.Pose, FRelPos = Pose^T * (kf.Pos - Pos), no division by a scale; one kfvo::mapKLUsingIDK (the live definition,
 * :1276-1360, through rotateQs, include/mtracklib/kfvo.h:68-81, which returns zeros when qr[2] == 0) for every key-frame KeyLine with
 * m_id_f >= 0 against the slot's KeyLine m_id_f, zf = cam.zfm.  The clamp chain keeps its order and its holes: rho < RHO_MIN: s_rho +=
 * RHO_MIN - rho, rho = RHO_MIN (a NaN s_rho stays NaN); rho > RHO_MAX: rho = RHO_MAX; a NaN or infinity in either: (RhoInit, RHO_MAX);
 * s_rho < 0: (RhoInit, RHO_MAX); RHO_MAX = 20, RHO_MIN = 1e-3, RhoInit = 1 (edge_finder.h:38-40).  Writes the key frame's rho and s_rho
 * at linked indices and nothing else.  In-stream; synchronises only when out != NULL.  out: (links updated, guard, 0, 0, 0). */
int edgehip_keyframe_map_depth(edgehip_ctx *ctx, int slot_new, const double *Pose, const double *Pos, double reshape_q_abs,
                               double reshape_q_rel, double location_uncertainty, edgehip_kf_depth *out);
/* direction 0: kfvo::translateDepth_F2KF(kf, slot_new, Pose, Pos, K, optim_scale) (:653-686): BRelRot = kf.Pose^T * Pose, BRelPos =
 *   kf.Pose^T * (Pos - kf.Pos); with optim_scale first kf.K = optimizeScaleBack(...) (:305-341: sums over the key frame's linked
 *   KeyLines with q1[2] > 0, through kfvo::unProject / kfvo::project, kfvo.h:42-48; summed in a fixed order of the device's own, so K,
 *   rTr, rTr0 and what follows from K agree with the reference to rounding, and are the same bits alone and inside any batch); then
 *   for every linked key-frame KeyLine rho = q1[2] * kf.K, s_rho = rho * (kl.s_rho / kl.rho), m_num++, with q1 =
 *   cam.projectHomCordVec(BRelRot * cam.unprojectHomCordVec(p_m.x, p_m.y, rho) * K + BRelPos) of the slot's KeyLine m_id_f.  Writes the
 *   key frame's rho, s_rho, m_num at linked indices, and with optim_scale the key frame's pose block K; the slot is untouched.
 * direction 1: kfvo::translateDepth_KF2F(kf, slot_new, Pose, Pos, K) (:607-634): BRelRot = Pose^T * kf.Pose, BRelPos = Pose^T * (kf.Pos -
 *   Pos); for every slot KeyLine with m_id_kf >= 0: rho = q1[2] * kf.K, s_rho = rho / kl.rho * kl.s_rho (the other association), q1 from
 *   the key frame's KeyLine m_id_kf.  THIS IS THE ONE KEY-FRAME CALL THAT WRITES INTO A FRAME SLOT: the slot's rho and s_rho at linked
 *   indices, which the next frame's tracking and mapping then read; the key frame is untouched.  (No packed per-slot copy of rho / s_rho
 *   exists beside the arrays, so nothing else is refreshed.)  optim_scale must be 0 (EDGEHIP_ERR_ARG).
 * In-stream; synchronises only when out != NULL. */
int edgehip_keyframe_translate_depth(edgehip_ctx *ctx, int slot_new, int direction, const double *Pose, const double *Pos, const double *K,
                                     int optim_scale, edgehip_kf_depth *out);
/* kfvo::translateDepth_New2Old(kf_list, iters) (:637-650) over what the device holds of kf_list, per sequence: the held list entries,
 * oldest first, then the current key frame (the positions of edgehip_keyframe_covisibility).  For consecutive positions (i, i + 1):
 * translateDepth_F2KF without the scale step from i + 1 into i, with i + 1's header Pose, Pos, K and i's own K; position i's m_id_f
 * index position i + 1's KeyLines (so it is when i + 1 was taken by the frame driver's criterion from the frame i was last repaired
 * against, or when a caller built the list so); a link outside [0, kn of i + 1) is skipped and sets guard bit 2.  As in the
 * reference's ascending walk every position reads its successor as it was before the iteration, and iteration n + 1 reads iteration
 * n's results.  The list entries' rho, s_rho, m_num change in place, every other byte of the 168-byte records stays; the newest
 * position is only read.  out[nseq] (may be NULL) = (links of the last iteration over all positions, guard, 0, 0, 0).  Synchronises.
 * EDGEHIP_ERR_STATE without the key-frame list, EDGEHIP_ERR_ARG for iters < 0; iters == 0 does nothing. */
int edgehip_keyframe_list_translate_depth(edgehip_ctx *ctx, int iters, edgehip_kf_depth *out);
/* Restricts the three calls above to the sequences with mask[seq] != 0 (mask[nseq]; NULL: every sequence again, the default): the others
 * are treated as sequences without a key frame — count 0, K 0, nothing written.  For a caller that serves one sequence's request in a
 * batch whose other sequences did not ask (the mirror's REBVO::keyframeMapDepth).  Holds until changed or until the key frames are
 * freed.  Synchronises (mask != NULL).  EDGEHIP_ERR_STATE without key-frame tracking. */
int edgehip_keyframe_depth_select(edgehip_ctx *ctx, const uint8_t *mask);
/* Device time of the last of the three calls above, by HIP events (waits for that call's end). */
int edgehip_keyframe_depth_ms(edgehip_ctx *ctx, double *ms);

/* ---- the frame as a baseline JPEG (the MJPEG video path) --------------------------------------------------------------------
 * What the reference's output thread does with a finished frame before it sends or saves it (rebvo_third_t.cpp:184-257): MJPEGEncoder
 * at quality 90 (video_mjpeg.cpp:63-74), i.e. gdImageJpegPtr, i.e. libjpeg after jpeg_set_defaults and jpeg_set_quality(q, TRUE):
 * baseline, 8 bit, YCbCr 4:2:0, the Annex-K Huffman tables (not optimised), the islow integer DCT, no restart markers.  The device
 * encoder follows that in integers only (the rule is written out in rebvo/jpeg_encode.h and DESIGN.md §19) and its stream is libjpeg's
 * byte for byte: SOI, APP0 (JFIF 1.01, units 0, density 1x1, no thumbnail), the optional COM segment, DQT 0, DQT 1, SOF0, four DHT, SOS
 * (623 bytes without a comment), the entropy-coded data, EOI.  An image's bytes do not depend on the batch it is encoded in.
 * What could NOT be compared is gd's own decoration of the header, because no libgd was available where this was written: gd writes a
 * COM segment of the form "CREATOR: gd-jpeg v1.0 (using IJG JPEG v<N>), quality = 90\n" (pass that text as `comment` to get it at the
 * place jpeg_write_marker puts it, directly behind APP0), and newer gd versions write the image's resolution into APP0's density
 * fields, which stay 1x1 without units here. */
typedef struct edgehip_jpeg_size {
    uint32_t size;          /* the stream's true length in bytes, also when it did not fit */
    uint32_t overflow;      /* 1: size > cap_bytes; the region then holds the stream's first cap_bytes bytes */
} edgehip_jpeg_size;
/* No stream of a w x h image is longer than this: 623 + the COM segment (comment_len + 4, when there is one) + 2 * ceil(nblocks *
 * (22 + 63 * 26) / 8) + 2 with nblocks = 6 * ceil(w / 16) * ceil(h / 16) — every block at its longest code, every data byte stuffed.
 * 0 for w or h < 1. */
uint64_t edgehip_jpeg_bound(int w, int h, uint32_t comment_len);
/* Allocates the store: nseq regions of cap_bytes (each starting on a 16-byte boundary: the stride is cap_bytes rounded up to 16), nseq
 * size records, the tables of `quality` and the header (with `comment`, a C string, as COM segment; NULL: none), all regions zero.
 * cap_bytes == 0 frees the store.  EDGEHIP_ERR_ARG for a quality outside 1..100, a comment above 65533 bytes or a cap_bytes below
 * header + EOI; EDGEHIP_ERR_MEMORY when the allocation fails (the store is then off; the context stays usable). */
int edgehip_jpeg_enable(edgehip_ctx *ctx, int quality, uint32_t cap_bytes, const char *comment /* or NULL */);
/* The frame every sequence holds in `slot` becomes one JPEG in the sequence's region, in-stream (no synchronisation).  The frame is
 * read where stage A reads it — the slot's RGB24 or 8-bit mono storage (a mono value v is R = G = B = v: Y = v, Cb = Cr = 128), or the
 * frames of a bound pool — and, on a context with use_undistort, resampled as edgehip_download_undistorted resamples it (what
 * PipeBuffer::imgc holds).  A stream longer than cap_bytes leaves its true size and the overflow flag in the record and its first
 * cap_bytes bytes in the region; nothing is written past a region.  Uploads enqueued afterwards (into any slot: the upload streams
 * wait as a whole) wait for the encoder's reads, so call it where the next frame's upload may wait for the frame before.
 * edgehip_process_frame enqueues nothing of this.  A slot that never received a frame is encoded as its storage stands (zeros after
 * edgehip_create).  EDGEHIP_ERR_STATE when the store is off, EDGEHIP_ERR_ARG for a slot out of range. */
int edgehip_jpeg_encode(edgehip_ctx *ctx, int slot);
/* Restricts edgehip_jpeg_encode to the sequences with mask[seq] != 0 (mask[nseq]; NULL: every sequence again, the default): the regions
 * and size records of the others stay as they are.  Holds until changed or until the store is freed.  Synchronises (mask != NULL). */
int edgehip_jpeg_select(edgehip_ctx *ctx, const uint8_t *mask);
/* Sequence seq's stream: min(size, cap_bytes, cap) bytes into dst (may be NULL), the record into *size (may be NULL).  Synchronises. */
int edgehip_download_jpeg(edgehip_ctx *ctx, int seq, uint8_t *dst, uint32_t cap, edgehip_jpeg_size *size);
/* The same for n sequences seqs[n] (dst[j] with room for cap bytes each, sizes[n]; either array or any dst[j] may be NULL): the
 * records in one copy, then the streams.  Synchronises twice at most, whatever n. */
int edgehip_download_jpeg_batch(edgehip_ctx *ctx, int n, const int32_t *seqs, uint8_t *const *dst, uint32_t cap, edgehip_jpeg_size *sizes);
/* The regions of sequences [first, first + count) into DEVICE memory of the context's GPU: bytes_dev[count][stride] with stride =
 * cap_bytes rounded up to 16, sizes_dev[count] records (either may be NULL; e.g. torch uint8 tensors), without a host bounce — like
 * edgehip_net_keylines_device.  The copy is complete on return. */
int edgehip_jpeg_device(edgehip_ctx *ctx, int first, int count, void *bytes_dev, void *sizes_dev);
/* For output callbacks at full pipeline depth, through a staging ring like edgehip_export_keylines' (four tickets): the frames that
 * sequences seqs[n] hold in `slot` are encoded in-stream (no synchronisation) into a ring entry, n regions in the order of seqs; the
 * slot's frames and the store's regions are free again as far as the export goes.  edgehip_jpeg_export_sizes(ticket, sizes[n]) waits
 * for that encoder alone (an event, no stream) and gives the records; edgehip_jpeg_export_fetch(ticket, dst[n]) enqueues the copies
 * of min(size, cap_bytes) bytes each on the ring's own stream (dst[j] NULL: skipped; straight into memory of edgehip_register_host,
 * through a page-locked mirror otherwise) and does not wait for them; edgehip_jpeg_export_wait(ticket) blocks until they have landed
 * (a ticket never fetched: until its encoder has run) and releases the ticket.  The select mask does not apply.  EDGEHIP_ERR_STATE
 * when the store is off or four tickets are outstanding; edgehip_jpeg_enable drops outstanding tickets. */
int edgehip_jpeg_export(edgehip_ctx *ctx, int slot, int n, const int32_t *seqs, int *ticket_out);
int edgehip_jpeg_export_sizes(edgehip_ctx *ctx, int ticket, edgehip_jpeg_size *sizes);
int edgehip_jpeg_export_fetch(edgehip_ctx *ctx, int ticket, uint8_t *const *dst);
int edgehip_jpeg_export_wait(edgehip_ctx *ctx, int ticket);
/* The stage-level, geometry-free entry: `count` packed RGB24 images of w x h >= 1 x 1 in device memory (image i at rgb24_dev + i * w *
 * h * 3) through the same kernel, image i's stream to out_dev + i * cap and its record to sizes_dev[i] (edgehip_jpeg_size).  The
 * context's own sizes are multiples of 8 or 16 and never reach the padding and dummy-block rules; this entry does (tests), and it
 * compresses what is already on the device, e.g. edgehip_depth_image renderings.  No comment segment.  cap is a multiple of 16 and at
 * least 625, out_dev 16-byte aligned, w and h at most 65535 with w * h * 3 < 2^31 and edgehip_jpeg_bound(w, h, 0) < 2^31 (sizes and caps
 * are 32-bit: about 320 megapixels; EDGEHIP_ERR_ARG beyond, as in edgehip_jpeg_enable); needs no store.  The images are done on return. */
int edgehip_jpeg_encode_images(edgehip_ctx *ctx, const void *rgb24_dev, int w, int h, int count, int quality, void *out_dev, uint32_t cap,
                               void *sizes_dev);

/* ---- baseline JPEG frames decoded on the device (MJPEG ingest; jpeg_decode.hip) ------------------------------------
 * The counterpart of the encoder above: a camera's JPEG crosses the bus instead of its pixels and is decoded into the slot's own frame
 * storage, with the host reader's (libjpeg's) pixel values: Huffman decoding, jpeg_idct_islow, fancy upsampling, ycc_rgb_convert, in
 * integers only.  Decodable on the device: SOF0 / SOF1, 8-bit, one scan over every component, grey or YCbCr 4:4:4 / 4:2:2 (h2v1) /
 * 4:2:0 (h2v2), any DHT tables, any restart interval.  Everything else gets a reason code (rebvo/jpeg_decode.h: 1 truncated header or
 * not a JPEG, 2 progressive, 3 lossless / hierarchical / arithmetic, 4 not 8-bit, 5 neither 1 nor 3 components, 6 sampling, 7 more than
 * one scan, 8 not YCbCr, 9 a missing or invalid table, 10 a malformed segment, 11 not the expected size, 12 longer than cap_bytes). */
#define EDGEHIP_FRAME_RGB24 0
#define EDGEHIP_FRAME_GREY8 1
#define EDGEHIP_JPEG_REASON_WALK 100 /* edgehip_jpeg_decode_images: reason 100 + s, the entropy walk ended with status s */
typedef struct edgehip_jpeg_info {
    int32_t w, h, components, hsamp, vsamp; /* the first component's sampling factors: (1,1), (2,1) or (2,2) when decodable */
    int32_t restart_interval;
    uint32_t entropy_offset, entropy_length; /* the entropy-coded segment: behind the scan header, up to the first marker but RSTn */
    int32_t reason;                          /* 0: decodable on the device */
} edgehip_jpeg_info;
/* Parses the stream's markers up to its scan (host only, no context).  Returns 0 with info->reason set; EDGEHIP_ERR_ARG for info == NULL. */
int edgehip_jpeg_probe(const uint8_t *data, size_t len, edgehip_jpeg_info *info);
/* Room for max_streams (<= nseq) compressed frames per call, cap_bytes of entropy-coded data each: page-locked and device regions,
 * descriptors, coefficient (2 B) and sample (1 B) planes per padded sample of any sampling of the context's frame, and status words.
 * cap_bytes == 0 frees it.  EDGEHIP_ERR_MEMORY when an allocation fails (the decoder is then off; the context stays usable).  A context
 * that never calls this allocates and launches nothing new. */
int edgehip_jpeg_decode_enable(edgehip_ctx *ctx, int max_streams, uint32_t cap_bytes);
/* data[count] / len[count]: one JPEG per sequence seq_first .. seq_first + count - 1, into `slot`'s own storage as RGB24
 * (EDGEHIP_FRAME_RGB24) or, when every stream has one component, as the 8-bit plane (EDGEHIP_FRAME_GREY8: what edgehip_upload_grey8
 * leaves; a colour stream is EDGEHIP_ERR_ARG).  All or nothing: the headers are parsed on the host first, and if any stream is not
 * decodable on the device — including one that is not the context's w x h or whose entropy-coded segment exceeds cap_bytes — nothing is
 * enqueued, slot and storage stay as they were, reason_out[count] (or NULL) says why per stream and the call returns EDGEHIP_ERR_ARG:
 * decode on the host and use the raw upload.  Otherwise the segments and descriptors go up asynchronously on the upload stream and the
 * kernels run there, ordered like edgehip_upload_rgb_pinned: behind the slot's last use, ahead of the slot's stage A.  The caller's
 * buffers are free on return.  A corrupt or short segment is found on the device: see edgehip_read_jpeg_decode_status.
 * EDGEHIP_ERR_STATE when the decoder is off. */
int edgehip_upload_jpeg(edgehip_ctx *ctx, int slot, const uint8_t *const *data, const size_t *len, int seq_first, int count, int format,
                        int32_t *reason_out /* or NULL */);
/* status[nseq]: per sequence, how the entropy walk of the slot's last compressed upload ended — 0 complete, 1 invalid code, 2 out of
 * data, 3 a DC or coefficient outside the range the host reader accepts, 4 a run past the block's end (the largest over the stream's
 * restart-interval groups).  A stream with a nonzero status leaves unspecified pixels in its own frame; the others are untouched.
 * Synchronises the upload stream. */
int edgehip_read_jpeg_decode_status(edgehip_ctx *ctx, int slot, int32_t *status);
/* Measurement (tools/jpeg_decode_timing.py): device time of the three kernels of the last edgehip_upload_jpeg (entropy walk, inverse
 * DCT, pixels) in milliseconds, and the bytes its two host-to-device copies moved (segments padded to 16 bytes, descriptors).  The
 * events are recorded only for an upload made under edgehip_profile_enable(ctx, 1): EDGEHIP_ERR_STATE otherwise.  Waits for them. */
int edgehip_jpeg_decode_ms(edgehip_ctx *ctx, float ms[3], uint64_t *bytes_moved /* or NULL */);
/* The stage-level, geometry-free entry, counterpart of edgehip_jpeg_encode_images: `count` streams of one size w x h >= 1 x 1, image i as
 * packed RGB24 to rgb24_dev_out + i * w * h * 3 (device memory, any alignment; nothing outside count * w * h * 3 bytes is written).
 * Needs no edgehip_jpeg_decode_enable; done on return.  EDGEHIP_ERR_ARG with reason_out[count] (or NULL) filled when a stream is not
 * decodable or not w x h (nothing is written then), or when a walk ended with status s (reason 100 + s; that image is unspecified). */
int edgehip_jpeg_decode_images(edgehip_ctx *ctx, const uint8_t *const *data, const size_t *len, int count, int w, int h, void *rgb24_dev_out,
                               int32_t *reason_out /* or NULL */);
/* The slot's own frame storage of sequence `seq` as it stands: w * h * 3 bytes RGB24 or w * h bytes 8-bit mono, *format (or NULL) says
 * which.  Synchronises.  EDGEHIP_ERR_STATE for a slot bound to a frame pool. */
int edgehip_download_frame(edgehip_ctx *ctx, int seq, int slot, uint8_t *out, int *format);

/* ---- measurement ------------------------------------------------------------------------------------- */
/* Names of the kernel groups timed by the built-in HIP-event profiler, and their accumulated device time.
 * edgehip_profile_enable(ctx, 1) brackets every launch group with events on the context stream (adds host
 * overhead: use for attribution, not for throughput).  ms[n], calls[n] with n = edgehip_profile_count(). */
int edgehip_profile_enable(edgehip_ctx *ctx, int on);
/* Restrict the profiler to the groups whose bit is set (bit i = group i); default: all. */
int edgehip_profile_select(edgehip_ctx *ctx, uint64_t mask);
int edgehip_profile_count(void);
const char *edgehip_profile_name(int i);
int edgehip_profile_read(edgehip_ctx *ctx, double *ms, int64_t *calls); /* synchronises, then resets */

#ifdef __cplusplus
}
#endif
#endif /* EDGEHIP_H */
