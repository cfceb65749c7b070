// Flat C entry of rebvo/keyframe_reloc.h for ctypes (tests/test_keyframe_reloc_cpu.py): one (query, key frame) pair.
#include "rebvo/keyframe_reloc.h"

// q_* / t_*: the query's and the key frame's KeyLines ([kn][2] floats for p_m, c_p, u_m, m_m; [kn] n_m; [kn] doubles rho, s_rho);
// q_pose / t_pose: Pose[9], Pos[3], K; cam: w, h as doubles, ppx, ppy, zfm; args: field_radius, field_min_mod, iter_max, rew_dis, rho_tol,
// s_rho_q; out: X[6], RRV[36], score_ratio, F, F0, Kp, K, Pose[9], Pos[3] (59 doubles); ints: mnum, evals, accepted; m_id_f[q_kn] or null.
extern "C" int rebvo_keyframe_relocalize_c(int q_kn, const float *q_pm, const float *q_cp, const float *q_um, const float *q_mm, const float *q_nm,
                                           const double *q_rho, const double *q_srho, const double *q_pose, int t_kn, const float *t_pm,
                                           const float *t_cp, const float *t_um, const float *t_mm, const float *t_nm, const double *t_rho,
                                           const double *t_srho, const double *t_pose, const double *cam, const double *args, double *out,
                                           int32_t *ints, int32_t *m_id_f) {
    if (q_kn < 0 || t_kn < 0 || !q_pose || !t_pose || !cam || !args || !out || !ints) return -1;
    const rebvo::RelocKeyLines q = {q_kn, q_pm, q_cp, q_um, q_mm, q_nm, q_rho, q_srho}, t = {t_kn, t_pm, t_cp, t_um, t_mm, t_nm, t_rho, t_srho};
    const rebvo::RelocCamera c = {(int)cam[0], (int)cam[1], (float)cam[2], (float)cam[3], cam[4]};
    const rebvo::RelocArgs a = {(int)args[0], (float)args[1], (int)args[2], args[3], args[4], args[5]};
    if (c.w < 1 || c.h < 1 || a.field_radius < 1 || a.iter_max < 0) return -1;
    rebvo::RelocResult r;
    rebvo::rebvo_keyframe_relocalize(q, q_pose, q_pose + 9, q_pose[12], t, t_pose, t_pose + 9, t_pose[12], c, a, r, m_id_f);
    double *o = out;
    for (double x : r.X) *o++ = x;
    for (double x : r.RRV) *o++ = x;
    *o++ = r.score_ratio; *o++ = r.F; *o++ = r.F0; *o++ = r.Kp; *o++ = r.K;
    for (double x : r.Pose) *o++ = x;
    for (double x : r.Pos) *o++ = x;
    ints[0] = r.mnum; ints[1] = r.evals; ints[2] = r.accepted;
    return 0;
}
