// linalg_check — rebvo/linalg.h on a fixed list of small inputs, one line of hex doubles per result.
//
// tests/test_linalg_cpu.py builds this with the host compiler (-ffp-contract=off) and compares the output line by line
// with tests/golden/linalg/linalg_check.txt, which holds what the tracker's and the glue's former private copies of
// the same algebra (and the header as it was) gave on these inputs: see DESIGN.md, "One copy of the algebra".
// A second build with -fsanitize=address,undefined runs the same list.
//
// Numbers are printed with %a (exact); every NaN prints as "nan" (its sign and payload depend on operand order, which a
// compiler may choose).  The inputs use +, -, *, / and sqrt only (the rotations given to ln come from so3_exp, which has its own
// rows), so what the fixture pins beyond IEEE arithmetic is the host's sin, cos, asin and acos.
#include <cstdio>
#include <initializer_list>

#include "rebvo/linalg.h"

using namespace rebvo::la;

// ---- inputs ---------------------------------------------------------------------------------------------------------
// Q diag(eig) Q^T, Q a product of Givens rotations with rational (c, s) over every pair of axes; symmetric by construction
template <int N>
static Mat<N, N> sym_from_eig(const double (&eig)[N], int seed) {
    static const double cs[4][2] = {{3.0 / 5, 4.0 / 5}, {5.0 / 13, 12.0 / 13}, {8.0 / 17, 15.0 / 17}, {7.0 / 25, 24.0 / 25}};
    Mat<N, N> Q = Mat<N, N>::identity();
    int k = seed;
    for (int p = 0; p < N - 1; p++)
        for (int q = p + 1; q < N; q++, k++) {
            const double c = cs[k % 4][0], s = (k % 3 == 0 ? -1.0 : 1.0) * cs[k % 4][1];
            for (int r = 0; r < N; r++) { const double a = Q(r, p), b = Q(r, q); Q(r, p) = c * a - s * b; Q(r, q) = s * a + c * b; }
        }
    Mat<N, N> QD = Q;
    for (int r = 0; r < N; r++) for (int c = 0; c < N; c++) QD(r, c) = Q(r, c) * eig[c];
    Mat<N, N> A = QD * transpose(Q);
    for (int r = 0; r < N; r++) for (int c = r + 1; c < N; c++) A(c, r) = A(r, c);
    return A;
}
template <int N>
static Mat<N, N> spd(double cond, int seed) {   // eigenvalues from 1 down to 1 / cond
    double eig[N];
    for (int i = 0; i < N; i++) eig[i] = 1.0 / (1.0 + (cond - 1.0) * i / (N - 1));
    return sym_from_eig<N>(eig, seed);
}
// L D L^T in small integers and powers of two (exact in fp64, and exact through the factorisation), D[k] = dk
template <int N>
static Mat<N, N> ldlt_int(int k, double dk) {
    static const double D0[7] = {4, 2, 8, 1, 2, 4, 2};
    Mat<N, N> L = Mat<N, N>::identity(), D = Mat<N, N>::zeros();
    for (int i = 0; i < N; i++) {
        D(i, i) = (i == k) ? dk : D0[i];
        for (int j = 0; j < i; j++) L(i, j) = (double)((i * 3 + j * 5) % 5 - 2);
    }
    return L * D * transpose(L);
}
template <int N>
static Vec<N> rhs(double scale) {
    Vec<N> b;
    for (int i = 0; i < N; i++) b[i] = (double)((i * 7 + 3) % 11 - 5) * scale;
    return b;
}
template <int N>
static double max_abs(const Mat<N, N> &A) {
    double m = 0;
    for (int i = 0; i < N * N; i++) m = std::fmax(m, std::fabs(A.a[i]));
    return m;
}
static Mat<3, 3> phi_t_phi(int win_s) {   // the plane fit's normal matrix (edge_finder.cpp:83-100)
    Mat<3, 3> A = Mat<3, 3>::zeros();
    for (int i = -win_s; i <= win_s; i++)
        for (int j = -win_s; j <= win_s; j++) {
            const double phi[3] = {(double)j, (double)i, 1.0};
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) A(r, c) += phi[r] * phi[c];
        }
    return A;
}

// ---- output ---------------------------------------------------------------------------------------------------------
static void put(const char *name, const char *what, const double *v, int n) {
    std::printf("%s.%s", name, what);
    for (int i = 0; i < n; i++) {
        if (std::isnan(v[i])) std::printf(" nan");
        else std::printf(" %a", v[i]);
    }
    std::printf("\n");
}

// ---- the operations ---------------------------------------------------------------------------------------------------
template <int N>
static void chol_case(const char *name, const Mat<N, N> &A) {
    const Cholesky<N> ch(A);
    put(name, "L", ch.L.a, N * N);
    put(name, "backsub", ch.backsub(rhs<N>(0.375)).v, N);
    put(name, "inverse", ch.inverse().a, N * N);
}
template <int N>
static void chol_cases(const char *n) {
    char name[64];
    const double conds[3] = {10, 1e3, 1e5};
    for (int i = 0; i < 3; i++) { std::snprintf(name, sizeof name, "chol%s_cond%d", n, i); chol_case<N>(name, spd<N>(conds[i], i)); }
    const int cols[3] = {0, N / 2, N - 1};
    for (int i = 0; i < 3; i++) { std::snprintf(name, sizeof name, "chol%s_zero_pivot_col%d", n, cols[i]); chol_case<N>(name, ldlt_int<N>(cols[i], 0.0)); }
    std::snprintf(name, sizeof name, "chol%s_negative_pivot", n);
    chol_case<N>(name, ldlt_int<N>(1, -2.0));
    Mat<N, N> A = spd<N>(10, 3);
    A(1, 2) = A(2, 1) = NAN;
    std::snprintf(name, sizeof name, "chol%s_nan_entry", n);
    chol_case<N>(name, A);
}
static void svd6_case(const char *name, const double (&eig)[6], int seed) {
    const Mat<6, 6> A = sym_from_eig<6>(eig, seed);
    const Vec<6> b = rhs<6>(0.25 * max_abs(A));
    const SymSVD<6> svd(A);
    const Mat<6, 6> P = svd.pinv();
    put(name, "pinv", P.a, 36);
    put(name, "pinv_times_b", (P * b).v, 6);
    put(name, "backsub", svd.backsub(b).v, 6);
}
static void exp_case(const char *name, double x, double y, double z) {
    put(name, "R", so3_exp(Vec<3>{{x, y, z}}).a, 9);
}
static void ln_case(const char *name, const Mat<3, 3> &M) { put(name, "w", so3_ln_raw(M).v, 3); }
static void ln_of_exp(const char *name, double angle, double x, double y, double z) {
    const double s = angle / std::sqrt(x * x + y * y + z * z);
    ln_case(name, so3_exp(Vec<3>{{x * s, y * s, z * s}}));
}
static void inv3_case(const char *name, const Mat<3, 3> &A) {
    const double det = det3_gauss(A);
    put(name, "det", &det, 1);
    put(name, "inverse", inv3(A).a, 9);
}

int main() {
    chol_cases<3>("3");
    chol_cases<6>("6");
    chol_cases<7>("7");

    // the eigenvalue sets of tests/test_knife_edge_gpu.py::test_lm_solve_against_toon_either_side_of_the_svd_cutoff
    int k = 0;
    char name[64];
    for (double c : {1e1, 1e3, 1e5}) {
        const double eig[6] = {3e11 * 1, 3e11 * 0.5, 3e11 * 0.1, 3e11 * 0.03, 3e11 * (3.0 / c), 3e11 * (1.0 / c)};
        std::snprintf(name, sizeof name, "svd6_tracker_%d", k);
        svd6_case(name, eig, k++);
    }
    for (double ratio : {0.5e9, 0.999e9, 1.001e9, 2e9, 1e12}) {
        const double one[6] = {1.0, 0.4, 0.2, 0.1, 0.05, 1.0 / ratio};
        const double two[6] = {7e10, 3e10, 2e9, 1e9, 7e10 / ratio, 0.3 * 7e10 / ratio};
        std::snprintf(name, sizeof name, "svd6_cutoff_one_%d", k);
        svd6_case(name, one, k++);
        std::snprintf(name, sizeof name, "svd6_cutoff_two_%d", k);
        svd6_case(name, two, k++);
    }
    const double rank5[6] = {1.0, 0.5, 0.2, 0.1, 0.05, 0.0}, rank3[6] = {1.0, 0.5, 0.2, 0.0, 0.0, 0.0};
    svd6_case("svd6_rank5", rank5, k++);
    svd6_case("svd6_rank3", rank3, k++);

    {   // SymSVD<7>, cold and from the eigenvectors of a nearby matrix
        double e0[7], e1[7];
        for (int i = 0; i < 7; i++) { e0[i] = 1e4 / (1 + 37.0 * i * i); e1[i] = e0[i] * (1 + 1e-3 * (i - 3)); }
        const Mat<7, 7> A0 = sym_from_eig<7>(e0, 2), A1 = A0 + sym_from_eig<7>(e1, 5) * 1e-3;
        const Vec<7> b = rhs<7>(0.25 * max_abs(A1));
        const SymSVD<7> prev(A0), cold(A1), warm(A1, 1e9, &prev.V);
        put("svd7_cold", "e", cold.e, 7);
        put("svd7_cold", "backsub", cold.backsub(b).v, 7);
        put("svd7_cold", "pinv", cold.pinv().a, 49);
        put("svd7_warm", "e", warm.e, 7);
        put("svd7_warm", "backsub", warm.backsub(b).v, 7);
        put("svd7_warm", "pinv", warm.pinv().a, 49);
    }

    exp_case("exp_zero", 0, 0, 0);
    exp_case("exp_z_only", 0, 0, 0.3);
    {   // theta_sq = 9 s^2 either side of the two series thresholds
        const double s8 = std::sqrt(1e-8 / 9), s6 = std::sqrt(1e-6 / 9);
        exp_case("exp_below_1e-8", s8 * (1 - 1e-3), 2 * s8 * (1 - 1e-3), -2 * s8 * (1 - 1e-3));
        exp_case("exp_above_1e-8", s8 * (1 + 1e-3), 2 * s8 * (1 + 1e-3), -2 * s8 * (1 + 1e-3));
        exp_case("exp_below_1e-6", s6 * (1 - 1e-3), 2 * s6 * (1 - 1e-3), -2 * s6 * (1 - 1e-3));
        exp_case("exp_above_1e-6", s6 * (1 + 1e-3), 2 * s6 * (1 + 1e-3), -2 * s6 * (1 + 1e-3));
    }
    exp_case("exp_large", 1.5, -2.0, 1.0);
    exp_case("exp_beyond_pi", 3.0, 2.0, -1.0);

    ln_case("ln_identity", Mat<3, 3>::identity());
    ln_of_exp("ln_near_small", 0.01, 1, -2, 2);
    ln_of_exp("ln_near_below_45deg", M_PI / 4 * (1 - 1e-3), 1, 2, 2);
    ln_of_exp("ln_mid_above_45deg", M_PI / 4 * (1 + 1e-3), 1, 2, 2);
    ln_of_exp("ln_mid_below_135deg", 3 * M_PI / 4 * (1 - 1e-3), 1, 2, 2);
    // the far branch (angle above 135 degrees): these rows are the header's own (TooN's unit(r2) * angle), see DESIGN.md
    ln_of_exp("ln_far_above_135deg", 3 * M_PI / 4 * (1 + 1e-3), 1, 2, 2);
    ln_of_exp("ln_far_x_dominant", M_PI - 1e-3, 3, 1, 1);
    ln_of_exp("ln_far_y_dominant", M_PI - 1e-3, 1, 3, 1);
    ln_of_exp("ln_far_z_dominant", M_PI - 1e-3, 1, 1, 3);
    ln_of_exp("ln_far_sign_flip", M_PI - 1e-3, -3, 1, 1);

    inv3_case("inv3_both_swaps", Mat<3, 3>{{1, 2, 3, 4, 5, 6, 7, 8, 10}});
    inv3_case("inv3_singular", Mat<3, 3>{{1, 2, 3, 4, 5, 6, 7, 8, 9}});
    inv3_case("inv3_plane_fit_win1", phi_t_phi(1));
    inv3_case("inv3_plane_fit_win2", phi_t_phi(2));
    inv3_case("inv3_plane_fit_win3", phi_t_phi(3));
    return 0;
}
