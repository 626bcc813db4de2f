// CPU restatement of pmv_find_homography (include/pmv_hip.h): cv::findHomography(points1, points2, cv::RANSAC, threshold, mask, maxIters,
// confidence), written from memory of OpenCV 3.4 (fundam.cpp: HomographyEstimatorCallback, HomographyRefineCallback, findHomography;
// ptsetreg.cpp: RANSACPointSetRegistrator; lmsolver.cpp: LMSolverImpl; lapack.cpp: JacobiImpl_). [mem: OpenCV 3.4 fundam.cpp, ptsetreg.cpp,
// lmsolver.cpp; parity with a real OpenCV unpinned]
// It is what fixes the bits of k_homography_ransac (csrc/backend_homography.hip): every floating-point statement below is IEEE + - * / sqrt
// in this order (-ffp-contract=off, no fast-math on both sides). Three things are this file's own choices, because cv's bits cannot be had
// on a device:
//   1. the null space of the 8x9 system of a four-point sample: Gauss-Jordan with complete pivoting, the vector normalised to unit length
//      (cv: the least eigenvector of LtL from eigen()). The refit on the inliers does take the least eigenvector of the 9x9 LtL, by the
//      restatement of JacobiImpl_ below.
//   2. hypot inside the Jacobi rotations: hg_hypot below (|a| > |b|: |a| sqrt(1 + (b/a)^2), ...), not libm's.
//   3. the order of every sum over the inliers (the centroids and deviations, LtL, JtJ, Jtr, S, Sd of the refit): point i goes to partial sum
//      i mod 64, each partial sum takes its points in increasing i starting from 0.0, and the 64 partial sums are then added by the xor
//      butterfly 32, 16, 8, 4, 2, 1 (part[l] = part[l] + part[l ^ o] for every l at once; the result is part[0]). Points that are not inliers
//      are skipped; cv compresses the inliers and sums them one after the other. The sums of a four-point sample are cv's: sequential.
// The solver's arrays are reached through W(k), so that the kernel's text is this text with another W.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr int MAX_ATTEMPTS = 10000;   // RANSACPointSetRegistrator::run calls getSubset(.., rng, 10000)

struct RNG {   // cv::RNG: multiply-with-carry
    uint64_t state;
    explicit RNG(uint64_t s) : state(s) {}
    unsigned next() { state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32); return (unsigned)state; }
};

// haveCollinearPoints on the subset's LAST point (cv's quirk): against every pair (j, k < j) of the earlier ones; q: the subset's points (x, y)
bool last_point_collinear(const float* q, int count) {
    const int i = count - 1;
    const float xi = q[2 * i], yi = q[2 * i + 1];
    for (int j = 0; j < i; j++) {
        const double dx1 = q[2 * j] - xi, dy1 = q[2 * j + 1] - yi;   // float subtractions, widened
        for (int k = 0; k < j; k++) {
            const double dx2 = q[2 * k] - xi, dy2 = q[2 * k + 1] - yi;
            if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
        }
    }
    return false;
}

// determinant of the homogeneous points a, b, c of q (floats widened), cv's Matx33d expression
inline double det3(const float* q, int a, int b, int c) {
    const double a0 = q[2 * a], a1 = q[2 * a + 1], b0 = q[2 * b], b1 = q[2 * b + 1], c0 = q[2 * c], c1 = q[2 * c + 1];
    return a0 * (b1 * 1. - c1 * 1.) - a1 * (b0 * 1. - c0 * 1.) + 1. * (b0 * c1 - c0 * b1);
}
// the four-point consistency test: for each of the four triples the orientation in image 1 and in image 2 must agree
bool orientation_consistent(const float* q1, const float* q2) {
    const int tt[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
    for (int t = 0; t < 4; t++)
        if (det3(q1, tt[t][0], tt[t][1], tt[t][2]) * det3(q2, tt[t][0], tt[t][1], tt[t][2]) < 0) return false;
    return true;
}
// HomographyEstimatorCallback::checkSubset on the four points q1, q2: 0 accepted, 1 collinear, 2 orientation
int check_subset(const float* q1, const float* q2) {
    if (last_point_collinear(q1, 4) || last_point_collinear(q2, 4)) return 1;
    return orientation_consistent(q1, q2) ? 0 : 2;
}

// getSubset with modelPoints = 4 + checkSubset; refused[0], refused[1]: the subsets turned down as collinear / by the orientation test
bool get_subset(RNG& rng, const float* p1, const float* p2, int n, int* idx, int* refused) {
    for (int attempt = 0; attempt < MAX_ATTEMPTS; attempt++) {
        for (int i = 0; i < 4;) {
            const int v = (int)(rng.next() % (unsigned)n);
            idx[i] = v;
            int j = 0;
            for (; j < i; j++) if (v == idx[j]) break;
            if (j == i) i++;
        }
        float q1[8], q2[8];
        for (int i = 0; i < 4; i++) { q1[2 * i] = p1[2 * idx[i]]; q1[2 * i + 1] = p1[2 * idx[i] + 1]; q2[2 * i] = p2[2 * idx[i]]; q2[2 * i + 1] = p2[2 * idx[i] + 1]; }
        const int why = check_subset(q1, q2);
        if (why) { if (refused) ++refused[why - 1]; continue; }
        return true;
    }
    return false;
}

// ---- what the sample solver and the refit share: the workspace slots [T1 = invHnorm at 0 | T2 = Hnorm2 at 9 | Htemp at 18 | H at 27 | .. | h0 at 72]
#define W(k) ws[(k)]
#define CP(k) cp[(k)]
// cv's two normalising matrices from the centroids (cM, cm) and the scales (sM, sm = count / sum of absolute deviations) of image 1 and 2
void hg_set_T(double* ws, double cMx, double cMy, double cmx, double cmy, double sMx, double sMy, double smx, double smy) {
    W(0) = 1. / smx; W(1) = 0; W(2) = cmx; W(3) = 0; W(4) = 1. / smy; W(5) = cmy; W(6) = 0; W(7) = 0; W(8) = 1;
    W(9) = sMx; W(10) = 0; W(11) = -cMx * sMx; W(12) = 0; W(13) = sMy; W(14) = -cMy * sMy; W(15) = 0; W(16) = 0; W(17) = 1;
}
// H = invHnorm * H0 * Hnorm2 scaled by 1 / H[8] (H[8] = 1 then); no model where H[8] is 0 or not a number (cv divides unguarded)
int hg_compose(double* ws) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) W(18 + 3 * i + j) = W(3 * i) * W(72 + j) + W(3 * i + 1) * W(75 + j) + W(3 * i + 2) * W(78 + j);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) W(27 + 3 * i + j) = W(18 + 3 * i) * W(9 + j) + W(19 + 3 * i) * W(12 + j) + W(20 + 3 * i) * W(15 + j);
    const double h8 = W(35);
    if (!(fabs(h8) > 0)) return 0;
    const double s = 1. / h8;
    for (int k = 0; k < 8; k++) W(27 + k) *= s;
    W(35) = 1.;
    return 1;
}

// runKernel on the subset idx[4] of the float points; workspace ws: A 8x9 at 0 (the slots above once it is eliminated) | h0 at 72 (81 doubles),
// cp: the column permutation (9). Returns the number of models (0 or 1); H at W(27)
constexpr int TW_WS = 81;
int four_point(const float* p1, const float* p2, const int* idx, double* ws, unsigned char* cp) {
    float Mx[4], My[4], mx[4], my[4];
    for (int i = 0; i < 4; i++) { Mx[i] = p1[2 * idx[i]]; My[i] = p1[2 * idx[i] + 1]; mx[i] = p2[2 * idx[i]]; my[i] = p2[2 * idx[i] + 1]; }
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
    for (int i = 0; i < 4; i++) { cmx += mx[i]; cmy += my[i]; cMx += Mx[i]; cMy += My[i]; }
    cmx /= 4; cmy /= 4; cMx /= 4; cMy /= 4;
    for (int i = 0; i < 4; i++) { smx += fabs(mx[i] - cmx); smy += fabs(my[i] - cmy); sMx += fabs(Mx[i] - cMx); sMy += fabs(My[i] - cMy); }
    if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return 0;
    smx = 4 / smx; smy = 4 / smy; sMx = 4 / sMx; sMy = 4 / sMy;
    for (int i = 0; i < 4; i++) {
        const double x = (mx[i] - cmx) * smx, y = (my[i] - cmy) * smy, X = (Mx[i] - cMx) * sMx, Y = (My[i] - cMy) * sMy;
        W(18 * i + 0) = X; W(18 * i + 1) = Y; W(18 * i + 2) = 1; W(18 * i + 3) = 0; W(18 * i + 4) = 0; W(18 * i + 5) = 0;
        W(18 * i + 6) = -x * X; W(18 * i + 7) = -x * Y; W(18 * i + 8) = -x;
        W(18 * i + 9) = 0; W(18 * i + 10) = 0; W(18 * i + 11) = 0; W(18 * i + 12) = X; W(18 * i + 13) = Y; W(18 * i + 14) = 1;
        W(18 * i + 15) = -y * X; W(18 * i + 16) = -y * Y; W(18 * i + 17) = -y;
    }
    // null space: Gauss-Jordan with complete pivoting (fundamental_twin.cpp's construction for its 7x9 system), then one unit vector
    for (int c = 0; c < 9; c++) CP(c) = (unsigned char)c;
    for (int r = 0; r < 8; r++) {
        int pr = r, pc = r;
        double best = -1;
        for (int i = r; i < 8; i++)
            for (int j = r; j < 9; j++) { const double v = fabs(W(i * 9 + j)); if (v > best) { best = v; pr = i; pc = j; } }
        if (!(best > 1e-300)) return 0;
        if (pr != r) for (int j = 0; j < 9; j++) { const double t = W(r * 9 + j); W(r * 9 + j) = W(pr * 9 + j); W(pr * 9 + j) = t; }
        if (pc != r) {
            for (int i = 0; i < 8; i++) { const double t = W(i * 9 + r); W(i * 9 + r) = W(i * 9 + pc); W(i * 9 + pc) = t; }
            const unsigned char t = CP(r); CP(r) = CP(pc); CP(pc) = t;
        }
        const double inv = 1.0 / W(r * 9 + r);
        for (int j = 0; j < 9; j++) W(r * 9 + j) *= inv;
        for (int i = 0; i < 8; i++) {
            if (i == r) continue;
            const double f = W(i * 9 + r);
            if (f == 0.0) continue;
            for (int j = 0; j < 9; j++) W(i * 9 + j) -= f * W(r * 9 + j);
        }
    }
    double nrm = 1.0;   // the vector's own 1 at column 8
    for (int i = 0; i < 8; i++) nrm += W(i * 9 + 8) * W(i * 9 + 8);
    nrm = sqrt(nrm);
    for (int j = 0; j < 9; j++) {
        const double v = j < 8 ? -W(j * 9 + 8) : 1.0;
        W(72 + CP(j)) = v / nrm;
    }
    hg_set_T(ws, cMx, cMy, cmx, cmy, sMx, sMy, smx, smy);
    return hg_compose(ws);
}
#undef CP

// HomographyEstimatorCallback::computeError of correspondence i: float32 throughout
inline float hg_error(const double* H, const float* p1, const float* p2, int i) {
    const float H0 = (float)H[0], H1 = (float)H[1], H2 = (float)H[2], H3 = (float)H[3], H4 = (float)H[4], H5 = (float)H[5], H6 = (float)H[6], H7 = (float)H[7];
    const float Mx = p1[2 * i], My = p1[2 * i + 1];
    const float ww = 1.f / (H6 * Mx + H7 * My + 1.f);
    const float dx = (H0 * Mx + H1 * My + H2) * ww - p2[2 * i];
    const float dy = (H3 * Mx + H4 * My + H5) * ww - p2[2 * i + 1];
    return dx * dx + dy * dy;
}

// RANSACUpdateNumIters(p, (n - g) / n, model_points, .) split as vo::ransac_iters_table splits it: the logarithms here ...
void iters_table(int n, double p, int model_points, double* out_denoms, double* out_num) {
    p = p < 0. ? 0. : p; p = p > 1. ? 1. : p;
    const double num = 1. - p;
    *out_num = log(num < DBL_MIN ? DBL_MIN : num);
    for (int g = 0; g <= n; g++) {
        double ep = n > 0 ? (double)(n - g) / n : 0.;
        ep = ep < 0. ? 0. : ep; ep = ep > 1. ? 1. : ep;
        const double denom = 1. - pow(1. - ep, model_points);
        out_denoms[g] = denom < DBL_MIN ? -HUGE_VAL : log(denom);
    }
}
// ... and the final expression there
inline int update_iters(const double* tab, int good, int max_iters) {
    const double num = tab[0], denom = tab[1 + good];
    return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

// ---- the refit's serial algebra: plain arrays, so the kernel's text is this text ----
inline double hg_hypot(double a, double b) {
    a = fabs(a); b = fabs(b);
    if (a > b) { b /= a; return a * sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
    return 0;
}

// cv's JacobiImpl_<double> on the symmetric n x n matrix A (row-major, destroyed): eigenvalues Wv in descending order, eigenvectors the ROWS of V.
// ind: 2 n ints. The pivot of a rotation is the largest off-diagonal element of the upper triangle, tracked per row (indR) and column (indC).
void hg_jacobi(double* A, int n, double* Wv, double* V, int* ind) {
    const double eps = DBL_EPSILON;
    int* indR = ind;
    int* indC = ind + n;
    int i, k, m;
    double mv;
    for (i = 0; i < n; i++) { for (k = 0; k < n; k++) V[i * n + k] = 0; V[i * n + i] = 1; }
    for (k = 0; k < n; k++) {
        Wv[k] = A[(n + 1) * k];
        if (k < n - 1) {
            for (m = k + 1, mv = fabs(A[n * k + m]), i = k + 2; i < n; i++) { const double val = fabs(A[n * k + i]); if (mv < val) { mv = val; m = i; } }
            indR[k] = m;
        }
        if (k > 0) {
            for (m = 0, mv = fabs(A[k]), i = 1; i < k; i++) { const double val = fabs(A[n * i + k]); if (mv < val) { mv = val; m = i; } }
            indC[k] = m;
        }
    }
    const int max_iters = n * n * 30;
    if (n > 1) for (int iters = 0; iters < max_iters; iters++) {
        for (k = 0, mv = fabs(A[indR[0]]), i = 1; i < n - 1; i++) { const double val = fabs(A[n * i + indR[i]]); if (mv < val) { mv = val; k = i; } }
        int l = indR[k];
        for (i = 1; i < n; i++) { const double val = fabs(A[n * indC[i] + i]); if (mv < val) { mv = val; k = indC[i]; l = i; } }
        const double p = A[n * k + l];
        if (fabs(p) <= eps) break;
        const double y = (Wv[l] - Wv[k]) * 0.5;
        double t = fabs(y) + hg_hypot(p, y);
        double s = hg_hypot(p, t);
        const double c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) { s = -s; t = -t; }
        A[n * k + l] = 0;
        Wv[k] -= t;
        Wv[l] += t;
        double a0, b0;
#define HG_ROTATE(v0, v1) { a0 = v0; b0 = v1; v0 = a0 * c - b0 * s; v1 = a0 * s + b0 * c; }
        for (i = 0; i < k; i++) HG_ROTATE(A[n * i + k], A[n * i + l])
        for (i = k + 1; i < l; i++) HG_ROTATE(A[n * k + i], A[n * i + l])
        for (i = l + 1; i < n; i++) HG_ROTATE(A[n * k + i], A[n * l + i])
        for (i = 0; i < n; i++) HG_ROTATE(V[n * k + i], V[n * l + i])
#undef HG_ROTATE
        for (int j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                for (m = idx + 1, mv = fabs(A[n * idx + m]), i = idx + 2; i < n; i++) { const double val = fabs(A[n * idx + i]); if (mv < val) { mv = val; m = i; } }
                indR[idx] = m;
            }
            if (idx > 0) {
                for (m = 0, mv = fabs(A[idx]), i = 1; i < idx; i++) { const double val = fabs(A[n * i + idx]); if (mv < val) { mv = val; m = i; } }
                indC[idx] = m;
            }
        }
    }
    for (k = 0; k < n - 1; k++) {
        m = k;
        for (i = k + 1; i < n; i++) if (Wv[m] < Wv[i]) m = i;
        if (k != m) {
            double t = Wv[m]; Wv[m] = Wv[k]; Wv[k] = t;
            for (i = 0; i < n; i++) { t = V[n * m + i]; V[n * m + i] = V[n * k + i]; V[n * k + i] = t; }
        }
    }
}

// the refit's workspace rw (doubles): the slots of hg_compose | reduction results | Jacobi's matrix, vectors, values | LM's A = JtJ, v = Jtr, D,
// step d, x, xd, temp | LM's scalars
constexpr int RF_RED = 81, RF_A = 136, RF_V = 224, RF_W = 312, RF_JTJ = 328, RF_JTR = 392, RF_D = 400, RF_STEP = 408, RF_X = 416, RF_XD = 424, RF_T = 432,
              RF_S = 440, RF_LAMBDA = 441, RF_LC = 442, RF_RINF = 443, RF_SIZE = 448;
constexpr int RED_N = 46;   // reduction results of one pass at most: 45 sums and one maximum

// entry e of the upper triangle of a symmetric n x n matrix, rows first: (j, k >= j)
inline void hg_tri(int e, int n, int* j, int* k) { int r = 0; while (e >= n - r) { e -= n - r; r++; } *j = r; *k = r + e; }

// the 9x9 system of the refit from its 45 sums: the symmetric matrix, its least eigenvector into h0, then hg_compose
int hg_refit_solve(double* rw, int* ind) {
    for (int e = 0; e < 45; e++) { int j, k; hg_tri(e, 9, &j, &k); rw[RF_A + 9 * j + k] = rw[RF_RED + e]; rw[RF_A + 9 * k + j] = rw[RF_RED + e]; }
    hg_jacobi(rw + RF_A, 9, rw + RF_W, rw + RF_V, ind);
    for (int j = 0; j < 9; j++) rw[72 + j] = rw[RF_V + 72 + j];
    return hg_compose(rw);
}

// solve(A, b, x, DECOMP_EIG) on the eigenpairs in RF_W, RF_V of the 8x8 matrix: the terms of eigenvalues within 2 eps sum|w| of zero are left out
void hg_eig_backsub(double* rw, const double* b, double* x) {
    double thr = 0;
    for (int k = 0; k < 8; k++) thr += fabs(rw[RF_W + k]);
    thr *= 2 * DBL_EPSILON;
    for (int i = 0; i < 8; i++) x[i] = 0;
    for (int k = 0; k < 8; k++) {
        const double w = rw[RF_W + k];
        if (!(fabs(w) > thr)) continue;
        double s = 0;
        for (int j = 0; j < 8; j++) s += rw[RF_V + 8 * k + j] * b[j];
        s /= w;
        for (int i = 0; i < 8; i++) x[i] += s * rw[RF_V + 8 * k + i];
    }
}
// LMSolver: what a full pass at x leaves in the reduction results goes into A, v, (S), the residuals' largest magnitude
void hg_lm_load(double* rw) {
    for (int e = 0; e < 36; e++) { int j, k; hg_tri(e, 8, &j, &k); rw[RF_JTJ + 8 * j + k] = rw[RF_RED + e]; rw[RF_JTJ + 8 * k + j] = rw[RF_RED + e]; }
    for (int j = 0; j < 8; j++) rw[RF_JTR + j] = rw[RF_RED + 36 + j];
    rw[RF_RINF] = rw[RF_RED + 45];
}
void hg_lm_begin(double* rw) {
    hg_lm_load(rw);
    rw[RF_S] = rw[RF_RED + 44];
    for (int i = 0; i < 8; i++) rw[RF_D + i] = rw[RF_JTJ + 9 * i];
    rw[RF_LAMBDA] = 1; rw[RF_LC] = 0.75;
}
// Ap = A + lambda diag(D); d = Ap^-1 v; xd = x - d
void hg_lm_step(double* rw, int* ind) {
    for (int i = 0; i < 64; i++) rw[RF_A + i] = rw[RF_JTJ + i];
    for (int i = 0; i < 8; i++) rw[RF_A + 9 * i] += rw[RF_LAMBDA] * rw[RF_D + i];
    hg_jacobi(rw + RF_A, 8, rw + RF_W, rw + RF_V, ind);
    hg_eig_backsub(rw, rw + RF_JTR, rw + RF_STEP);
    for (int i = 0; i < 8; i++) rw[RF_XD + i] = rw[RF_X + i] - rw[RF_STEP + i];
}
// the damping rule on Sd = |r(xd)|^2; true if xd is taken (Sd < S: x and xd swap, S = Sd; the caller makes a full pass at the new x)
bool hg_lm_decide(double* rw, double Sd, int* ind) {
    const double Rlo = 0.25, Rhi = 0.75, S = rw[RF_S];
    double dS = 0;
    for (int i = 0; i < 8; i++) {   // temp_d = 2 v - A d; dS = d . temp_d
        double a = 0;
        for (int j = 0; j < 8; j++) a += rw[RF_JTJ + 8 * i + j] * rw[RF_STEP + j];
        rw[RF_T + i] = 2 * rw[RF_JTR + i] - a;
    }
    for (int i = 0; i < 8; i++) dS += rw[RF_STEP + i] * rw[RF_T + i];
    const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1);
    if (R > Rhi) {
        rw[RF_LAMBDA] *= 0.5;
        if (rw[RF_LAMBDA] < rw[RF_LC]) rw[RF_LAMBDA] = 0;
    } else if (R < Rlo) {
        double t = 0;
        for (int i = 0; i < 8; i++) t += rw[RF_STEP + i] * rw[RF_JTR + i];
        double nu = (Sd - S) / (fabs(t) > DBL_EPSILON ? t : 1) + 2;
        nu = nu > 2. ? nu : 2.; nu = nu < 10. ? nu : 10.;   // min(max(nu, 2), 10)
        if (rw[RF_LAMBDA] == 0) {   // invert(A, DECOMP_EIG): the largest diagonal magnitude of the (pseudo-)inverse
            for (int i = 0; i < 64; i++) rw[RF_A + i] = rw[RF_JTJ + i];
            hg_jacobi(rw + RF_A, 8, rw + RF_W, rw + RF_V, ind);
            double thr = 0;
            for (int k = 0; k < 8; k++) thr += fabs(rw[RF_W + k]);
            thr *= 2 * DBL_EPSILON;
            double maxval = DBL_EPSILON;
            for (int i = 0; i < 8; i++) {
                double a = 0;
                for (int k = 0; k < 8; k++) { const double w = rw[RF_W + k]; if (fabs(w) > thr) a += rw[RF_V + 8 * k + i] * rw[RF_V + 8 * k + i] / w; }
                if (fabs(a) > maxval) maxval = fabs(a);
            }
            rw[RF_LAMBDA] = rw[RF_LC] = 1. / maxval;
            nu *= 0.5;
        }
        rw[RF_LAMBDA] *= nu;
    }
    if (!(Sd < S)) return false;
    rw[RF_S] = Sd;
    for (int i = 0; i < 8; i++) { const double t = rw[RF_X + i]; rw[RF_X + i] = rw[RF_XD + i]; rw[RF_XD + i] = t; }
    return true;
}
// after iteration `iter` (1-based): go on?
bool hg_lm_proceed(const double* rw, int iter) {
    double dinf = 0;
    for (int i = 0; i < 8; i++) { const double a = fabs(rw[RF_STEP + i]); if (a > dinf) dinf = a; }
    return iter < 10 && dinf >= FLT_EPSILON && rw[RF_RINF] >= FLT_EPSILON;
}

// ---- the refit's sums over the inliers (choice 3 of the header) ----
inline double butterfly(double* part) {
    for (int o = 32; o > 0; o >>= 1) {
        double t[64];
        for (int l = 0; l < 64; l++) t[l] = part[l] + part[l ^ o];
        memcpy(part, t, sizeof(t));
    }
    return part[0];
}
template <class Term> double lane_sum(int n, const uint8_t* inl, Term term) {
    double part[64];
    for (int l = 0; l < 64; l++) {
        double acc = 0;
        for (int i = l; i < n; i += 64) if (inl[i]) acc += term(i);
        part[l] = acc;
    }
    return butterfly(part);
}
template <class Term> double lane_max(int n, const uint8_t* inl, Term term) {
    double acc = 0;
    for (int i = 0; i < n; i++) if (inl[i]) acc = fmax(acc, term(i));   // (a maximum has no order)
    return acc;
}

// cv's two rows of correspondence (X, Y) -> (x, y) in normalised coordinates
inline double hg_lx(int j, double X, double Y, double x) {
    switch (j) { case 0: return X; case 1: return Y; case 2: return 1; case 6: return -x * X; case 7: return -x * Y; case 8: return -x; default: return 0; }
}
inline double hg_ly(int j, double X, double Y, double y) {
    switch (j) { case 3: return X; case 4: return Y; case 5: return 1; case 6: return -y * X; case 7: return -y * Y; case 8: return -y; default: return 0; }
}
// HomographyRefineCallback at the parameters h[8] for the correspondence (Mx, My) -> (mx, my): residuals, then the two Jacobian rows
struct LmPoint { double Mx, My, ww, xi, yi, rx, ry; };
inline LmPoint hg_lm_point(const double* h, double Mx, double My, double mx, double my) {
    LmPoint q;
    q.Mx = Mx; q.My = My;
    double ww = h[6] * Mx + h[7] * My + 1.;
    ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
    q.ww = ww;
    q.xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
    q.yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
    q.rx = q.xi - mx; q.ry = q.yi - my;
    return q;
}
inline double hg_jx(int a, const LmPoint& q) {
    switch (a) { case 0: return q.Mx * q.ww; case 1: return q.My * q.ww; case 2: return q.ww; case 6: return -q.Mx * q.ww * q.xi; case 7: return -q.My * q.ww * q.xi; default: return 0; }
}
inline double hg_jy(int a, const LmPoint& q) {
    switch (a) { case 3: return q.Mx * q.ww; case 4: return q.My * q.ww; case 5: return q.ww; case 6: return -q.Mx * q.ww * q.yi; case 7: return -q.My * q.ww * q.yi; default: return 0; }
}
// term e of a pass: 0..35 the upper triangle of JtJ, 36..43 Jtr, 44 |r|^2
inline double hg_lm_term(int e, const LmPoint& q) {
    if (e < 36) { int a, b; hg_tri(e, 8, &a, &b); return hg_jx(a, q) * hg_jx(b, q) + hg_jy(a, q) * hg_jy(b, q); }
    if (e < 44) return hg_jx(e - 36, q) * q.rx + hg_jy(e - 36, q) * q.ry;
    return q.rx * q.rx + q.ry * q.ry;
}

// the reductions of one LM pass at h into rw's results: everything (full) or |r|^2 alone
void lm_pass(double* rw, const double* h, const float* p1, const float* p2, int n, const uint8_t* inl, bool full) {
    for (int e = full ? 0 : 44; e < 45; e++)
        rw[RF_RED + e] = lane_sum(n, inl, [&](int i) { return hg_lm_term(e, hg_lm_point(h, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1])); });
    if (full) rw[RF_RED + 45] = lane_max(n, inl, [&](int i) { const LmPoint q = hg_lm_point(h, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]); return fmax(fabs(q.rx), fabs(q.ry)); });
}

// runKernel on the `count` inliers: H into rw[27..35], 0 where it gives no model
int refit_dlt(double* rw, int* ind, const float* p1, const float* p2, int n, const uint8_t* inl, int count) {
    double cmx = lane_sum(n, inl, [&](int i) { return (double)p2[2 * i]; }), cmy = lane_sum(n, inl, [&](int i) { return (double)p2[2 * i + 1]; });
    double cMx = lane_sum(n, inl, [&](int i) { return (double)p1[2 * i]; }), cMy = lane_sum(n, inl, [&](int i) { return (double)p1[2 * i + 1]; });
    cmx /= count; cmy /= count; cMx /= count; cMy /= count;
    double smx = lane_sum(n, inl, [&](int i) { return fabs(p2[2 * i] - cmx); }), smy = lane_sum(n, inl, [&](int i) { return fabs(p2[2 * i + 1] - cmy); });
    double sMx = lane_sum(n, inl, [&](int i) { return fabs(p1[2 * i] - cMx); }), sMy = lane_sum(n, inl, [&](int i) { return fabs(p1[2 * i + 1] - cMy); });
    if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return 0;
    smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
    for (int e = 0; e < 45; e++) {
        int j, k;
        hg_tri(e, 9, &j, &k);
        rw[RF_RED + e] = lane_sum(n, inl, [&](int i) {
            const double x = (p2[2 * i] - cmx) * smx, y = (p2[2 * i + 1] - cmy) * smy, X = (p1[2 * i] - cMx) * sMx, Y = (p1[2 * i + 1] - cMy) * sMy;
            return hg_lx(j, X, Y, x) * hg_lx(k, X, Y, x) + hg_ly(j, X, Y, y) * hg_ly(k, X, Y, y);
        });
    }
    hg_set_T(rw, cMx, cMy, cmx, cmy, sMx, sMy, smx, smy);
    return hg_refit_solve(rw, ind);
}

// LMSolver(HomographyRefineCallback, max_iter).run on H9's eight free entries (H9[8] is 1); returns the iterations made. S2: |r|^2 before and after
int lm_refine(double* rw, int* ind, const float* p1, const float* p2, int n, const uint8_t* inl, double* H9, int max_iter, double* S2) {
    for (int i = 0; i < 8; i++) rw[RF_X + i] = H9[i];
    lm_pass(rw, rw + RF_X, p1, p2, n, inl, true);
    hg_lm_begin(rw);
    if (S2) S2[0] = rw[RF_S];
    int iter = 0;
    for (;;) {
        hg_lm_step(rw, ind);
        lm_pass(rw, rw + RF_XD, p1, p2, n, inl, false);
        if (hg_lm_decide(rw, rw[RF_RED + 44], ind)) { lm_pass(rw, rw + RF_X, p1, p2, n, inl, true); hg_lm_load(rw); }
        iter++;
        if (!(iter < max_iter && hg_lm_proceed(rw, iter))) break;
    }
    for (int i = 0; i < 8; i++) H9[i] = rw[RF_X + i];
    if (S2) S2[1] = rw[RF_S];
    return iter;
}
#undef W

}  // namespace

extern "C" {

// the first `count` subsets of a call: returns how many were drawn before getSubset failed (count if it never did); out_refused2: the
// subsets checkSubset turned down as collinear / by the orientation test
int hg_twin_subsets(const float* p1, const float* p2, int n, int count, int* out4, int* out_refused2) {
    RNG rng((uint64_t)-1);
    int refused[2] = {0, 0}, k = 0;
    for (; k < count; k++) if (!get_subset(rng, p1, p2, n, out4 + 4 * k, refused)) break;
    if (out_refused2) { out_refused2[0] = refused[0]; out_refused2[1] = refused[1]; }
    return k;
}

int hg_twin_check_subset(const float* p1_4, const float* p2_4) { return check_subset(p1_4, p2_4); }

int hg_twin_four_point(const float* p1_4, const float* p2_4, double* H9) {
    const int idx[4] = {0, 1, 2, 3};
    double ws[TW_WS];
    unsigned char cp[9];
    const int n = four_point(p1_4, p2_4, idx, ws, cp);
    if (n) memcpy(H9, ws + 27, sizeof(double) * 9);
    return n;
}

void hg_twin_errors(const double* H9, const float* p1, const float* p2, int n, float* err) {
    for (int i = 0; i < n; i++) err[i] = hg_error(H9, p1, p2, i);
}

void hg_twin_iters_table(int n, double confidence, double* out_denoms, double* out_num) { iters_table(n, confidence, 4, out_denoms, out_num); }

int hg_twin_update_iters(const double* tab, int good, int max_iters) { return update_iters(tab, good, max_iters); }

// eigenvalues (descending) and eigenvectors (rows of V) of the symmetric n x n matrix A, n <= 9
void hg_twin_jacobi(const double* A, int n, double* Wv, double* V) {
    double a[81];
    int ind[18];
    memcpy(a, A, sizeof(double) * (size_t)(n * n));
    hg_jacobi(a, n, Wv, V, ind);
}

double hg_twin_hypot(double a, double b) { return hg_hypot(a, b); }

// runKernel on the points whose mask byte is set: 1 and H9, or 0 (H9 untouched)
int hg_twin_refit_dlt(const float* p1, const float* p2, int n, const uint8_t* mask, double* H9) {
    double rw[RF_SIZE];
    int ind[18], count = 0;
    for (int i = 0; i < n; i++) count += mask[i] != 0;
    if (!refit_dlt(rw, ind, p1, p2, n, mask, count)) return 0;
    memcpy(H9, rw + 27, sizeof(double) * 9);
    return 1;
}

// up to max_iter (cv: 10) LM iterations on H9 (H9[8] == 1) over the points whose mask byte is set; returns the iterations made
int hg_twin_lm(const float* p1, const float* p2, int n, const uint8_t* mask, double* H9, int max_iter, double* out_S2) {
    double rw[RF_SIZE];
    int ind[18];
    return lm_refine(rw, ind, p1, p2, n, mask, H9, max_iter, out_S2);
}

// the whole call for n >= 4: returns found; H9 untouched and the mask all 0 when not. *out_updates: how often a model became the best;
// H9_ransac (optional): the model in front of the refit; out_S2 (optional): the LM stage's |r|^2 before and after (untouched without a refit)
int hg_twin_find(const float* p1, const float* p2, int n, double threshold, double confidence, int max_iters, double* H9, uint8_t* mask, int* out_drawn,
                 int* out_updates, double* H9_ransac, double* out_S2) {
    const float thr = (float)(threshold * threshold);
    double best[9] = {0};
    int max_good = 0, iter = 0, updates = 0;
    if (n == 4) {   // cv's count == modelPoints branch: one runKernel, every point an inlier
        const int idx[4] = {0, 1, 2, 3};
        double ws[TW_WS];
        unsigned char cp[9];
        if (four_point(p1, p2, idx, ws, cp)) { memcpy(best, ws + 27, sizeof(best)); max_good = n; }
    } else {
        std::vector<double> tab((size_t)n + 2);
        iters_table(n, confidence, 4, tab.data() + 1, tab.data());
        RNG rng((uint64_t)-1);
        int niters = max_iters;
        for (; iter < niters; iter++) {
            int idx[4];
            if (!get_subset(rng, p1, p2, n, idx, nullptr)) break;   // (at iter 0: no model, nothing drawn)
            double ws[TW_WS];
            unsigned char cp[9];
            if (!four_point(p1, p2, idx, ws, cp)) continue;
            const double* H = ws + 27;
            int good = 0;
            for (int i = 0; i < n; i++) good += hg_error(H, p1, p2, i) <= thr;
            if (good > (max_good > 3 ? max_good : 3)) {
                memcpy(best, H, sizeof(best));
                max_good = good;
                niters = update_iters(tab.data(), good, niters);
                updates++;
            }
        }
    }
    *out_drawn = iter;
    if (out_updates) *out_updates = updates;
    if (max_good <= 0) { memset(mask, 0, (size_t)n); return 0; }
    if (H9_ransac) memcpy(H9_ransac, best, sizeof(best));
    if (n == 4) memset(mask, 1, (size_t)n);
    else {
        for (int i = 0; i < n; i++) mask[i] = (uint8_t)(hg_error(best, p1, p2, i) <= thr);
        // the refit: runKernel on the inliers (H stays the RANSAC model where it gives none), then LMSolver with 10 iterations at most
        double rw[RF_SIZE];
        int ind[18];
        if (refit_dlt(rw, ind, p1, p2, n, mask, max_good)) memcpy(best, rw + 27, sizeof(best));
        lm_refine(rw, ind, p1, p2, n, mask, best, 10, out_S2);
    }
    memcpy(H9, best, sizeof(best));
    return 1;
}

}  // extern "C"
