// gfx950 homography RANSAC: cv::findHomography(p1, p2, cv::RANSAC, threshold, mask, maxIters, confidence) for n >= 4 correspondences
// (pmv_find_homography, include/pmv_hip.h).
// k_homography_ransac: the adaptive RANSAC of one call AND findHomography's refit on the inliers in ONE workgroup. The loop is
// pmv_ransac.h's whole_ransac with what HomographyEstimatorCallback holds: checkSubset (the collinearity test on the subset's last point and
// the four-point orientation test, up to 10000 attempts per subset), the four-point solver and the float32 reprojection error. As in
// k_fundamental_ransac ONE LANE solves one hypothesis on workspaces interleaved in LDS (element k of hypothesis h at k * R + h: the lanes of
// a wave read consecutive doubles), a round holds HG_R = 64 of them and no loop of the solver is unrolled over a dynamically indexed array.
// The refit (HomogModel::finish, behind the loop and the mask, in front of the result block): runKernel on the inliers - the normalisation,
// the 9x9 LtL and its least eigenvector by cv's Jacobi - and up to 10 LMSolver iterations on the 8 free entries. Its sums over the inliers
// are made by all waves: a wave takes every HG_WAVES-th sum, lane l adds the inliers i = l, l + 64, .. in that order and the 64 partial sums
// meet in the xor butterfly 32 .. 1 - the order tests/twin/homography_twin.cpp states. What lies between the sums - the Jacobi sweeps at
// size 9 and 8, LM's damping rule - is serial FP64 work on matrices that stay in LDS: thread 0 runs it. A rotation's t, s, c are a dependent
// chain that one lane does as fast as sixty-four; its 2 n element updates and the pivot searches around it are not, and measured
//  the refit costs ~2 ms per call this way - spreading those over a wavefront is open work that would not change a bit.
// Every statement of the solver and of the refit is the twin's, in its order: IEEE + - * / sqrt only (-ffp-contract=off, no fast-math), so
// found, H, the mask and the sample count are the twin's bits.
#include "pmv_ctx.h"
#include "backend.h"
#include "pmv_prof.h"
#include "pmv_ransac.h"
#include <float.h>

namespace pmv {

namespace {

constexpr int HG_WS = 81;            // doubles per hypothesis: A 8x9 at 0 (T1 at 0 | T2 at 9 | Htemp at 18 | H at 27 once it is eliminated) | h0 at 72
constexpr int HG_THREADS = 512;      // 8 waves score and reduce; the lanes of wave 0 solve
constexpr int HG_WAVES = HG_THREADS / 64;
// the refit's workspace (plain doubles at the start of the solver workspaces, which are free by then): the slots of hg_compose | reduction
// results | Jacobi's matrix, vectors, values | LM's A = JtJ, v = Jtr, D, step d, x, xd, temp | LM's scalars | the normalisation
constexpr int RF_RED = 81, RF_A = 136, RF_V = 224, RF_W = 312, RF_JTJ = 328, RF_JTR = 392, RF_D = 400, RF_STEP = 408, RF_X = 416, RF_XD = 424, RF_T = 432,
              RF_S = 440, RF_LAMBDA = 441, RF_LC = 442, RF_RINF = 443, RF_STAT = 448, RF_SIZE = 456;
static_assert(RF_SIZE <= HG_R * HG_WS, "the refit's workspace lies inside the solver workspaces");

// determinant of the homogeneous points a, b, c of q (floats widened), cv's Matx33d expression
__device__ inline double hg_det3(const float* q, int a, int b, int c) {
    const double a0 = q[2 * a], a1 = q[2 * a + 1], b0 = q[2 * b], b1 = q[2 * b + 1], c0 = q[2 * c], c1 = q[2 * c + 1];
    return a0 * (b1 * 1. - c1 * 1.) - a1 * (b0 * 1. - c0 * 1.) + 1. * (b0 * c1 - c0 * b1);
}
// the four-point consistency test: for each of the four triples the orientation in image 1 and in image 2 must agree
__device__ inline bool hg_orientation_consistent(const float* q1, const float* q2) {
    if (hg_det3(q1, 0, 1, 2) * hg_det3(q2, 0, 1, 2) < 0) return false;
    if (hg_det3(q1, 0, 1, 3) * hg_det3(q2, 0, 1, 3) < 0) return false;
    if (hg_det3(q1, 0, 2, 3) * hg_det3(q2, 0, 2, 3) < 0) return false;
    if (hg_det3(q1, 1, 2, 3) * hg_det3(q2, 1, 2, 3) < 0) return false;
    return true;
}

// the workspace of hypothesis h is W(k) = ws[k * R + h]; the refit's is the same text with R = 1, h = 0
#define W(k) ws[(k) * R + h]
#define CP(k) cp[(k) * R + h]
__device__ inline void hg_set_T(double* ws, int R, int h, double cMx, double cMy, double cmx, double cmy, double sMx, double sMy, double smx, double smy) {
    W(0) = 1. / smx; W(1) = 0; W(2) = cmx; W(3) = 0; W(4) = 1. / smy; W(5) = cmy; W(6) = 0; W(7) = 0; W(8) = 1;
    W(9) = sMx; W(10) = 0; W(11) = -cMx * sMx; W(12) = 0; W(13) = sMy; W(14) = -cMy * sMy; W(15) = 0; W(16) = 0; W(17) = 1;
}
// H = invHnorm * H0 * Hnorm2 scaled by 1 / H[8]; no model where H[8] is 0 or not a number (homography_twin.cpp:hg_compose)
__device__ int hg_compose(double* ws, int R, int h) {
    #pragma unroll 1
    for (int i = 0; i < 3; i++)
        #pragma unroll 1
        for (int j = 0; j < 3; j++) W(18 + 3 * i + j) = W(3 * i) * W(72 + j) + W(3 * i + 1) * W(75 + j) + W(3 * i + 2) * W(78 + j);
    #pragma unroll 1
    for (int i = 0; i < 3; i++)
        #pragma unroll 1
        for (int j = 0; j < 3; j++) W(27 + 3 * i + j) = W(18 + 3 * i) * W(9 + j) + W(19 + 3 * i) * W(12 + j) + W(20 + 3 * i) * W(15 + j);
    const double h8 = W(35);
    if (!(fabs(h8) > 0)) return 0;
    const double s = 1. / h8;
    #pragma unroll 1
    for (int k = 0; k < 8; k++) W(27 + k) *= s;
    W(35) = 1.;
    return 1;
}

// runKernel on the subset idx[0..3] (homography_twin.cpp:four_point)
__device__ int hg_four_point(const float* __restrict__ p1, const float* __restrict__ p2, const int* idx, double* ws, unsigned char* cp, int R, int h) {
    float Mx[4], My[4], mx[4], my[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float2 a = ((const float2*)p1)[idx[i]], c = ((const float2*)p2)[idx[i]];
        Mx[i] = a.x; My[i] = a.y; mx[i] = c.x; my[i] = c.y;
    }
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { cmx += mx[i]; cmy += my[i]; cMx += Mx[i]; cMy += My[i]; }
    cmx /= 4; cmy /= 4; cMx /= 4; cMy /= 4;
#pragma unroll
    for (int i = 0; i < 4; i++) { smx += fabs(mx[i] - cmx); smy += fabs(my[i] - cmy); sMx += fabs(Mx[i] - cMx); sMy += fabs(My[i] - cMy); }
    if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return 0;
    smx = 4 / smx; smy = 4 / smy; sMx = 4 / sMx; sMy = 4 / sMy;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double x = (mx[i] - cmx) * smx, y = (my[i] - cmy) * smy, X = (Mx[i] - cMx) * sMx, Y = (My[i] - cMy) * sMy;
        W(18 * i + 0) = X; W(18 * i + 1) = Y; W(18 * i + 2) = 1; W(18 * i + 3) = 0; W(18 * i + 4) = 0; W(18 * i + 5) = 0;
        W(18 * i + 6) = -x * X; W(18 * i + 7) = -x * Y; W(18 * i + 8) = -x;
        W(18 * i + 9) = 0; W(18 * i + 10) = 0; W(18 * i + 11) = 0; W(18 * i + 12) = X; W(18 * i + 13) = Y; W(18 * i + 14) = 1;
        W(18 * i + 15) = -y * X; W(18 * i + 16) = -y * Y; W(18 * i + 17) = -y;
    }
    #pragma unroll 1
    for (int c = 0; c < 9; c++) CP(c) = (unsigned char)c;
    #pragma unroll 1
    for (int r = 0; r < 8; r++) {
        int pr = r, pc = r;
        double best = -1;
        #pragma unroll 1
        for (int i = r; i < 8; i++)
            #pragma unroll 1
            for (int j = r; j < 9; j++) { const double v = fabs(W(i * 9 + j)); if (v > best) { best = v; pr = i; pc = j; } }
        if (!(best > 1e-300)) return 0;
        if (pr != r) {
            #pragma unroll 1
            for (int j = 0; j < 9; j++) { const double t = W(r * 9 + j); W(r * 9 + j) = W(pr * 9 + j); W(pr * 9 + j) = t; }
        }
        if (pc != r) {
            #pragma unroll 1
            for (int i = 0; i < 8; i++) { const double t = W(i * 9 + r); W(i * 9 + r) = W(i * 9 + pc); W(i * 9 + pc) = t; }
            const unsigned char t = CP(r); CP(r) = CP(pc); CP(pc) = t;
        }
        const double inv = 1.0 / W(r * 9 + r);
        #pragma unroll 1
        for (int j = 0; j < 9; j++) W(r * 9 + j) *= inv;
        #pragma unroll 1
        for (int i = 0; i < 8; i++) {
            if (i == r) continue;
            const double f = W(i * 9 + r);
            if (f == 0.0) continue;
            #pragma unroll 1
            for (int j = 0; j < 9; j++) W(i * 9 + j) -= f * W(r * 9 + j);
        }
    }
    double nrm = 1.0;
    #pragma unroll 1
    for (int i = 0; i < 8; i++) nrm += W(i * 9 + 8) * W(i * 9 + 8);
    nrm = sqrt(nrm);
    #pragma unroll 1
    for (int j = 0; j < 9; j++) {
        const double v = j < 8 ? -W(j * 9 + 8) : 1.0;
        W(72 + CP(j)) = v / nrm;
    }
    hg_set_T(ws, R, h, cMx, cMy, cmx, cmy, sMx, sMy, smx, smy);
    return hg_compose(ws, R, h);
}
#undef W
#undef CP

// HomographyEstimatorCallback::computeError of correspondence i: float32 throughout (homography_twin.cpp:hg_error)
__device__ inline float hg_error(const double* H, const float* __restrict__ p1, const float* __restrict__ p2, int i) {
    const float H0 = (float)H[0], H1 = (float)H[1], H2 = (float)H[2], H3 = (float)H[3], H4 = (float)H[4], H5 = (float)H[5], H6 = (float)H[6], H7 = (float)H[7];
    const float2 M = ((const float2*)p1)[i], m = ((const float2*)p2)[i];
    const float ww = 1.f / (H6 * M.x + H7 * M.y + 1.f);
    const float dx = (H0 * M.x + H1 * M.y + H2) * ww - m.x;
    const float dy = (H3 * M.x + H4 * M.y + H5) * ww - m.y;
    return dx * dx + dy * dy;
}

// ---- the refit's serial algebra (thread 0): homography_twin.cpp's text on plain arrays in LDS ----
__device__ inline double hg_hypot(double a, double b) {
    a = fabs(a); b = fabs(b);
    if (a > b) { b /= a; return a * sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrt(1 + a * a); }
    return 0;
}

// cv's JacobiImpl_<double> on the symmetric n x n matrix A (destroyed): eigenvalues Wv in descending order, eigenvectors the ROWS of V; ind: 2 n ints
__device__ void hg_jacobi(double* A, int n, double* Wv, double* V, int* ind) {
    const double eps = DBL_EPSILON;
    int* indR = ind;
    int* indC = ind + n;
    int i, k, m;
    double mv;
    #pragma unroll 1
    for (i = 0; i < n; i++) {
        #pragma unroll 1
        for (k = 0; k < n; k++) V[i * n + k] = 0;
        V[i * n + i] = 1;
    }
    #pragma unroll 1
    for (k = 0; k < n; k++) {
        Wv[k] = A[(n + 1) * k];
        if (k < n - 1) {
            #pragma unroll 1
            for (m = k + 1, mv = fabs(A[n * k + m]), i = k + 2; i < n; i++) { const double val = fabs(A[n * k + i]); if (mv < val) { mv = val; m = i; } }
            indR[k] = m;
        }
        if (k > 0) {
            #pragma unroll 1
            for (m = 0, mv = fabs(A[k]), i = 1; i < k; i++) { const double val = fabs(A[n * i + k]); if (mv < val) { mv = val; m = i; } }
            indC[k] = m;
        }
    }
    const int max_iters = n * n * 30;
    if (n > 1) {
        #pragma unroll 1
        for (int iters = 0; iters < max_iters; iters++) {
            #pragma unroll 1
            for (k = 0, mv = fabs(A[indR[0]]), i = 1; i < n - 1; i++) { const double val = fabs(A[n * i + indR[i]]); if (mv < val) { mv = val; k = i; } }
            int l = indR[k];
            #pragma unroll 1
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
            #pragma unroll 1
            for (i = 0; i < k; i++) HG_ROTATE(A[n * i + k], A[n * i + l])
            #pragma unroll 1
            for (i = k + 1; i < l; i++) HG_ROTATE(A[n * k + i], A[n * i + l])
            #pragma unroll 1
            for (i = l + 1; i < n; i++) HG_ROTATE(A[n * k + i], A[n * l + i])
            #pragma unroll 1
            for (i = 0; i < n; i++) HG_ROTATE(V[n * k + i], V[n * l + i])
#undef HG_ROTATE
            #pragma unroll 1
            for (int j = 0; j < 2; j++) {
                const int idx = j == 0 ? k : l;
                if (idx < n - 1) {
                    #pragma unroll 1
                    for (m = idx + 1, mv = fabs(A[n * idx + m]), i = idx + 2; i < n; i++) { const double val = fabs(A[n * idx + i]); if (mv < val) { mv = val; m = i; } }
                    indR[idx] = m;
                }
                if (idx > 0) {
                    #pragma unroll 1
                    for (m = 0, mv = fabs(A[idx]), i = 1; i < idx; i++) { const double val = fabs(A[n * i + idx]); if (mv < val) { mv = val; m = i; } }
                    indC[idx] = m;
                }
            }
        }
    }
    #pragma unroll 1
    for (k = 0; k < n - 1; k++) {
        m = k;
        #pragma unroll 1
        for (i = k + 1; i < n; i++) if (Wv[m] < Wv[i]) m = i;
        if (k != m) {
            double t = Wv[m]; Wv[m] = Wv[k]; Wv[k] = t;
            #pragma unroll 1
            for (i = 0; i < n; i++) { t = V[n * m + i]; V[n * m + i] = V[n * k + i]; V[n * k + i] = t; }
        }
    }
}

// entry e of the upper triangle of a symmetric n x n matrix, rows first: (j, k >= j)
__device__ inline void hg_tri(int e, int n, int* j, int* k) { int r = 0; while (e >= n - r) { e -= n - r; r++; } *j = r; *k = r + e; }

__device__ int hg_refit_solve(double* rw, int* ind) {
    #pragma unroll 1
    for (int e = 0; e < 45; e++) { int j, k; hg_tri(e, 9, &j, &k); rw[RF_A + 9 * j + k] = rw[RF_RED + e]; rw[RF_A + 9 * k + j] = rw[RF_RED + e]; }
    hg_jacobi(rw + RF_A, 9, rw + RF_W, rw + RF_V, ind);
    #pragma unroll 1
    for (int j = 0; j < 9; j++) rw[72 + j] = rw[RF_V + 72 + j];
    return hg_compose(rw, 1, 0);
}

__device__ void hg_eig_backsub(double* rw, const double* b, double* x) {
    double thr = 0;
    #pragma unroll 1
    for (int k = 0; k < 8; k++) thr += fabs(rw[RF_W + k]);
    thr *= 2 * DBL_EPSILON;
    #pragma unroll 1
    for (int i = 0; i < 8; i++) x[i] = 0;
    #pragma unroll 1
    for (int k = 0; k < 8; k++) {
        const double w = rw[RF_W + k];
        if (!(fabs(w) > thr)) continue;
        double s = 0;
        #pragma unroll 1
        for (int j = 0; j < 8; j++) s += rw[RF_V + 8 * k + j] * b[j];
        s /= w;
        #pragma unroll 1
        for (int i = 0; i < 8; i++) x[i] += s * rw[RF_V + 8 * k + i];
    }
}
__device__ void hg_lm_load(double* rw) {
    #pragma unroll 1
    for (int e = 0; e < 36; e++) { int j, k; hg_tri(e, 8, &j, &k); rw[RF_JTJ + 8 * j + k] = rw[RF_RED + e]; rw[RF_JTJ + 8 * k + j] = rw[RF_RED + e]; }
    #pragma unroll 1
    for (int j = 0; j < 8; j++) rw[RF_JTR + j] = rw[RF_RED + 36 + j];
    rw[RF_RINF] = rw[RF_RED + 45];
}
__device__ void hg_lm_begin(double* rw) {
    hg_lm_load(rw);
    rw[RF_S] = rw[RF_RED + 44];
    #pragma unroll 1
    for (int i = 0; i < 8; i++) rw[RF_D + i] = rw[RF_JTJ + 9 * i];
    rw[RF_LAMBDA] = 1; rw[RF_LC] = 0.75;
}
__device__ void hg_lm_step(double* rw, int* ind) {
    #pragma unroll 1
    for (int i = 0; i < 64; i++) rw[RF_A + i] = rw[RF_JTJ + i];
    #pragma unroll 1
    for (int i = 0; i < 8; i++) rw[RF_A + 9 * i] += rw[RF_LAMBDA] * rw[RF_D + i];
    hg_jacobi(rw + RF_A, 8, rw + RF_W, rw + RF_V, ind);
    hg_eig_backsub(rw, rw + RF_JTR, rw + RF_STEP);
    #pragma unroll 1
    for (int i = 0; i < 8; i++) rw[RF_XD + i] = rw[RF_X + i] - rw[RF_STEP + i];
}
__device__ bool hg_lm_decide(double* rw, double Sd, int* ind) {
    const double Rlo = 0.25, Rhi = 0.75, S = rw[RF_S];
    double dS = 0;
    #pragma unroll 1
    for (int i = 0; i < 8; i++) {
        double a = 0;
        #pragma unroll 1
        for (int j = 0; j < 8; j++) a += rw[RF_JTJ + 8 * i + j] * rw[RF_STEP + j];
        rw[RF_T + i] = 2 * rw[RF_JTR + i] - a;
    }
    #pragma unroll 1
    for (int i = 0; i < 8; i++) dS += rw[RF_STEP + i] * rw[RF_T + i];
    const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1);
    if (R > Rhi) {
        rw[RF_LAMBDA] *= 0.5;
        if (rw[RF_LAMBDA] < rw[RF_LC]) rw[RF_LAMBDA] = 0;
    } else if (R < Rlo) {
        double t = 0;
        #pragma unroll 1
        for (int i = 0; i < 8; i++) t += rw[RF_STEP + i] * rw[RF_JTR + i];
        double nu = (Sd - S) / (fabs(t) > DBL_EPSILON ? t : 1) + 2;
        nu = nu > 2. ? nu : 2.; nu = nu < 10. ? nu : 10.;
        if (rw[RF_LAMBDA] == 0) {
            #pragma unroll 1
            for (int i = 0; i < 64; i++) rw[RF_A + i] = rw[RF_JTJ + i];
            hg_jacobi(rw + RF_A, 8, rw + RF_W, rw + RF_V, ind);
            double thr = 0;
            #pragma unroll 1
            for (int k = 0; k < 8; k++) thr += fabs(rw[RF_W + k]);
            thr *= 2 * DBL_EPSILON;
            double maxval = DBL_EPSILON;
            #pragma unroll 1
            for (int i = 0; i < 8; i++) {
                double a = 0;
                #pragma unroll 1
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
    #pragma unroll 1
    for (int i = 0; i < 8; i++) { const double t = rw[RF_X + i]; rw[RF_X + i] = rw[RF_XD + i]; rw[RF_XD + i] = t; }
    return true;
}
__device__ bool hg_lm_proceed(const double* rw, int iter) {
    double dinf = 0;
    #pragma unroll 1
    for (int i = 0; i < 8; i++) { const double a = fabs(rw[RF_STEP + i]); if (a > dinf) dinf = a; }
    return iter < 10 && dinf >= FLT_EPSILON && rw[RF_RINF] >= FLT_EPSILON;
}

// ---- the refit's terms, one per correspondence and sum (homography_twin.cpp) ----
__device__ inline double hg_lx(int j, double X, double Y, double x) {
    switch (j) { case 0: return X; case 1: return Y; case 2: return 1; case 6: return -x * X; case 7: return -x * Y; case 8: return -x; default: return 0; }
}
__device__ inline double hg_ly(int j, double X, double Y, double y) {
    switch (j) { case 3: return X; case 4: return Y; case 5: return 1; case 6: return -y * X; case 7: return -y * Y; case 8: return -y; default: return 0; }
}
struct LmPoint { double Mx, My, ww, xi, yi, rx, ry; };
struct LmParams { double h0, h1, h2, h3, h4, h5, h6, h7; };
__device__ inline LmPoint hg_lm_point(const LmParams& h, double Mx, double My, double mx, double my) {
    LmPoint q;
    q.Mx = Mx; q.My = My;
    double ww = h.h6 * Mx + h.h7 * My + 1.;
    ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
    q.ww = ww;
    q.xi = (h.h0 * Mx + h.h1 * My + h.h2) * ww;
    q.yi = (h.h3 * Mx + h.h4 * My + h.h5) * ww;
    q.rx = q.xi - mx; q.ry = q.yi - my;
    return q;
}
__device__ inline double hg_jx(int a, const LmPoint& q) {
    switch (a) { case 0: return q.Mx * q.ww; case 1: return q.My * q.ww; case 2: return q.ww; case 6: return -q.Mx * q.ww * q.xi; case 7: return -q.My * q.ww * q.xi; default: return 0; }
}
__device__ inline double hg_jy(int a, const LmPoint& q) {
    switch (a) { case 3: return q.Mx * q.ww; case 4: return q.My * q.ww; case 5: return q.ww; case 6: return -q.Mx * q.ww * q.yi; case 7: return -q.My * q.ww * q.yi; default: return 0; }
}
__device__ inline double hg_lm_term(int e, const LmPoint& q) {
    if (e < 36) { int a, b; hg_tri(e, 8, &a, &b); return hg_jx(a, q) * hg_jx(b, q) + hg_jy(a, q) * hg_jy(b, q); }
    if (e < 44) return hg_jx(e - 36, q) * q.rx + hg_jy(e - 36, q) * q.ry;
    return q.rx * q.rx + q.ry * q.ry;
}

// HomographyEstimatorCallback as pmv_ransac.h's model: one lane per hypothesis on the interleaved workspaces
struct HomogModel {
    using Problem = HomographyProblem;
    static constexpr int S = 4, MODELS = 1, MAX_R = HG_R, MAX_ATTEMPTS = 10000;
    struct Extra {
        alignas(8) float sp[16];       // the points of the subset thread 0 is testing: image 1, then image 2
        unsigned char cp[HG_R * 9];    // column permutations of the eliminations, interleaved like the workspaces
        int ind[18];                   // Jacobi's pivot indices
        int flag[3];                   // the refit's decisions, from thread 0 to everyone: the normalisation stands, LM takes the step, LM goes on
    };
    using Shared = WholeShared<HomogModel>;
    __device__ static bool direct(int n) { return n == 4; }
    __device__ static bool solve_direct(const Problem& P, double* ws, Shared& sh) {
        #pragma unroll 1
        for (int i = 0; i < 4; i++) sh.idx[i] = i;
        if (!hg_four_point(P.p1, P.p2, sh.idx, ws, sh.x.cp, HG_R, 0)) return false;
        #pragma unroll 1
        for (int k = 0; k < 9; k++) sh.best[k] = model(ws, HG_R, 0, 0, k);
        return true;
    }
    __device__ static bool subset_ok(const Problem& P, const int* idx, Extra& x) {
#pragma unroll
        for (int i = 0; i < 4; i++) {   // all loads in flight together, the tests then run on LDS (FundModel::subset_ok)
            const float2 a = ((const float2*)P.p1)[idx[i]], c = ((const float2*)P.p2)[idx[i]];
            x.sp[2 * i] = a.x; x.sp[2 * i + 1] = a.y; x.sp[8 + 2 * i] = c.x; x.sp[9 + 2 * i] = c.y;
        }
        if (whole_last_point_collinear<4>(x.sp) || whole_last_point_collinear<4>(x.sp + 8)) return false;
        return hg_orientation_consistent(x.sp, x.sp + 8);
    }
    __device__ static void solve(const Problem& P, double* ws, Shared& sh, int R, int nh) {
        const int tid = (int)threadIdx.x;
        if (tid < nh) sh.nm[tid] = hg_four_point(P.p1, P.p2, sh.idx + 4 * tid, ws, sh.x.cp, R, tid);
    }
    __device__ static double model(const double* ws, int R, int b, int, int k) { return ws[(27 + k) * R + b]; }
    __device__ static float error(const double* H, const float* __restrict__ p1, const float* __restrict__ p2, int i) { return hg_error(H, p1, p2, i); }

    // One pass of sums over the inliers of the RANSAC model Hr: sum e of e0 .. e1 - 1 is made by wave e mod HG_WAVES in the twin's order and lands
    // in rw[RF_RED + e]; with `maxima` the last "sum" (e1 - 1) is a maximum. term(e, i): what correspondence i adds to sum e.
    template <class Term> __device__ static void reduce(const Problem& P, const double* Hr, double* rw, int e0, int e1, bool maxima, Term term) {
        const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
        #pragma unroll 1
        for (int e = e0 + wave; e < e1; e += HG_WAVES) {
            const bool mx = maxima && e == e1 - 1;
            double acc = 0;
            #pragma unroll 1
            for (int i = lane; i < P.n; i += 64) {
                if (!(hg_error(Hr, P.p1, P.p2, i) <= P.thr)) continue;
                const double t = term(e, i);
                acc = mx ? fmax(acc, t) : acc + t;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(acc, o, 64); acc = mx ? fmax(acc, t) : acc + t; }
            if (lane == 0) rw[RF_RED + e] = acc;
        }
    }
    // the sums of one LM pass at the parameters x[0..7]: JtJ, Jtr, |r|^2 and the residuals' largest magnitude (full), or |r|^2 alone
    __device__ static void lm_pass(const Problem& P, const double* Hr, double* rw, const double* x, bool full) {
        const LmParams h{x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]};
        reduce(P, Hr, rw, full ? 0 : 44, full ? 46 : 45, full, [&](int e, int i) {
            const float2 M = ((const float2*)P.p1)[i], m = ((const float2*)P.p2)[i];
            const LmPoint q = hg_lm_point(h, M.x, M.y, m.x, m.y);
            return e == 45 ? fmax(fabs(q.rx), fabs(q.ry)) : hg_lm_term(e, q);
        });
    }

    // findHomography behind the registrator, for a model from the loop (n > 4): runKernel on the inliers, then LMSolver; the result into sh.best
    __device__ static void finish(const Problem& P, double* ws, Shared& sh) {
        if (!(sh.max_good > 0) || direct(P.n)) return;   // (uniform: written in front of the loop's last barrier)
        const int tid = (int)threadIdx.x;
        double Hr[9];   // the RANSAC model: it says who is an inlier, whatever sh.best becomes
#pragma unroll
        for (int k = 0; k < 9; k++) Hr[k] = sh.best[k];
        const int count = sh.max_good;
        double* rw = ws;
        int* ind = sh.x.ind;
        __syncthreads();   // every thread has the model and is through with the mask; the workspaces are free
        reduce(P, Hr, rw, 0, 4, false, [&](int e, int i) { return (double)(e < 2 ? P.p2 : P.p1)[2 * i + (e & 1)]; });
        __syncthreads();
        if (tid == 0) {
            #pragma unroll 1
            for (int e = 0; e < 4; e++) rw[RF_STAT + e] = rw[RF_RED + e] / count;
        }
        __syncthreads();
        const double cmx = rw[RF_STAT], cmy = rw[RF_STAT + 1], cMx = rw[RF_STAT + 2], cMy = rw[RF_STAT + 3];
        reduce(P, Hr, rw, 0, 4, false, [&](int e, int i) { return fabs((e < 2 ? P.p2 : P.p1)[2 * i + (e & 1)] - (e == 0 ? cmx : e == 1 ? cmy : e == 2 ? cMx : cMy)); });
        __syncthreads();
        if (tid == 0) {
            bool ok = true;
            #pragma unroll 1
            for (int e = 0; e < 4; e++) {
                const double s = rw[RF_RED + e];
                if (fabs(s) < DBL_EPSILON) ok = false;
                rw[RF_STAT + 4 + e] = count / s;
            }
            sh.x.flag[0] = ok;
        }
        __syncthreads();
        if (sh.x.flag[0]) {
            const double smx = rw[RF_STAT + 4], smy = rw[RF_STAT + 5], sMx = rw[RF_STAT + 6], sMy = rw[RF_STAT + 7];
            reduce(P, Hr, rw, 0, 45, false, [&](int e, int i) {
                int j, k;
                hg_tri(e, 9, &j, &k);
                const float2 M = ((const float2*)P.p1)[i], m = ((const float2*)P.p2)[i];
                const double x = (m.x - cmx) * smx, y = (m.y - cmy) * smy, X = (M.x - cMx) * sMx, Y = (M.y - cMy) * sMy;
                return hg_lx(j, X, Y, x) * hg_lx(k, X, Y, x) + hg_ly(j, X, Y, y) * hg_ly(k, X, Y, y);
            });
            __syncthreads();
            if (tid == 0) {
                hg_set_T(rw, 1, 0, cMx, cMy, cmx, cmy, sMx, sMy, smx, smy);
                if (hg_refit_solve(rw, ind)) {
                    #pragma unroll 1
                    for (int k = 0; k < 9; k++) sh.best[k] = rw[27 + k];
                }
            }
        }
        if (tid == 0) {
            #pragma unroll 1
            for (int i = 0; i < 8; i++) rw[RF_X + i] = sh.best[i];
        }
        __syncthreads();
        lm_pass(P, Hr, rw, rw + RF_X, true);
        __syncthreads();
        if (tid == 0) hg_lm_begin(rw);
        #pragma unroll 1
        for (int iter = 1;; iter++) {
            if (tid == 0) hg_lm_step(rw, ind);
            __syncthreads();
            lm_pass(P, Hr, rw, rw + RF_XD, false);
            __syncthreads();
            if (tid == 0) sh.x.flag[1] = hg_lm_decide(rw, rw[RF_RED + 44], ind);
            __syncthreads();
            if (sh.x.flag[1]) {
                lm_pass(P, Hr, rw, rw + RF_X, true);
                __syncthreads();
                if (tid == 0) hg_lm_load(rw);
            }
            if (tid == 0) sh.x.flag[2] = hg_lm_proceed(rw, iter);
            __syncthreads();
            if (!sh.x.flag[2]) break;
        }
        if (tid == 0) {
            #pragma unroll 1
            for (int i = 0; i < 8; i++) sh.best[i] = rw[RF_X + i];
        }
    }
};
static_assert((size_t)HG_R * HG_WS * sizeof(double) + sizeof(HomogModel::Shared) <= 64 * 1024, "the workgroup's LDS stays within the default limit");

}  // namespace

__global__ __launch_bounds__(HG_THREADS) void k_homography_ransac(const HomographyProblem* __restrict__ probs) { BACKEND_PRIO();
    extern __shared__ __attribute__((aligned(16))) double homog_lds[];   // HG_R interleaved solver workspaces of HG_WS doubles, then the shared block
    const HomographyProblem P = probs[blockIdx.x];
    whole_ransac<HomogModel>(P, homog_lds, *(HomogModel::Shared*)(homog_lds + HG_R * HG_WS), HG_R, HG_WAVES);
}

hipError_t launch_homography_ransac(hipStream_t s, const HomographyProblem* d_probs, int n_probs) {
    if (n_probs <= 0) return hipSuccess;
    if (!d_probs) return hipErrorInvalidValue;
    const size_t lds = (size_t)HG_R * HG_WS * sizeof(double) + sizeof(HomogModel::Shared);
    ProfScope ps(K_FIVEPOINT, s);
    hipLaunchKernelGGL(k_homography_ransac, dim3(n_probs), dim3(HG_THREADS), lds, s, d_probs);
    return hipGetLastError();
}

}  // namespace pmv
