// gfx950 fundamental-matrix RANSAC: cv::findFundamentalMat(p1, p2, FM_RANSAC, threshold, confidence, mask) for n >= 15 correspondences
// (pmv_find_fundamental_mat, include/pmv_hip.h), the rejectWithF of a KLT loop.
// k_fundamental_ransac: the whole adaptive RANSAC of one call in ONE workgroup, in the round structure that pmv_ransac.h states for it and
// for k_essential_ransac (backend_fivepoint.hip); this file holds what FMEstimatorCallback holds: checkSubset (the collinearity test on the
// subset's last point, up to 10000 attempts per subset), the seven-point solver and the error.
// What differs from the five-point kernel follows from the size of the solver (a 7x9 elimination, a cubic, up to three 3x3 builds: ~10^3
// dependent FP64 operations instead of ~10^5): ONE LANE solves one hypothesis, so a round holds up to 64 of them, and their workspaces
// (FD_WS doubles each) are interleaved in LDS - element k of hypothesis h at k * R + h - so that the lanes of a wave, which all execute the
// same statement on the same k, read consecutive doubles (ds_read_b64 banks on (address / 4) mod 64: a block per lane would put every
// lane of a half-wave on the same bank). As locals the arrays would be indexed dynamically, i.e. scratch memory (backend_fivepoint.hip:120);
// no loop of the solver is unrolled.
// Every solver statement is tests/twin/fundamental_twin.cpp's, in its order: IEEE + - * / sqrt only (-ffp-contract=off, no fast-math), so
// found, F, the mask and the sample count are the twin's bits.
#include "pmv_ctx.h"
#include "backend.h"
#include "pmv_prof.h"
#include "pmv_ransac.h"
#include <float.h>
#include <atomic>
#include <cstdlib>

namespace pmv {

namespace {

constexpr int FD_WS = 108;           // doubles per hypothesis: A 7x9 at 0 | f1 at 63 | f2 at 72 | up to three models at 81
constexpr int FD_THREADS = 512;      // 8 waves score; the lanes of wave 0 solve

__device__ inline double fd_cubic_at(double a1, double a2, double a3, double x) { return ((x + a1) * x + a2) * x + a3; }
__device__ inline double fd_cubic_slope(double a1, double a2, double x) { return (3 * x + 2 * a1) * x + a2; }
__device__ inline double fd_cubic_polish(double a1, double a2, double a3, double x) {
    #pragma unroll 1
    for (int it = 0; it < 2; it++) {
        const double f = fd_cubic_at(a1, a2, a3, x), g = fd_cubic_slope(a1, a2, x);
        if (f == 0 || g == 0) break;
        const double xn = x - f / g;
        if (!(fabs(fd_cubic_at(a1, a2, a3, xn)) <= fabs(f))) break;
        x = xn;
    }
    return x;
}

// cv::solveCubic: its case analysis for the NUMBER of roots, IEEE arithmetic for their values (fundamental_twin.cpp:solve_cubic)
__device__ int fd_solve_cubic(double c0, double c1, double c2, double c3, double* x0p, double* x1p, double* x2p) {
    double a0 = c0, a1 = c1, a2 = c2, a3 = c3;
    double x0 = 0., x1 = 0., x2 = 0.;
    int n = 0;
    if (a0 == 0) {
        if (a1 == 0) {
            if (a2 == 0) n = a3 == 0 ? -1 : 0;
            else { x0 = -a3 / a2; n = 1; }
        } else {
            double d = a2 * a2 - 4 * a1 * a3;
            if (d >= 0) {
                d = sqrt(d);
                const double q1 = (-a2 + d) * 0.5, q2 = (a2 + d) * -0.5;
                if (fabs(q1) > fabs(q2)) { x0 = q1 / a1; x1 = a3 / q1; }
                else { x0 = q2 / a1; x1 = a3 / q2; }
                n = d > 0 ? 2 : 1;
            }
        }
    } else {
        a0 = 1. / a0;
        a1 *= a0; a2 *= a0; a3 *= a0;
        const double Q = (a1 * a1 - 3 * a2) * (1. / 9);
        const double R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1. / 54);
        const double Qcubed = Q * Q * Q;
        const double d = Qcubed - R * R;
        if (d == 0) {
            const double sq = sqrt(Q), e = R >= 0 ? sq : -sq;
            x0 = -2 * e - a1 / 3;
            x1 = e - a1 / 3;
            n = x0 == x1 ? 1 : 2;
            x1 = x0 == x1 ? 0 : x1;
        } else if (!(d > 0) && !(d < 0)) {
            n = 0;
        } else {
            double m = fabs(a1);
            if (fabs(a2) > m) m = fabs(a2);
            if (fabs(a3) > m) m = fabs(a3);
            double lo = -(1 + m), hi = 1 + m;
            double x = 0.5 * (lo + hi);
            #pragma unroll 1
            for (int it = 0; it < 200; it++) {
                const double f = fd_cubic_at(a1, a2, a3, x);
                if (f == 0) break;
                if (f < 0) lo = x; else hi = x;
                const double g = fd_cubic_slope(a1, a2, x);
                double xn = g != 0 ? x - f / g : lo;
                if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
                if (xn == x) break;
                x = xn;
            }
            const double r = fd_cubic_polish(a1, a2, a3, x);
            if (d < 0) { x0 = r; n = 1; }
            else {
                const double b1 = a1 + r, b0 = a2 + r * b1;
                double disc = b1 * b1 - 4 * b0;
                if (!(disc > 0)) disc = 0;
                const double sd = sqrt(disc);
                const double q = b1 >= 0 ? (b1 + sd) * -0.5 : (-b1 + sd) * 0.5;
                double s = q, t = q != 0 ? b0 / q : 0.;
                s = fd_cubic_polish(a1, a2, a3, s);
                t = fd_cubic_polish(a1, a2, a3, t);
                double u = r, w;
                if (s > t) { w = s; s = t; t = w; }
                if (u > t) { w = u; u = t; t = w; }
                if (s > u) { w = s; s = u; u = w; }
                x0 = s; x1 = t; x2 = u;
                n = 3;
            }
        }
    }
    *x0p = x0; *x1p = x1; *x2p = x2;
    return n;
}

// run7Point on the subset idx[0..6] (fundamental_twin.cpp:seven_point): the workspace of hypothesis h is W(k) = ws[k * R + h]
#define W(k) ws[(k) * R + h]
#define CP(k) cp[(k) * R + h]
__device__ int fd_seven_point(const float* __restrict__ p1, const float* __restrict__ p2, const int* idx, double* ws, unsigned char* cp, int R, int h) {
    #pragma unroll 1
    for (int i = 0; i < 7; i++) {
        const double x0 = p1[2 * idx[i]], y0 = p1[2 * idx[i] + 1], x1 = p2[2 * idx[i]], y1 = p2[2 * idx[i] + 1];
        W(i * 9 + 0) = x1 * x0; W(i * 9 + 1) = x1 * y0; W(i * 9 + 2) = x1;
        W(i * 9 + 3) = y1 * x0; W(i * 9 + 4) = y1 * y0; W(i * 9 + 5) = y1;
        W(i * 9 + 6) = x0; W(i * 9 + 7) = y0; W(i * 9 + 8) = 1.0;
    }
    #pragma unroll 1
    for (int c = 0; c < 9; c++) CP(c) = (unsigned char)c;
    #pragma unroll 1
    for (int r = 0; r < 7; r++) {
        int pr = r, pc = r;
        double best = -1;
        #pragma unroll 1
        for (int i = r; i < 7; i++)
            #pragma unroll 1
            for (int j = r; j < 9; j++) { const double v = fabs(W(i * 9 + j)); if (v > best) { best = v; pr = i; pc = j; } }
        if (!(best > 1e-300)) return 0;
        if (pr != r) {
            #pragma unroll 1
            for (int j = 0; j < 9; j++) { const double t = W(r * 9 + j); W(r * 9 + j) = W(pr * 9 + j); W(pr * 9 + j) = t; }
        }
        if (pc != r) {
            #pragma unroll 1
            for (int i = 0; i < 7; i++) { const double t = W(i * 9 + r); W(i * 9 + r) = W(i * 9 + pc); W(i * 9 + pc) = t; }
            const unsigned char t = CP(r); CP(r) = CP(pc); CP(pc) = t;
        }
        const double inv = 1.0 / W(r * 9 + r);
        #pragma unroll 1
        for (int j = 0; j < 9; j++) W(r * 9 + j) *= inv;
        #pragma unroll 1
        for (int i = 0; i < 7; i++) {
            if (i == r) continue;
            const double f = W(i * 9 + r);
            if (f == 0.0) continue;
            #pragma unroll 1
            for (int j = 0; j < 9; j++) W(i * 9 + j) -= f * W(r * 9 + j);
        }
    }
    #pragma unroll 1
    for (int k = 0; k < 2; k++) {
        double nrm = 1.0;
        #pragma unroll 1
        for (int i = 0; i < 7; i++) nrm += W(i * 9 + 7 + k) * W(i * 9 + 7 + k);
        nrm = sqrt(nrm);
        #pragma unroll 1
        for (int j = 0; j < 9; j++) {
            const double v = j < 7 ? -W(j * 9 + 7 + k) : (j == 7 + k ? 1.0 : 0.0);
            W(63 + 9 * k + CP(j)) = v / nrm;
        }
    }
#define F1(i) W(63 + (i))
#define F2(i) W(72 + (i))
    #pragma unroll 1
    for (int i = 0; i < 9; i++) F1(i) -= F2(i);
    double t0 = F2(4) * F2(8) - F2(5) * F2(7);
    double t1 = F2(3) * F2(8) - F2(5) * F2(6);
    double t2 = F2(3) * F2(7) - F2(4) * F2(6);
    const double c3 = F2(0) * t0 - F2(1) * t1 + F2(2) * t2;
    const double c2 = F1(0) * t0 - F1(1) * t1 + F1(2) * t2 -
                      F1(3) * (F2(1) * F2(8) - F2(2) * F2(7)) +
                      F1(4) * (F2(0) * F2(8) - F2(2) * F2(6)) -
                      F1(5) * (F2(0) * F2(7) - F2(1) * F2(6)) +
                      F1(6) * (F2(1) * F2(5) - F2(2) * F2(4)) -
                      F1(7) * (F2(0) * F2(5) - F2(2) * F2(3)) +
                      F1(8) * (F2(0) * F2(4) - F2(1) * F2(3));
    t0 = F1(4) * F1(8) - F1(5) * F1(7);
    t1 = F1(3) * F1(8) - F1(5) * F1(6);
    t2 = F1(3) * F1(7) - F1(4) * F1(6);
    const double c0 = F1(0) * t0 - F1(1) * t1 + F1(2) * t2;
    const double c1 = F2(0) * t0 - F2(1) * t1 + F2(2) * t2 -
                      F2(3) * (F1(1) * F1(8) - F1(2) * F1(7)) +
                      F2(4) * (F1(0) * F1(8) - F1(2) * F1(6)) -
                      F2(5) * (F1(0) * F1(7) - F1(1) * F1(6)) +
                      F2(6) * (F1(1) * F1(5) - F1(2) * F1(4)) -
                      F2(7) * (F1(0) * F1(5) - F1(2) * F1(3)) +
                      F2(8) * (F1(0) * F1(4) - F1(1) * F1(3));
    double r0, r1, r2;
    const int n = fd_solve_cubic(c0, c1, c2, c3, &r0, &r1, &r2);
    if (n < 1 || n > 3) return 0;
    #pragma unroll 1
    for (int k = 0; k < n; k++) {
        const double rk = k == 0 ? r0 : k == 1 ? r1 : r2;
        double lambda = rk, mu = 1.;
        const double s = F1(8) * rk + F2(8);
        if (fabs(s) > DBL_EPSILON) { mu = 1. / s; lambda *= mu; W(81 + 9 * k + 8) = 1.; }
        else W(81 + 9 * k + 8) = 0.;
        #pragma unroll 1
        for (int i = 0; i < 8; i++) W(81 + 9 * k + i) = F1(i) * lambda + F2(i) * mu;
    }
#undef F1
#undef F2
    return n;
}
#undef W
#undef CP

// FMEstimatorCallback::computeError of correspondence i (fundamental_twin.cpp:fm_error)
__device__ inline float fd_error(const double* F, const float* __restrict__ p1, const float* __restrict__ p2, int i) {
    const double m1x = p1[2 * i], m1y = p1[2 * i + 1], m2x = p2[2 * i], m2y = p2[2 * i + 1];
    double a = F[0] * m1x + F[1] * m1y + F[2];
    double b = F[3] * m1x + F[4] * m1y + F[5];
    double c = F[6] * m1x + F[7] * m1y + F[8];
    const double s2 = 1. / (a * a + b * b);
    const double d2 = m2x * a + m2y * b + c;
    a = F[0] * m2x + F[3] * m2y + F[6];
    b = F[1] * m2x + F[4] * m2y + F[7];
    c = F[2] * m2x + F[5] * m2y + F[8];
    const double s1 = 1. / (a * a + b * b);
    const double d1 = m1x * a + m1y * b + c;
    const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
    return (float)(e1 < e2 ? e2 : e1);
}

// FMEstimatorCallback as pmv_ransac.h's model: one lane per hypothesis on the interleaved workspaces, checkSubset on the subset's last point
struct FundModel {
    using Problem = FundamentalProblem;
    static constexpr int S = 7, MODELS = 3, MAX_R = FUND_MAX_R, MAX_ATTEMPTS = 10000;
    struct Extra {
        alignas(8) float sp[28];            // the points of the subset thread 0 is testing: image 1, then image 2 (aligned: a point is one ds_read_b64)
        unsigned char cp[FUND_MAX_R * 9];   // column permutations of the eliminations, interleaved like the workspaces
    };
    using Shared = WholeShared<FundModel>;
    __device__ static bool direct(int) { return false; }   // (fundamental_check: n >= 15)
    __device__ static bool solve_direct(const Problem&, double*, Shared&) { return false; }
    __device__ static bool subset_ok(const Problem& P, const int* idx, Extra& x) {
        // the subset's points first, all loads in flight together: the test below then runs on LDS instead of waiting for global
        // memory once per pair (measured: ~10 us per subset before, which made the draw the longest part of a round)
#pragma unroll
        for (int i = 0; i < 7; i++) {
            const float2 a = ((const float2*)P.p1)[idx[i]], c = ((const float2*)P.p2)[idx[i]];
            x.sp[2 * i] = a.x; x.sp[2 * i + 1] = a.y; x.sp[14 + 2 * i] = c.x; x.sp[15 + 2 * i] = c.y;
        }
        return !whole_last_point_collinear<7>(x.sp) && !whole_last_point_collinear<7>(x.sp + 14);
    }
    __device__ static void solve(const Problem& P, double* ws, Shared& sh, int R, int nh) {
        const int tid = (int)threadIdx.x;
        if (tid < nh) sh.nm[tid] = fd_seven_point(P.p1, P.p2, sh.idx + 7 * tid, ws, sh.x.cp, R, tid);
    }
    __device__ static double model(const double* ws, int R, int b, int mi, int k) { return ws[(81 + 9 * mi + k) * R + b]; }
    __device__ static float error(const double* F, const float* __restrict__ p1, const float* __restrict__ p2, int i) { return fd_error(F, p1, p2, i); }
    __device__ static void finish(const Problem&, double*, Shared&) {}   // (cv has no refit for F)
};
static_assert((size_t)FUND_MAX_R * FD_WS * sizeof(double) + sizeof(FundModel::Shared) <= 64 * 1024, "the workgroup's LDS stays within the default limit");

}  // namespace

__global__ __launch_bounds__(FD_THREADS) void k_fundamental_ransac(const FundamentalProblem* __restrict__ probs, int R) { BACKEND_PRIO();
    extern __shared__ __attribute__((aligned(16))) double fund_lds[];   // R interleaved solver workspaces of FD_WS doubles, then the shared block
    const FundamentalProblem P = probs[blockIdx.x];
    whole_ransac<FundModel>(P, fund_lds, *(FundModel::Shared*)(fund_lds + R * FD_WS), R, FD_THREADS / 64);
}

namespace {
std::atomic<int> g_fund_r{0};   // pmv_debug_set_fundamental_r (0: the environment's value or the default)
int clamp_r(int r) { return r < 1 ? 1 : r > FUND_MAX_R ? FUND_MAX_R : r; }
}  // namespace

void fundamental_set_round_width(int r) { g_fund_r.store(r <= 0 ? 0 : clamp_r(r)); }
int fundamental_round_width() {
    static const int R = [] { const char* e = getenv("PMV_FUNDAMENTAL_R"); return clamp_r(e ? atoi(e) : FUND_DEFAULT_R); }();
    const int r = g_fund_r.load();
    return r ? r : R;
}

hipError_t launch_fundamental_ransac(hipStream_t s, const FundamentalProblem* d_probs, int n_probs) {
    if (n_probs <= 0) return hipSuccess;
    if (!d_probs) return hipErrorInvalidValue;
    const int R = fundamental_round_width();
    const size_t lds = (size_t)R * FD_WS * sizeof(double) + sizeof(FundModel::Shared);
    ProfScope ps(K_FIVEPOINT, s);
    hipLaunchKernelGGL(k_fundamental_ransac, dim3(n_probs), dim3(FD_THREADS), lds, s, d_probs, R);
    return hipGetLastError();
}

}  // namespace pmv
