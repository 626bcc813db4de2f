// CPU restatement of pmv_find_fundamental_mat (include/pmv_hip.h): cv::findFundamentalMat(p1, p2, FM_RANSAC, threshold, confidence, mask)
// for n >= 15, written from memory of OpenCV 3.4 (fundam.cpp: run7Point, FMEstimatorCallback; ptsetreg.cpp: RANSACPointSetRegistrator;
// mathfuncs.cpp: solveCubic). It is what fixes the bits of k_fundamental_ransac (csrc/backend_fundamental.hip): every floating-point
// statement below is IEEE + - * / sqrt in this order (-ffp-contract=off, no fast-math on both sides); the two places where cv's own
// bits cannot be had on a device - the SVD null space and the acos / cos / pow of solveCubic - are replaced as the header says.
// The solver's arrays are reached through W(k), so that the kernel's text is this text with another W.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr int MAX_ATTEMPTS = 10000;   // RANSACPointSetRegistrator::run calls getSubset(.., rng, 10000)
constexpr int MAX_ITERS = 1000;

struct RNG {   // cv::RNG: multiply-with-carry
    uint64_t state;
    explicit RNG(uint64_t s) : state(s) {}
    unsigned next() { state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32); return (unsigned)state; }
};

// haveCollinearPoints on the subset's LAST point (cv's quirk): against every pair (j, k < j) of the earlier ones
bool last_point_collinear(const float* p, const int* idx, int count) {
    const int i = count - 1;
    const float xi = p[2 * idx[i]], yi = p[2 * idx[i] + 1];
    for (int j = 0; j < i; j++) {
        const double dx1 = p[2 * idx[j]] - xi, dy1 = p[2 * idx[j] + 1] - yi;   // float subtractions, widened
        for (int k = 0; k < j; k++) {
            const double dx2 = p[2 * idx[k]] - xi, dy2 = p[2 * idx[k] + 1] - yi;
            if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
        }
    }
    return false;
}

// getSubset with modelPoints = 7 + FMEstimatorCallback::checkSubset; *refused counts the subsets checkSubset turned down
bool get_subset(RNG& rng, const float* p1, const float* p2, int n, int* idx, int* refused) {
    for (int attempt = 0; attempt < MAX_ATTEMPTS; attempt++) {
        for (int i = 0; i < 7;) {
            const int v = (int)(rng.next() % (unsigned)n);
            idx[i] = v;
            int j = 0;
            for (; j < i; j++) if (v == idx[j]) break;
            if (j == i) i++;
        }
        if (last_point_collinear(p1, idx, 7) || last_point_collinear(p2, idx, 7)) { if (refused) ++*refused; continue; }
        return true;
    }
    return false;
}

inline double cubic_at(double a1, double a2, double a3, double x) { return ((x + a1) * x + a2) * x + a3; }
inline double cubic_slope(double a1, double a2, double x) { return (3 * x + 2 * a1) * x + a2; }
// two Newton steps on the monic cubic; a step is taken only where it does not increase |f|
inline double cubic_polish(double a1, double a2, double a3, double x) {
    for (int it = 0; it < 2; it++) {
        const double f = cubic_at(a1, a2, a3, x), g = cubic_slope(a1, a2, x);
        if (f == 0 || g == 0) break;
        const double xn = x - f / g;
        if (!(fabs(cubic_at(a1, a2, a3, xn)) <= fabs(f))) break;
        x = xn;
    }
    return x;
}

// cv::solveCubic(c[0] x^3 + c[1] x^2 + c[2] x + c[3]): its case analysis decides how many roots there are; their values come from
// IEEE arithmetic only. Order of three roots: smallest, largest, middle (the order of cv's cos(t), cos(t + 2 pi / 3), cos(t + 4 pi / 3)).
int solve_cubic(double c0, double c1, double c2, double c3, double* x0p, double* x1p, double* x2p) {
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
        if (d == 0) {   // a double root: cv's pow(R, 1/3) is sign(R) sqrt(Q) here
            const double sq = sqrt(Q), e = R >= 0 ? sq : -sq;
            x0 = -2 * e - a1 / 3;
            x1 = e - a1 / 3;
            n = x0 == x1 ? 1 : 2;
            x1 = x0 == x1 ? 0 : x1;
        } else if (!(d > 0) && !(d < 0)) {
            n = 0;   // not a number: no root (cv's third branch would return a NaN)
        } else {
            // one real root inside the Cauchy bound by Newton's iteration kept inside a shrinking bracket (bisection where it leaves)
            double m = fabs(a1);
            if (fabs(a2) > m) m = fabs(a2);
            if (fabs(a3) > m) m = fabs(a3);
            double lo = -(1 + m), hi = 1 + m;   // f(lo) < 0 < f(hi)
            double x = 0.5 * (lo + hi);
            for (int it = 0; it < 200; it++) {
                const double f = cubic_at(a1, a2, a3, x);
                if (f == 0) break;
                if (f < 0) lo = x; else hi = x;
                const double g = cubic_slope(a1, a2, x);
                double xn = g != 0 ? x - f / g : lo;
                if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
                if (xn == x) break;
                x = xn;
            }
            const double r = cubic_polish(a1, a2, a3, x);
            if (d < 0) { x0 = r; n = 1; }
            else {
                // x^3 + a1 x^2 + a2 x + a3 = (x - r)(x^2 + b1 x + b0)
                const double b1 = a1 + r, b0 = a2 + r * b1;
                double disc = b1 * b1 - 4 * b0;
                if (!(disc > 0)) disc = 0;   // (cv's analysis says three real roots)
                const double sd = sqrt(disc);
                const double q = b1 >= 0 ? (b1 + sd) * -0.5 : (-b1 + sd) * 0.5;
                double s = q, t = q != 0 ? b0 / q : 0.;
                s = cubic_polish(a1, a2, a3, s);
                t = cubic_polish(a1, a2, a3, t);
                double u = r, w;
                if (s > t) { w = s; s = t; t = w; }
                if (u > t) { w = u; u = t; t = w; }
                if (s > u) { w = s; s = u; u = w; }   // s <= u <= t
                x0 = s; x1 = t; x2 = u;
                n = 3;
            }
        }
    }
    *x0p = x0; *x1p = x1; *x2p = x2;
    return n;
}

// run7Point on the subset idx[7] of the float points; workspace ws: A 7x9 at 0 | f1 at 63 | f2 at 72 | models 27 at 81 (108 doubles),
// cp: the column permutation (9). Returns the number of models (0..3); F at W(81 + 9 k)
constexpr int TW_WS = 108;
#define W(k) ws[(k)]
#define CP(k) cp[(k)]
int seven_point(const float* p1, const float* p2, const int* idx, double* ws, unsigned char* cp) {
    for (int i = 0; i < 7; i++) {
        const double x0 = p1[2 * idx[i]], y0 = p1[2 * idx[i] + 1], x1 = p2[2 * idx[i]], y1 = p2[2 * idx[i] + 1];
        W(i * 9 + 0) = x1 * x0; W(i * 9 + 1) = x1 * y0; W(i * 9 + 2) = x1;
        W(i * 9 + 3) = y1 * x0; W(i * 9 + 4) = y1 * y0; W(i * 9 + 5) = y1;
        W(i * 9 + 6) = x0; W(i * 9 + 7) = y0; W(i * 9 + 8) = 1.0;
    }
    // null space: Gauss-Jordan with complete pivoting (fp_essentials' construction for its 5x9 system), then two unit vectors
    for (int c = 0; c < 9; c++) CP(c) = (unsigned char)c;
    for (int r = 0; r < 7; r++) {
        int pr = r, pc = r;
        double best = -1;
        for (int i = r; i < 7; i++)
            for (int j = r; j < 9; j++) { const double v = fabs(W(i * 9 + j)); if (v > best) { best = v; pr = i; pc = j; } }
        if (!(best > 1e-300)) return 0;
        if (pr != r) for (int j = 0; j < 9; j++) { const double t = W(r * 9 + j); W(r * 9 + j) = W(pr * 9 + j); W(pr * 9 + j) = t; }
        if (pc != r) {
            for (int i = 0; i < 7; i++) { const double t = W(i * 9 + r); W(i * 9 + r) = W(i * 9 + pc); W(i * 9 + pc) = t; }
            const unsigned char t = CP(r); CP(r) = CP(pc); CP(pc) = t;
        }
        const double inv = 1.0 / W(r * 9 + r);
        for (int j = 0; j < 9; j++) W(r * 9 + j) *= inv;
        for (int i = 0; i < 7; i++) {
            if (i == r) continue;
            const double f = W(i * 9 + r);
            if (f == 0.0) continue;
            for (int j = 0; j < 9; j++) W(i * 9 + j) -= f * W(r * 9 + j);
        }
    }
    for (int k = 0; k < 2; k++) {
        double nrm = 1.0;   // the vector's own 1 at column 7 + k
        for (int i = 0; i < 7; i++) nrm += W(i * 9 + 7 + k) * W(i * 9 + 7 + k);
        nrm = sqrt(nrm);
        for (int j = 0; j < 9; j++) {
            const double v = j < 7 ? -W(j * 9 + 7 + k) : (j == 7 + k ? 1.0 : 0.0);
            W(63 + 9 * k + CP(j)) = v / nrm;
        }
    }
#define F1(i) W(63 + (i))
#define F2(i) W(72 + (i))
    // f = lambda f1 + (1 - lambda) f2, det f = 0: a cubic in lambda (cv: f1 -= f2 first)
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
    const int n = solve_cubic(c0, c1, c2, c3, &r0, &r1, &r2);
    if (n < 1 || n > 3) return 0;
    for (int k = 0; k < n; k++) {
        const double rk = k == 0 ? r0 : k == 1 ? r1 : r2;
        double lambda = rk, mu = 1.;
        const double s = F1(8) * rk + F2(8);
        if (fabs(s) > DBL_EPSILON) { mu = 1. / s; lambda *= mu; W(81 + 9 * k + 8) = 1.; }
        else W(81 + 9 * k + 8) = 0.;
        for (int i = 0; i < 8; i++) W(81 + 9 * k + i) = F1(i) * lambda + F2(i) * mu;
    }
#undef F1
#undef F2
    return n;
}
#undef W
#undef CP

// FMEstimatorCallback::computeError of correspondence i
inline float fm_error(const double* F, const float* p1, const float* p2, int i) {
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
    return (float)(e1 < e2 ? e2 : e1);   // std::max(e1, e2)
}

// RANSACUpdateNumIters(p, (n - g) / n, model_points, .) split as vo::five_point_iters_table splits it: the logarithms here ...
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

}  // namespace

extern "C" {

// the first `count` subsets of a call: returns how many were drawn before getSubset failed (count if it never did)
int fund_twin_subsets(const float* p1, const float* p2, int n, int count, int* out7, int* out_refused) {
    RNG rng((uint64_t)-1);
    int refused = 0, k = 0;
    for (; k < count; k++) if (!get_subset(rng, p1, p2, n, out7 + 7 * k, &refused)) break;
    if (out_refused) *out_refused = refused;
    return k;
}

int fund_twin_seven_point(const float* p1_7, const float* p2_7, double* F27) {
    const int idx[7] = {0, 1, 2, 3, 4, 5, 6};
    double ws[TW_WS];
    unsigned char cp[9];
    const int n = seven_point(p1_7, p2_7, idx, ws, cp);
    memcpy(F27, ws + 81, sizeof(double) * 9 * (size_t)n);
    return n;
}

int fund_twin_cubic(const double* c4, double* roots3) {
    return solve_cubic(c4[0], c4[1], c4[2], c4[3], roots3, roots3 + 1, roots3 + 2);
}

void fund_twin_errors(const double* F9, const float* p1, const float* p2, int n, float* err) {
    for (int i = 0; i < n; i++) err[i] = fm_error(F9, p1, p2, i);
}

void fund_twin_iters_table(int n, double confidence, int model_points, double* out_denoms, double* out_num) {
    iters_table(n, confidence, model_points, out_denoms, out_num);
}

int fund_twin_update_iters(const double* tab, int good, int max_iters) { return update_iters(tab, good, max_iters); }

// the whole call for n >= 15: returns found; F9 untouched and the mask all 0 when not. *out_updates: how often a model became the best
int fund_twin_find(const float* p1, const float* p2, int n, double threshold, double confidence, double* F9, uint8_t* mask, int* out_drawn,
                   int* out_updates) {
    const float thr = (float)(threshold * threshold);
    std::vector<double> tab((size_t)n + 2);
    iters_table(n, confidence, 7, tab.data() + 1, tab.data());
    RNG rng((uint64_t)-1);
    int niters = MAX_ITERS, max_good = 0, iter = 0, updates = 0;
    double best[9] = {0};
    for (; iter < niters; iter++) {
        int idx[7];
        if (!get_subset(rng, p1, p2, n, idx, nullptr)) break;   // (at iter 0: no model, nothing drawn)
        double ws[TW_WS];
        unsigned char cp[9];
        const int nm = seven_point(p1, p2, idx, ws, cp);
        for (int mi = 0; mi < nm; mi++) {
            const double* F = ws + 81 + 9 * mi;
            int good = 0;
            for (int i = 0; i < n; i++) good += fm_error(F, p1, p2, i) <= thr;
            if (good > (max_good > 6 ? max_good : 6)) {
                memcpy(best, F, sizeof(best));
                max_good = good;
                niters = update_iters(tab.data(), good, niters);
                updates++;
            }
        }
    }
    *out_drawn = iter;
    if (out_updates) *out_updates = updates;
    if (max_good <= 0) { memset(mask, 0, (size_t)n); return 0; }
    memcpy(F9, best, sizeof(best));
    for (int i = 0; i < n; i++) mask[i] = (uint8_t)(fm_error(best, p1, p2, i) <= thr);
    return 1;
}

}  // extern "C"
