// TEST INFRASTRUCTURE ONLY. CPU restatement of pmv_triangulate_tracks (include/pmv_hip.h): N-view DLT triangulation of track landmarks,
// an optional Gauss-Newton refinement of the reprojection error, and the depth / reprojection / parallax gates. It FIXES the arithmetic of
// the contract: the GPU tests compare out_xyz, out_status, out_err and out_good with this file's results bit for bit (compiled with
// -ffp-contract=off; every sum below is sequential, in the order written). It includes nothing from the library or the oracle.
//   lists       a landmark's observations in order of appearance in the caller's arrays (stable counting sort by pt_idx)
//   DLT         two rows per observation, x P[8+k] - P[k] and y P[8+k] - P[4+k]; AtA accumulated row by row from 0; cyclic Jacobi (the
//               statement of d_jacobi_eig<4> / vmath::jacobi_eig); the eigenvector of the smallest eigenvalue; X = Qh[0..2] / Qh[3]
//   refinement  cost, JtJ and Jtr of one X in one pass over the list; the step from the explicit adjugate over the determinant; a step is
//               taken only if the new cost is strictly smaller, and the first step that is not ends the refinement (an undamped step from
//               the same X would be the same step again)
//   gates       no early exit, status bits OR-ed; the camera centres by the adjugate, the cosine bound from libm's cos on the host
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

enum { TRI_OK = 0, TRI_FEW_VIEWS = 1, TRI_DEGENERATE = 2, TRI_DEPTH = 4, TRI_REPROJ = 8, TRI_PARALLAX = 16 };

void jacobi4(double* A, double* w, double* V) {
    const int n = 4;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i * n + j] = (i == j) ? 1.0 : 0.0;
    double tol_abs = 0;
    for (int i = 0; i < n; i++) tol_abs += std::fabs(A[i * n + i]);
    tol_abs *= 1e-17;
    for (int sweep = 0; sweep < 30; sweep++) {
        int rotated = 0;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double app = A[p * n + p], aqq = A[q * n + q];
                if (std::fabs(apq) <= tol_abs) { A[p * n + q] = A[q * n + p] = 0.0; continue; }
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; k++) {
                    if (k == p || k == q) continue;
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    const double nkp = c * akp - s * akq, nkq = s * akp + c * akq;
                    A[k * n + p] = A[p * n + k] = nkp;
                    A[k * n + q] = A[q * n + k] = nkq;
                }
                A[p * n + p] = app - t * apq;
                A[q * n + q] = aqq + t * apq;
                A[p * n + q] = A[q * n + p] = 0.0;
                for (int k = 0; k < n; k++) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
                rotated++;
            }
        if (!rotated) break;
    }
    for (int i = 0; i < n; i++) w[i] = A[i * n + i];
    for (int i = 0; i < n - 1; i++) {
        int m = i;
        for (int j = i + 1; j < n; j++) if (w[j] < w[m]) m = j;
        if (m != i) {
            double t = w[i]; w[i] = w[m]; w[m] = t;
            for (int k = 0; k < n; k++) { t = V[k * n + i]; V[k * n + i] = V[k * n + m]; V[k * n + m] = t; }
        }
    }
}

inline bool finite_d(double v) { return std::fabs(v) < __builtin_huge_val(); }

struct Eval { double cost, H[6], g[3]; };   // H: 00 01 02 11 12 22

// cost, JtJ and Jtr of X over the observations s..e-1 of the sorted lists
void eval(const double* P, const double* obs, const int* cam, int s, int e, const double* X, Eval* E) {
    E->cost = 0;
    for (int k = 0; k < 6; k++) E->H[k] = 0;
    for (int k = 0; k < 3; k++) E->g[k] = 0;
    for (int o = s; o < e; o++) {
        const double* p = P + 12 * cam[o];
        const double x = obs[2 * o], y = obs[2 * o + 1];
        const double nu = p[0] * X[0] + p[1] * X[1] + p[2] * X[2] + p[3];
        const double nv = p[4] * X[0] + p[5] * X[1] + p[6] * X[2] + p[7];
        const double w = p[8] * X[0] + p[9] * X[1] + p[10] * X[2] + p[11];
        const double u = nu / w, v = nv / w;
        const double ru = u - x, rv = v - y;
        E->cost += ru * ru + rv * rv;
        double ju[3], jv[3];
        for (int k = 0; k < 3; k++) { ju[k] = (p[k] - u * p[8 + k]) / w; jv[k] = (p[4 + k] - v * p[8 + k]) / w; }
        E->H[0] += ju[0] * ju[0] + jv[0] * jv[0];
        E->H[1] += ju[0] * ju[1] + jv[0] * jv[1];
        E->H[2] += ju[0] * ju[2] + jv[0] * jv[2];
        E->H[3] += ju[1] * ju[1] + jv[1] * jv[1];
        E->H[4] += ju[1] * ju[2] + jv[1] * jv[2];
        E->H[5] += ju[2] * ju[2] + jv[2] * jv[2];
        for (int k = 0; k < 3; k++) E->g[k] += ju[k] * ru + jv[k] * rv;
    }
}

}  // namespace

extern "C" {

// C = -M^-1 p4 by the adjugate for each of the nc cameras; returns the index of the first camera with det M == 0 (its centre is not written), or -1
int tt_twin_centres(const double* P3x4, int nc, double* C3) {
    for (int c = 0; c < nc; c++) {
        const double* p = P3x4 + 12 * c;
        const double m00 = p[0], m01 = p[1], m02 = p[2], m10 = p[4], m11 = p[5], m12 = p[6], m20 = p[8], m21 = p[9], m22 = p[10];
        const double a00 = m11 * m22 - m12 * m21, a01 = m02 * m21 - m01 * m22, a02 = m01 * m12 - m02 * m11;
        const double a10 = m12 * m20 - m10 * m22, a11 = m00 * m22 - m02 * m20, a12 = m02 * m10 - m00 * m12;
        const double a20 = m10 * m21 - m11 * m20, a21 = m01 * m20 - m00 * m21, a22 = m00 * m11 - m01 * m10;
        const double det = m00 * a00 + m01 * a10 + m02 * a20;
        if (det == 0) return c;
        C3[3 * c] = -(a00 * p[3] + a01 * p[7] + a02 * p[11]) / det;
        C3[3 * c + 1] = -(a10 * p[3] + a11 * p[7] + a12 * p[11]) / det;
        C3[3 * c + 2] = -(a20 * p[3] + a21 * p[7] + a22 * p[11]) / det;
    }
    return -1;
}

// pmv_triangulate_tracks on valid arguments. Returns 0, or -(1 + c) if the parallax gate is on and camera c has det M == 0 (nothing written).
// Optional diagnostics: out_Qh (np x 4: the DLT's homogeneous vector, zeros for FEW_VIEWS), out_costs (np x (refine_iters + 1): the cost at
// the DLT's X and after every accepted step, NaN behind the last), out_steps (np: accepted steps).
int tt_twin_run(const double* P3x4, int nc, const double* obs_xy, const int* cam_idx, const int* pt_idx, int n_obs, int np, int min_views,
                int refine_iters, double min_depth, double max_depth, double max_reproj, double min_parallax_deg, double* out_xyz,
                uint8_t* out_status, double* out_err, int* out_good, double* out_Qh, double* out_costs, int* out_steps) {
    const double huge = __builtin_huge_val();
    const bool parallax_on = min_parallax_deg > 0, reproj_on = max_reproj < huge;
    std::vector<double> C((size_t)3 * (nc > 0 ? nc : 1), 0.0);
    double cos_thr = 1.0;
    if (parallax_on) {
        const int bad = tt_twin_centres(P3x4, nc, C.data());
        if (bad >= 0) return -(1 + bad);
        cos_thr = std::cos(min_parallax_deg * M_PI / 180.0);
    }
    // stable counting sort by landmark
    std::vector<int> start((size_t)np + 1, 0), cam((size_t)n_obs);
    std::vector<double> obs((size_t)2 * n_obs);
    for (int i = 0; i < n_obs; i++) start[(size_t)pt_idx[i] + 1]++;
    for (int p = 0; p < np; p++) start[(size_t)p + 1] += start[p];
    {
        std::vector<int> fill(start.begin(), start.end() - 1);
        for (int i = 0; i < n_obs; i++) {
            const int o = fill[pt_idx[i]]++;
            obs[2 * (size_t)o] = obs_xy[2 * (size_t)i]; obs[2 * (size_t)o + 1] = obs_xy[2 * (size_t)i + 1]; cam[o] = cam_idx[i];
        }
    }
    int good = 0;
    for (int p = 0; p < np; p++) {
        const int s = start[p], e = start[(size_t)p + 1], m = e - s;
        double* xyz = out_xyz + 3 * (size_t)p;
        if (out_Qh) for (int k = 0; k < 4; k++) out_Qh[4 * (size_t)p + k] = 0;
        if (out_costs) for (int k = 0; k <= refine_iters; k++) out_costs[(size_t)p * (refine_iters + 1) + k] = NAN;
        if (out_steps) out_steps[p] = 0;
        if (m < min_views) {
            xyz[0] = xyz[1] = xyz[2] = 0; out_status[p] = TRI_FEW_VIEWS;
            if (out_err) out_err[p] = huge;
            continue;
        }
        // DLT
        double AtA[16];
        for (int k = 0; k < 16; k++) AtA[k] = 0;
        for (int o = s; o < e; o++) {
            const double* pc = P3x4 + 12 * cam[o];
            const double x = obs[2 * (size_t)o], y = obs[2 * (size_t)o + 1];
            double r[4];
            for (int k = 0; k < 4; k++) r[k] = x * pc[8 + k] - pc[k];
            for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) AtA[a * 4 + b] += r[a] * r[b];
            for (int k = 0; k < 4; k++) r[k] = y * pc[8 + k] - pc[4 + k];
            for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) AtA[a * 4 + b] += r[a] * r[b];
        }
        double w4[4], V4[16];
        jacobi4(AtA, w4, V4);
        const double Qh[4] = {V4[0], V4[4], V4[8], V4[12]};
        if (out_Qh) for (int k = 0; k < 4; k++) out_Qh[4 * (size_t)p + k] = Qh[k];
        double X[3] = {Qh[0] / Qh[3], Qh[1] / Qh[3], Qh[2] / Qh[3]};
        if (Qh[3] == 0 || !finite_d(X[0]) || !finite_d(X[1]) || !finite_d(X[2])) {
            xyz[0] = xyz[1] = xyz[2] = 0; out_status[p] = TRI_DEGENERATE;
            if (out_err) out_err[p] = huge;
            continue;
        }
        // Gauss-Newton
        if (refine_iters > 0) {
            Eval E, En;
            eval(P3x4, obs.data(), cam.data(), s, e, X, &E);
            if (out_costs) out_costs[(size_t)p * (refine_iters + 1)] = E.cost;
            for (int it = 0; it < refine_iters; it++) {
                if (!finite_d(E.cost)) break;
                const double h00 = E.H[0], h01 = E.H[1], h02 = E.H[2], h11 = E.H[3], h12 = E.H[4], h22 = E.H[5];
                const double c00 = h11 * h22 - h12 * h12, c01 = h02 * h12 - h01 * h22, c02 = h01 * h12 - h02 * h11;
                const double c11 = h00 * h22 - h02 * h02, c12 = h01 * h02 - h00 * h12, c22 = h00 * h11 - h01 * h01;
                const double det = h00 * c00 + h01 * c01 + h02 * c02;
                if (det == 0 || !finite_d(det)) break;
                double Xn[3];
                Xn[0] = X[0] + -(c00 * E.g[0] + c01 * E.g[1] + c02 * E.g[2]) / det;
                Xn[1] = X[1] + -(c01 * E.g[0] + c11 * E.g[1] + c12 * E.g[2]) / det;
                Xn[2] = X[2] + -(c02 * E.g[0] + c12 * E.g[1] + c22 * E.g[2]) / det;
                eval(P3x4, obs.data(), cam.data(), s, e, Xn, &En);
                if (!(En.cost < E.cost)) break;
                X[0] = Xn[0]; X[1] = Xn[1]; X[2] = Xn[2];
                E = En;
                if (out_steps) out_steps[p]++;
                if (out_costs) out_costs[(size_t)p * (refine_iters + 1) + out_steps[p]] = E.cost;
            }
        }
        // gates
        int st = 0;
        double ss = 0;
        for (int o = s; o < e; o++) {
            const double* pc = P3x4 + 12 * cam[o];
            const double x = obs[2 * (size_t)o], y = obs[2 * (size_t)o + 1];
            const double nu = pc[0] * X[0] + pc[1] * X[1] + pc[2] * X[2] + pc[3];
            const double nv = pc[4] * X[0] + pc[5] * X[1] + pc[6] * X[2] + pc[7];
            const double w = pc[8] * X[0] + pc[9] * X[1] + pc[10] * X[2] + pc[11];
            const double ru = nu / w - x, rv = nv / w - y;
            const double e2 = ru * ru + rv * rv;
            ss += e2;
            const double err = std::sqrt(e2);
            if (!(w >= min_depth && w <= max_depth)) st |= TRI_DEPTH;
            if (reproj_on && !(err <= max_reproj)) st |= TRI_REPROJ;
        }
        if (parallax_on) {
            double mincos = 1.0;
            for (int i = s; i < e; i++) {
                const double* ci = C.data() + 3 * cam[i];
                const double a0 = ci[0] - X[0], a1 = ci[1] - X[1], a2 = ci[2] - X[2];
                const double na = a0 * a0 + a1 * a1 + a2 * a2;
                for (int j = i + 1; j < e; j++) {
                    const double* cj = C.data() + 3 * cam[j];
                    const double b0 = cj[0] - X[0], b1 = cj[1] - X[1], b2 = cj[2] - X[2];
                    const double nb = b0 * b0 + b1 * b1 + b2 * b2;
                    const double cs = (a0 * b0 + a1 * b1 + a2 * b2) / std::sqrt(na * nb);
                    if (finite_d(cs) && cs < mincos) mincos = cs;
                }
            }
            if (!(mincos <= cos_thr)) st |= TRI_PARALLAX;
        }
        xyz[0] = X[0]; xyz[1] = X[1]; xyz[2] = X[2];
        out_status[p] = (uint8_t)st;
        if (out_err) out_err[p] = std::sqrt(ss / (double)m);
        good += st == 0;
    }
    *out_good = good;
    return 0;
}

}  // extern "C"
