// gfx950 N-view triangulation of track landmarks (pmv_triangulate_tracks, include/pmv_hip.h): per landmark the DLT over its observation
// list (two rows per observation, the 4x4 A^T A accumulated in list order, d_jacobi_eig<4>: the statement and the operation order of
// tri_dlt_body in backend_tri.hip), an optional Gauss-Newton refinement of the reprojection error, and the depth / reprojection / parallax
// gates. One lane per landmark, 64-lane workgroups; every sum is sequential per landmark in list order, the order of
// tests/twin/tri_tracks_twin.cpp => bit-identical results. The 4x4 and 3x3 accumulators are indexed at compile time only (registers); the
// loops over a landmark's observation run are the only ones with a run-time trip count.
// The projection matrices (and the camera centres of the parallax gate) go to LDS when nc <= TT_LDS_CAMS (7.5 KB); beyond that every lane
// reads them through L2. Results go straight into the request's mapped pinned result block; a workgroup counts itself done in the
// request's device counter behind a system fence, and the last one stores the request's sequence number into the block's completion word.
#include "pmv_ctx.h"
#include "backend.h"
#include "pmv_prof.h"
#include "pmv_dense.h"

namespace pmv {

namespace {

struct TTEval { double cost, H[6], g[3]; };   // H: 00 01 02 11 12 22

__device__ __forceinline__ bool tt_finite(double v) { return fabs(v) < __builtin_huge_val(); }

__device__ __forceinline__ void tt_load_cam(const double* __restrict__ Pp, int c, double* pc) {
#pragma unroll
    for (int k = 0; k < 12; k++) pc[k] = Pp[12 * c + k];
}

// cost, JtJ and Jtr of X over the observations s..e-1
__device__ __forceinline__ void tt_eval(const double* __restrict__ Pp, const double* __restrict__ obs, const int* __restrict__ cam, int s, int e,
                                        const double* X, TTEval& E) {
    E.cost = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) E.H[k] = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) E.g[k] = 0;
    #pragma unroll 1
    for (int o = s; o < e; o++) {
        double p[12];
        tt_load_cam(Pp, cam[o], p);
        const double x = obs[2 * (size_t)o], y = obs[2 * (size_t)o + 1];
        const double nu = p[0] * X[0] + p[1] * X[1] + p[2] * X[2] + p[3];
        const double nv = p[4] * X[0] + p[5] * X[1] + p[6] * X[2] + p[7];
        const double w = p[8] * X[0] + p[9] * X[1] + p[10] * X[2] + p[11];
        const double u = nu / w, v = nv / w;
        const double ru = u - x, rv = v - y;
        E.cost += ru * ru + rv * rv;
        double ju[3], jv[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { ju[k] = (p[k] - u * p[8 + k]) / w; jv[k] = (p[4 + k] - v * p[8 + k]) / w; }
        E.H[0] += ju[0] * ju[0] + jv[0] * jv[0];
        E.H[1] += ju[0] * ju[1] + jv[0] * jv[1];
        E.H[2] += ju[0] * ju[2] + jv[0] * jv[2];
        E.H[3] += ju[1] * ju[1] + jv[1] * jv[1];
        E.H[4] += ju[1] * ju[2] + jv[1] * jv[2];
        E.H[5] += ju[2] * ju[2] + jv[2] * jv[2];
#pragma unroll
        for (int k = 0; k < 3; k++) E.g[k] += ju[k] * ru + jv[k] * rv;
    }
}

// landmark p of request R; Pp / Cp: the projection matrices and the camera centres, in LDS or in the request's in-block
__device__ __forceinline__ void tt_landmark(const TriTracksProblem& R, const double* __restrict__ Pp, const double* __restrict__ Cp, const int p) {
    const double huge = __builtin_huge_val();
    const double* __restrict__ obs = R.obs;
    const int* __restrict__ cam = R.cam;
    double* __restrict__ o_xyz = (double*)(R.out + TT_OUT_HDR) + 3 * (size_t)p;
    double* __restrict__ o_err = (double*)(R.out + TT_OUT_HDR) + 3 * (size_t)R.np + p;
    uint8_t* __restrict__ o_st = (uint8_t*)(R.out + TT_OUT_HDR) + 32 * (size_t)R.np + p;
    const int s = R.start[p], e = R.start[p + 1], m = e - s;
    if (m < R.min_views) {
        o_xyz[0] = 0; o_xyz[1] = 0; o_xyz[2] = 0; *o_err = huge; *o_st = PMV_TRI_FEW_VIEWS;
        return;
    }
    double X[3];
    {
        double A[16], w4[4], V4[16];
#pragma unroll
        for (int k = 0; k < 16; k++) A[k] = 0;
        #pragma unroll 1
        for (int o = s; o < e; o++) {
            double pc[12], r[4];
            tt_load_cam(Pp, cam[o], pc);
            const double x = obs[2 * (size_t)o], y = obs[2 * (size_t)o + 1];
#pragma unroll
            for (int k = 0; k < 4; k++) r[k] = x * pc[8 + k] - pc[k];
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = a; b < 4; b++) A[a * 4 + b] += r[a] * r[b];
#pragma unroll
            for (int k = 0; k < 4; k++) r[k] = y * pc[8 + k] - pc[4 + k];
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = a; b < 4; b++) A[a * 4 + b] += r[a] * r[b];
        }
#pragma unroll
        for (int a = 1; a < 4; a++)
#pragma unroll
            for (int b = 0; b < a; b++) A[a * 4 + b] = A[b * 4 + a];   // (r[a] r[b] = r[b] r[a]: the lower half has the upper half's bits)
        d_jacobi_eig<4>(A, w4, V4);
        const double q3 = V4[12];
        X[0] = V4[0] / q3; X[1] = V4[4] / q3; X[2] = V4[8] / q3;
        if (q3 == 0 || !tt_finite(X[0]) || !tt_finite(X[1]) || !tt_finite(X[2])) {
            o_xyz[0] = 0; o_xyz[1] = 0; o_xyz[2] = 0; *o_err = huge; *o_st = PMV_TRI_DEGENERATE;
            return;
        }
    }
    if (R.refine_iters > 0) {
        TTEval E, En;
        tt_eval(Pp, obs, cam, s, e, X, E);
        #pragma unroll 1
        for (int it = 0; it < R.refine_iters; it++) {
            if (!tt_finite(E.cost)) break;
            const double h00 = E.H[0], h01 = E.H[1], h02 = E.H[2], h11 = E.H[3], h12 = E.H[4], h22 = E.H[5];
            const double c00 = h11 * h22 - h12 * h12, c01 = h02 * h12 - h01 * h22, c02 = h01 * h12 - h02 * h11;
            const double c11 = h00 * h22 - h02 * h02, c12 = h01 * h02 - h00 * h12, c22 = h00 * h11 - h01 * h01;
            const double det = h00 * c00 + h01 * c01 + h02 * c02;
            if (det == 0 || !tt_finite(det)) break;
            double Xn[3];
            Xn[0] = X[0] + -(c00 * E.g[0] + c01 * E.g[1] + c02 * E.g[2]) / det;
            Xn[1] = X[1] + -(c01 * E.g[0] + c11 * E.g[1] + c12 * E.g[2]) / det;
            Xn[2] = X[2] + -(c02 * E.g[0] + c12 * E.g[1] + c22 * E.g[2]) / det;
            tt_eval(Pp, obs, cam, s, e, Xn, En);
            if (!(En.cost < E.cost)) break;
            X[0] = Xn[0]; X[1] = Xn[1]; X[2] = Xn[2];
            E = En;
        }
    }
    int st = 0;
    double ss = 0;
    const bool reproj_on = R.max_reproj < huge;
    #pragma unroll 1
    for (int o = s; o < e; o++) {
        double pc[12];
        tt_load_cam(Pp, cam[o], pc);
        const double x = obs[2 * (size_t)o], y = obs[2 * (size_t)o + 1];
        const double nu = pc[0] * X[0] + pc[1] * X[1] + pc[2] * X[2] + pc[3];
        const double nv = pc[4] * X[0] + pc[5] * X[1] + pc[6] * X[2] + pc[7];
        const double w = pc[8] * X[0] + pc[9] * X[1] + pc[10] * X[2] + pc[11];
        const double ru = nu / w - x, rv = nv / w - y;
        const double e2 = ru * ru + rv * rv;
        ss += e2;
        const double err = sqrt(e2);
        if (!(w >= R.min_depth && w <= R.max_depth)) st |= PMV_TRI_DEPTH;
        if (reproj_on && !(err <= R.max_reproj)) st |= PMV_TRI_REPROJ;
    }
    if (R.parallax_on) {
        double mincos = 1.0;
        #pragma unroll 1
        for (int i = s; i < e; i++) {
            const int ci = cam[i];
            const double a0 = Cp[3 * ci] - X[0], a1 = Cp[3 * ci + 1] - X[1], a2 = Cp[3 * ci + 2] - X[2];
            const double na = a0 * a0 + a1 * a1 + a2 * a2;
            #pragma unroll 1
            for (int j = i + 1; j < e; j++) {
                const int cj = cam[j];
                const double b0 = Cp[3 * cj] - X[0], b1 = Cp[3 * cj + 1] - X[1], b2 = Cp[3 * cj + 2] - X[2];
                const double nb = b0 * b0 + b1 * b1 + b2 * b2;
                const double cs = (a0 * b0 + a1 * b1 + a2 * b2) / sqrt(na * nb);
                if (tt_finite(cs) && cs < mincos) mincos = cs;
            }
        }
        if (!(mincos <= R.cos_thr)) st |= PMV_TRI_PARALLAX;
    }
    o_xyz[0] = X[0]; o_xyz[1] = X[1]; o_xyz[2] = X[2];
    *o_err = sqrt(ss / (double)m);
    *o_st = (uint8_t)st;
}

// workgroup `block` of request R (block < the request's (np + 63) / 64 workgroups)
__device__ __forceinline__ void tri_tracks_body(const TriTracksProblem& R, const int block) {
    __shared__ double sP[TT_LDS_CAMS * 12];
    __shared__ double sC[TT_LDS_CAMS * 3];
    const int tid = (int)threadIdx.x;
    const bool lds = R.nc <= TT_LDS_CAMS;   // (uniform over the launch's workgroups of this request)
    if (lds) {
        for (int i = tid; i < 12 * R.nc; i += 64) sP[i] = R.P[i];
        if (R.parallax_on) for (int i = tid; i < 3 * R.nc; i += 64) sC[i] = R.C[i];
        __syncthreads();
    }
    const int p = block * 64 + tid;
    if (p < R.np) {
        if (lds) tt_landmark(R, sP, sC, p);
        else tt_landmark(R, R.P, R.C, p);
    }
    // the completion word: this workgroup's results are visible to the host before it counts itself; the last one to count signals
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        const unsigned blocks = (unsigned)((R.np + 63) / 64);
        const unsigned before = __hip_atomic_fetch_add(R.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1 == blocks) {
            __threadfence_system();
            __hip_atomic_store((unsigned*)(R.out + TT_OUT_DONE), R.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace

// one request: blockIdx.x = workgroup of 64 landmarks
__global__ __launch_bounds__(64) void k_tri_tracks(const TriTracksProblem* __restrict__ rec) { BACKEND_PRIO();
    const TriTracksProblem R = rec[0];
    tri_tracks_body(R, (int)blockIdx.x);
}
// batched: blockIdx.y = request, blockIdx.x = workgroup of 64 landmarks (the grid is as wide as the largest request)
__global__ __launch_bounds__(64) void k_tri_tracks_batch(const TriTracksProblem* __restrict__ probs) { BACKEND_PRIO();
    const TriTracksProblem R = probs[blockIdx.y];
    if ((int)blockIdx.x * 64 >= R.np) return;
    tri_tracks_body(R, (int)blockIdx.x);
}

hipError_t launch_tri_tracks(hipStream_t s, const TriTracksProblem* d_rec, int np) {
    if (np <= 0) return hipSuccess;
    if (!d_rec) return hipErrorInvalidValue;
    ProfScope ps(K_TRI_DLT, s);
    hipLaunchKernelGGL(k_tri_tracks, dim3((np + 63) / 64), dim3(64), 0, s, d_rec);
    return hipGetLastError();
}
hipError_t launch_tri_tracks_batch(hipStream_t s, const TriTracksProblem* d_probs, int n_probs, int max_np) {
    if (n_probs <= 0 || max_np <= 0) return hipSuccess;
    if (!d_probs) return hipErrorInvalidValue;
    ProfScope ps(K_TRI_DLT, s);
    hipLaunchKernelGGL(k_tri_tracks_batch, dim3((max_np + 63) / 64, n_probs), dim3(64), 0, s, d_probs);
    return hipGetLastError();
}

}  // namespace pmv
