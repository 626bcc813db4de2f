// The round structure of a whole adaptive RANSAC in ONE workgroup - cv::RANSACPointSetRegistrator::run as one kernel body - stated once for
// k_essential_ransac (backend_fivepoint.hip), k_fundamental_ransac (backend_fundamental.hip) and k_homography_ransac (backend_homography.hip),
// as cv's one registrator serves all three estimators.
// A round: thread 0 draws the next min(R, niters - iter) subsets from the request's MWC stream (getSubset: distinct indices, checkSubset, up
// to MAX_ATTEMPTS attempts each); the model's solver runs on the round's hypotheses; all waves score the round's (hypothesis, model) pairs
// with wave-reduced counts; thread 0 replays the registrator's bookkeeping in sample order - count > max(maxGood, S - 1), best model,
// maxGood, the niters update - and drops the speculative samples past niters. No host round trip per round, and a request is over when ITS
// loop is.
// What cv::PointSetRegistrator::Callback holds is the model policy M:
//   Problem            WholeProblem<double> or WholeProblem<float> (backend.h)
//   S, MODELS          points per sample, models per hypothesis at most
//   MAX_R              hypotheses per round at most (sizes WholeShared)
//   MAX_ATTEMPTS       of getSubset per sample
//   Extra              what the model's own steps keep in the shared block
//   direct(n)          cv's count == modelPoints branch: one solve without RANSAC
//   solve_direct       ... by thread 0 on the n points themselves: the first model into sh.best, true if there is one
//   subset_ok          checkSubset of the subset thread 0 has just drawn
//   solve              runKernel for the round's first nh subsets, called by every thread: models into the workspaces, their number into sh.nm
//   model(ws, R, b, mi, k)   element k of model mi of hypothesis b in the workspaces
//   error              computeError of one correspondence, as float32
//   finish             what the caller of the registrator does with the best model before it hands it out, called by every thread behind the
//                      mask: nothing for E and F, findHomography's refit on the inliers for H (it may replace sh.best)
#pragma once
#include "backend.h"
#include <float.h>

namespace pmv {

template <class M> struct WholeShared {
    double best[9];
    unsigned long long rng;
    int idx[M::MAX_R * M::S], nm[M::MAX_R], counts[M::MAX_R * M::MODELS];
    int iter, niters, max_good, drawn;
    int fail_at;   // the first sample of the round for which getSubset ran out of attempts (the round's length: none)
    typename M::Extra x;
};

// haveCollinearPoints on the last of a subset's S points (cv tests only that one): against every pair (j, k < j) of the earlier ones;
// q: the subset's points (x, y)
template <int S> __device__ inline bool whole_last_point_collinear(const float* q) {
    const float xi = q[2 * (S - 1)], yi = q[2 * (S - 1) + 1];
    #pragma unroll 1
    for (int j = 0; j < S - 1; j++) {
        const double dx1 = q[2 * j] - xi, dy1 = q[2 * j + 1] - yi;
        #pragma unroll 1
        for (int k = 0; k < j; k++) {
            const double dx2 = q[2 * k] - xi, dy2 = q[2 * k + 1] - yi;
            if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
        }
    }
    return false;
}

__device__ inline unsigned whole_rng_next(unsigned long long& st) { st = (unsigned long long)(unsigned)st * 4164903690U + (unsigned)(st >> 32); return (unsigned)st; }
// RANSACUpdateNumIters calls pow and log; the device's libm is not glibc's, so the host tabulates both per inlier count (WholeProblem::iters)
// and the kernel evaluates only the final expression: IEEE multiply, divide, compare, round-half-even.
__device__ inline int whole_update_iters(const double* __restrict__ tab, int good, int max_iters) {
    const double num = tab[0], denom = tab[1 + good];
    return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

// workspaces: the solver's LDS, in M's layout for R hypotheses; scoring_waves: the waves of the workgroup (all of them score)
template <class M> __device__ void whole_ransac(const typename M::Problem& P, double* workspaces, WholeShared<M>& sh, int R, int scoring_waves) {
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = P.n;
    if (tid == 0) { sh.iter = 0; sh.niters = P.max_iters; sh.max_good = 0; sh.drawn = 0; sh.rng = ~0ull; }
    __syncthreads();
    if (M::direct(n)) {   // the first model wins, every point is an inlier
        if (tid == 0 && M::solve_direct(P, workspaces, sh)) sh.max_good = n;
        __syncthreads();
    } else {
        for (;;) {
            const int iter = sh.iter, niters = sh.niters;   // (written by thread 0 before the barrier that ended the previous round)
            if (iter >= niters) break;
            const int nb = min(R, niters - iter);
            if (tid == 0) {
                unsigned long long st = sh.rng;
                int fail_at = nb;
                #pragma unroll 1
                for (int b = 0; b < nb; b++) {
                    int* idx = sh.idx + M::S * b;
                    int attempt = 0;
                    #pragma unroll 1
                    for (; attempt < M::MAX_ATTEMPTS; attempt++) {
                        #pragma unroll 1
                        for (int i = 0; i < M::S;) {
                            const int v = (int)(whole_rng_next(st) % (unsigned)n);
                            idx[i] = v;
                            int j = 0;
                            #pragma unroll 1
                            for (; j < i; j++) if (v == idx[j]) break;
                            if (j == i) i++;
                        }
                        if (M::subset_ok(P, idx, sh.x)) break;
                    }
                    if (attempt == M::MAX_ATTEMPTS) { fail_at = b; break; }
                }
                sh.rng = st; sh.fail_at = fail_at;
            }
            __syncthreads();
            const int nh = sh.fail_at;   // hypotheses to solve and score: the samples in front of a failed draw
            M::solve(P, workspaces, sh, R, nh);
            __syncthreads();
            #pragma unroll 1
            for (int p = wave; p < nh * M::MODELS; p += scoring_waves) {
                const int b = p / M::MODELS, mi = p - M::MODELS * b;
                if (mi >= sh.nm[b]) continue;   // (uniform over the wave)
                double m[9];
#pragma unroll
                for (int k = 0; k < 9; k++) m[k] = M::model(workspaces, R, b, mi, k);
                int good = 0;
                #pragma unroll 1
                for (int i = lane; i < n; i += 64) good += M::error(m, P.p1, P.p2, i) <= P.thr;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) good += __shfl_xor(good, o, 64);
                if (lane == 0) sh.counts[p] = good;
            }
            __syncthreads();
            if (tid == 0) {
                int it = iter, ni = niters, mg = sh.max_good;
                #pragma unroll 1
                for (int b = 0; b < nb && it < ni; b++, it++) {
                    if (b == nh) { ni = it; break; }   // getSubset failed for this sample: the loop ends here (at sample 0 without a model)
                    #pragma unroll 1
                    for (int mi = 0; mi < sh.nm[b]; mi++) {
                        const int c = sh.counts[M::MODELS * b + mi];
                        if (c > max(mg, M::S - 1)) {
                            #pragma unroll 1
                            for (int k = 0; k < 9; k++) sh.best[k] = M::model(workspaces, R, b, mi, k);
                            mg = c;
                            ni = whole_update_iters(P.iters, mg, ni);
                        }
                    }
                }
                sh.drawn += it - iter;
                sh.iter = it; sh.niters = ni; sh.max_good = mg;
            }
            __syncthreads();
        }
    }
    // result block: mask of the loop's best model (err <= thr, recomputed once), the model as M::finish leaves it, found, samples drawn, best
    // count. The request's sequence number is the workgroup's last store, behind a system fence and a barrier: its caller waits for that word
    // alone and reads the block and reuses the request's buffers as soon as it sees it.
    const bool found = sh.max_good > 0;
    uint8_t* mask = (uint8_t*)(P.out + ESS_OUT_HDR);
    if (found && !M::direct(n)) {
        double m[9];
#pragma unroll
        for (int k = 0; k < 9; k++) m[k] = sh.best[k];
        #pragma unroll 1
        for (int i = tid; i < n; i += (int)blockDim.x) mask[i] = (uint8_t)(M::error(m, P.p1, P.p2, i) <= P.thr);
    } else {
        #pragma unroll 1
        for (int i = tid; i < n; i += (int)blockDim.x) mask[i] = found ? 1 : 0;
    }
    M::finish(P, workspaces, sh);
    if (tid == 0) {
        double* Mo = (double*)P.out;
        #pragma unroll 1
        for (int k = 0; k < 9; k++) Mo[k] = found ? sh.best[k] : 0.0;
        int* info = (int*)(P.out + ESS_OUT_INFO);
        info[0] = found ? 1 : 0; info[1] = sh.drawn; info[2] = sh.max_good;
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store((unsigned*)(P.out + ESS_OUT_DONE), P.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace pmv
