// The sorting network of the one-workgroup selection kernels (k_gftt_pick_frame, k_track_select): 64-bit keys, descending, any n without
// padding, GF_T threads. The description of the stages stands above k_gftt_pick_frame (frontend.hip, step 2).
#pragma once
#include <hip/hip_runtime.h>

namespace pmv {

constexpr int GF_T = 1024;        // threads of a selection workgroup
__device__ __forceinline__ void gf_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
// comparator q of a stage whose comparators span 2 << lh keys: (i, i + half), or in a flip stage (i, mirror image of i in its block)
__device__ __forceinline__ void gf_cmpx(unsigned long long* keys, int n, int q, int lh, bool flip) {
    const int half = 1 << lh;
    const int i = ((q >> lh) << (lh + 1)) | (q & (half - 1));
    const int l = flip ? (i ^ (2 * half - 1)) : (i + half);
    if (l < n) {
        const unsigned long long a = keys[i], b = keys[l];
        if (a < b) { keys[i] = b; keys[l] = a; }
    }
}
template <bool ONCHIP> __device__ __forceinline__ void gf_sort(unsigned long long* keys, int n, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    int ln2 = 1;
    while ((1 << ln2) < n) ln2++;
    const int pairs = 1 << (ln2 - 1);
    for (int lk = 1; lk <= ln2; lk++) {              // merges of blocks of 2^lk keys: flip (lh = lk - 1), then lh = lk - 2 .. 0
        int lh = lk - 1;
        if (ONCHIP) {
            for (; lh >= 10; lh--) {                 // comparators that cross the 1024-key blocks
                for (int q = tid; q < pairs; q += GF_T) gf_cmpx(keys, n, q, lh, lh == lk - 1);
                __syncthreads();
            }
            for (int b = wave; b * 1024 < n; b += GF_T / 64) {   // block b, 512 comparators a stage, is wavefront b % 16's in every such stage
                for (int l2 = lh; l2 >= 0; l2--) {
#pragma unroll
                    for (int e = 0; e < 8; e++) gf_cmpx(keys, n, b * 512 + e * 64 + lane, l2, l2 == lk - 1);
                    gf_wave_sync();
                }
            }
            if (lk >= 10 || lk == ln2) __syncthreads();   // (merges below 1024 keys stay inside the blocks: nothing to wait for)
        } else {
            for (; lh >= 0; lh--) {
                for (int q = tid; q < pairs; q += GF_T) gf_cmpx(keys, n, q, lh, lh == lk - 1);
                __syncthreads();
            }
        }
    }
}

}  // namespace pmv
