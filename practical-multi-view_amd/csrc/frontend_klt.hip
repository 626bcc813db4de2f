// pmv_klt_*: a KLT tracker that lives in the context (contract: include/pmv_hip.h). The track list (id, age, position) stays in device memory
// from frame to frame; pmv_klt_step enqueues the whole per-frame chain on the front-end stream - forward-backward LK, filter, rejectWithF,
// setMask thinning, masked detection, sub-pixel refinement, append - and waits once (twice with rejectWithF: the host needs n1 for libm's
// iteration table). The existing kernels run as they are, on the tracker's device buffers; the three kernels here are the glue that the
// host did between the single calls: each is ONE 1024-thread workgroup that compacts a list in order (wave ballots, a prefix over the
// wavefronts in LDS, chunks of 1024 tracks) and leaves its count in device memory, where the launches behind it read it - the n of the
// refill record, the cap of the selection pass, the point count of the sub-pixel launch. Every count read from device memory is clamped to
// its buffer's capacity before it bounds a loop.
// pmv_klt_step_many steps a group of trackers through ONE such chain: the same three bodies as a grid over the trackers (blockIdx.x selects a
// per-tracker argument record in device memory), LK as one batched launch whose records k_klt_lk_records writes from the trackers' states,
// and the multi-request forms of the refill, frame and F launches. pmv_klt_step keeps its own argument form: a group of one is ~25 us slower
// (DESIGN.md §4). What the stage kernels of a tracker are given is described ONCE, by klt_stage_args: it fills a KltManyRec from the tracker
// and from where its parts of the per-launch tables live (KltShares); the many-call stores that record in its block, the single step passes
// the record's members as kernel arguments. klt_launch, klt_f_problem, klt_result_check, klt_result_copy and klt_book are shared too.
// pmv_klt_step_stereo / pmv_klt_step_many_stereo append a stage 8 behind the append and in front of the final wait: LK from the current left
// into the right frame for the list the step returns, in a launch sized by the bound (target) whose workgroups read the list's length from
// device memory, then one workgroup per tracker that applies stage 2's rule to the result and ends the chain with its own completion word.
// A tracker with an observation setting (pmv_klt_set_observe) gets a stage 9 behind that: one workgroup per tracker lifts the list the step
// returns onto the normalised image plane (lift_point, pmv_lift.h), forms the velocities and lifts the right observations of a stereo call,
// and ends the chain with a third completion word; with undistorted_f one more launch, enqueued under the wait for n1, writes stage 3's two
// point sets as virtual-camera points into the LK result arrays of stage 1, which are free by then. A step with the setting off makes
// neither launch and reads none of this.
// A tracker with a pending prediction (pmv_klt_set_prediction) runs stage 1 from projected guesses: one workgroup per tracker joins the
// state's ids against the prediction list (sorted once on the host; a binary search per track), projects the hits (project_point,
// pmv_lift.h) and zeroes the tracker's success word - k_klt_predict in a single step, folded into k_klt_lk_records in a group; LK then runs
// from the guesses on the capped levels and counts its forward successes into that word, and a second LK launch of the same size, whose
// workgroups read the word first and leave at once when the predicted pass had successes enough, is the fall-back to the full pyramid. Two
// launches more in a single step, one more in a group, no wait more; a call without a pending prediction launches what it launched before.
#include "pmv_ctx.h"
#include "pmv_lift.h"
#include "backend.h"
#include "vo_pipeline.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace pmv {

namespace {

constexpr int KT = 1024, KW = KT / 64;
// counts of a step in device memory: n0, n1, n2, n3, corners wanted (target - n3), corners found (k_gftt_pick_frame's count), its two statistics
// (C_NOUT: the length of the list after the append, left only by a stereo step - stage 8 reads it)
// (C_JOINED, C_SUCC, C_MINSUCC: a predicted step - tracks that got a projected guess, and the (successes, successes wanted) pair of its LK launches)
enum { C_N0 = 0, C_N1, C_N2, C_N3, C_WANT, C_M, C_STAT0, C_STAT1, C_NOUT, C_JOINED, C_SUCC, C_MINSUCC, C_COUNT = 16 };

struct KltList { int* id; int* age; float* prev; float* cur; };                     // a track list on its way through the chain
struct KltRefillIn { unsigned* pos; int* prio; uint8_t* flag; RefillRec* rec; };    // what k_track_select reads (pos null: not written)

// Stable compaction of the items i < n with pred(i), by the whole workgroup: emit(i, o) is called once per survivor with its place o.
// Returns the number of survivors (in every thread). n is uniform over the workgroup; s_w: KW words of LDS.
template <class Pred, class Emit>
__device__ __forceinline__ int klt_compact(int n, unsigned* s_w, Pred pred, Emit emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int done = 0;
    for (int base = 0; base < n; base += KT) {
        const int i = base + tid;
        const bool p = i < n && pred(i);
        const unsigned long long bal = __ballot(p);
        if (lane == 0) s_w[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w2 = 0; w2 < KW; w2++) { const int c = (int)s_w[w2]; off += w2 < wave ? c : 0; tot += c; }
        if (p) emit(i, done + off + __popcll(bal & ((1ull << lane) - 1ull)));
        __syncthreads();   // (the next chunk rewrites the wavefronts' counts)
        done += tot;
    }
    return done;
}
// the rounded position as k_track_select takes it: cvRound (half to even); the track passed the border test, so it lies inside the frame
__device__ __forceinline__ void klt_refill_in(const KltRefillIn& rf, int o, float x, float y) {
    rf.pos[o] = ((unsigned)__float2int_rn(y) << 16) | (unsigned)__float2int_rn(x);
    rf.prio[o] = 0;
    rf.flag[o] = 1;
}
__device__ __forceinline__ int klt_clamp(int v, int hi) { return v < 0 ? 0 : (v < hi ? v : hi); }

// Stage 2: the status bytes, the forward-backward distance and inBorder, then the compaction of (id, age + 1, prev xy, cur xy). n1 goes to
// the counts, to the refill record (a chain without rejectWithF goes on with k_track_select) and to the host's word in mapped pinned memory.
struct KltFilterArgs {
    int n0, fb, border, w, h;
    float thr2;
    const int* id; const int* age; const float* prev; const float* fwd; const float* back; const uint8_t* st; const uint8_t* bst;
    KltList out; KltRefillIn rf;
    int* cnt; int* h_n1;
};
// The rule of stages 2 and 8 for track i of A (KltFilterArgs or KltStereoArgs: fb, border, w, h, thr2, prev, fwd, back, st, bst): LK's status
// bytes, the round trip back to `prev` within thr2, the forward position inside the border.
template <class Args>
__device__ __forceinline__ bool klt_track_ok(const Args& A, int i) {
    const float lo = (float)A.border, hx = (float)(A.w - A.border), hy = (float)(A.h - A.border);
    bool ok = A.st[i] == 1;
    if (A.fb) {
        const float dx = __fsub_rn(A.back[2 * i], A.prev[2 * i]), dy = __fsub_rn(A.back[2 * i + 1], A.prev[2 * i + 1]);
        ok = ok && A.bst[i] == 1 && __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) <= A.thr2;
    }
    // rintf: half to even; the comparison in float is lrintf's in int for every finite value, and a NaN fails it
    const float rx = rintf(A.fwd[2 * i]), ry = rintf(A.fwd[2 * i + 1]);
    return ok && rx >= lo && rx < hx && ry >= lo && ry < hy;
}
__device__ __forceinline__ void klt_filter(const KltFilterArgs& A, unsigned* s_w) {
    const int n1 = klt_compact(A.n0, s_w,
        [&](int i) { return klt_track_ok(A, i); },
        [&](int i, int o) {
            const float x = A.fwd[2 * i], y = A.fwd[2 * i + 1];
            A.out.id[o] = A.id[i]; A.out.age[o] = A.age[i] + 1;
            A.out.prev[2 * o] = A.prev[2 * i]; A.out.prev[2 * o + 1] = A.prev[2 * i + 1];
            A.out.cur[2 * o] = x; A.out.cur[2 * o + 1] = y;
            klt_refill_in(A.rf, o, x, y);
        });
    if (threadIdx.x == 0) {
        A.cnt[C_N0] = A.n0; A.cnt[C_N1] = n1; A.cnt[C_N2] = n1;
        A.rf.rec->n = n1;
        *A.h_n1 = n1;
        __threadfence_system();
    }
}
__global__ __launch_bounds__(KT) void k_klt_filter(KltFilterArgs A) {
    __shared__ unsigned s_w[KW];
    BACKEND_PRIO();
    klt_filter(A, s_w);
}

// Stages 3 and 4: the same compaction driven by a byte mask - the F mask (then it also writes what k_track_select reads and the n of the
// refill record) or the keep bytes (then it leaves the number of corners wanted, target - n3, for the selection pass).
struct KltCompactArgs {
    KltList in, out;
    const uint8_t* mask; const int* n_in;
    int cap, cnt_out, target;       // cnt_out: the count's place (C_N2 or C_N3); target > 0: *want is written too
    KltRefillIn rf;
    int* cnt; int* want;            // want: the selection pass's word of this tracker (the step's own C_WANT, or the group's table)
};
// PASS (a group's rejectWithF stage): a null mask keeps every track - the tracker has no F stage in this call and its list goes through
template <bool PASS>
__device__ __forceinline__ void klt_compact_by(const KltCompactArgs& A, unsigned* s_w) {
    const int n = klt_clamp(*A.n_in, A.cap);
    const int no = klt_compact(n, s_w,
        [&](int i) { return (PASS && !A.mask) || A.mask[i] != 0; },
        [&](int i, int o) {
            const float x = A.in.cur[2 * i], y = A.in.cur[2 * i + 1];
            A.out.id[o] = A.in.id[i]; A.out.age[o] = A.in.age[i];
            A.out.prev[2 * o] = A.in.prev[2 * i]; A.out.prev[2 * o + 1] = A.in.prev[2 * i + 1];
            A.out.cur[2 * o] = x; A.out.cur[2 * o + 1] = y;
            if (A.rf.pos) klt_refill_in(A.rf, o, x, y);
        });
    if (threadIdx.x == 0) {
        A.cnt[A.cnt_out] = no;
        if (A.rf.pos) A.rf.rec->n = no;
        if (A.target > 0) *A.want = klt_clamp(A.target - no, A.target);
    }
}
__global__ __launch_bounds__(KT) void k_klt_compact(KltCompactArgs A) {
    __shared__ unsigned s_w[KW];
    BACKEND_PRIO();
    klt_compact_by<false>(A, s_w);
}

// Stage 7: survivors, then the m new tracks in detector order (ids next_id .., age 1, prev = their own position), into the state and into
// the result block in mapped pinned memory; the completion word is the last store.
struct KltAppendArgs {
    KltList in;
    const int* cnt; const int* m; const int* ixy; const float* sp_xy; const int* f_info;   // m: the selection pass's count; sp_xy: the refined corners or null; f_info: (found, drawn) or null
    int n0, next_id, target;
    unsigned seq;
    int* s_id; int* s_age; float* s_xy;
    int* r_hdr; int* r_id; int* r_age; float* r_xy; float* r_prev;
    int* n_out;                     // a stereo step: the device's copy of n3 + m (C_NOUT), else null
    const int* joined; const int* pred;   // a predicted step: C_JOINED and the (successes, wanted) pair of stage 1, else null
};
__device__ __forceinline__ void klt_append(const KltAppendArgs& A) {
    const int tid = threadIdx.x;
    const int n3 = klt_clamp(A.cnt[C_N3], A.target), m = klt_clamp(*A.m, A.target - n3);
    for (int i = tid; i < n3; i += KT) {
        const int id = A.in.id[i], age = A.in.age[i];
        const float x = A.in.cur[2 * i], y = A.in.cur[2 * i + 1];
        A.s_id[i] = id; A.s_age[i] = age; A.s_xy[2 * i] = x; A.s_xy[2 * i + 1] = y;
        A.r_id[i] = id; A.r_age[i] = age; A.r_xy[2 * i] = x; A.r_xy[2 * i + 1] = y;
        A.r_prev[2 * i] = A.in.prev[2 * i]; A.r_prev[2 * i + 1] = A.in.prev[2 * i + 1];
    }
    for (int j = tid; j < m; j += KT) {
        const int o = n3 + j, id = A.next_id + j;
        const float x = A.sp_xy ? A.sp_xy[2 * j] : (float)A.ixy[2 * j], y = A.sp_xy ? A.sp_xy[2 * j + 1] : (float)A.ixy[2 * j + 1];
        A.s_id[o] = id; A.s_age[o] = 1; A.s_xy[2 * o] = x; A.s_xy[2 * o + 1] = y;
        A.r_id[o] = id; A.r_age[o] = 1; A.r_xy[2 * o] = x; A.r_xy[2 * o + 1] = y;
        A.r_prev[2 * o] = x; A.r_prev[2 * o + 1] = y;
    }
    if (tid == 0) {
        A.r_hdr[0] = A.n0; A.r_hdr[1] = A.cnt[C_N1]; A.r_hdr[2] = A.cnt[C_N2]; A.r_hdr[3] = n3; A.r_hdr[4] = m;
        A.r_hdr[5] = A.f_info ? A.f_info[0] : -1; A.r_hdr[6] = A.f_info ? A.f_info[1] : 0; A.r_hdr[7] = 0;
        A.r_hdr[8] = n3 + m;
        A.r_hdr[12] = A.pred ? *A.joined : 0; A.r_hdr[13] = A.pred ? A.pred[0] : 0; A.r_hdr[14] = A.pred && A.pred[0] < A.pred[1] ? 1 : 0;
        if (A.n_out) *A.n_out = n3 + m;
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store((unsigned*)(A.r_hdr + 9), A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ __launch_bounds__(KT) void k_klt_append(KltAppendArgs A) {
    BACKEND_PRIO();
    klt_append(A);
}

// Stage 8 (pmv_klt_step_stereo): LK took the list after the append from the current left frame into the right frame (prev = the left
// positions, which are the state; fwd / back / st / bst = that launch's results, indexed like the list). The rule is stage 2's, with the
// stereo setting's threshold and border; right xy and status go to the result block for every track of the list, the number of matched
// tracks to counts8[7], and the stereo completion word (header word 10) is the last store of the chain. on = 0: the tracker has no right
// frame in this call (a many-call) - only the count, 0, and the word are written.
struct KltStereoArgs {
    const int* n;                   // the append's C_NOUT
    int cap, on, fb, border, w, h;
    float thr2;
    const float* prev; const float* fwd; const float* back; const uint8_t* st; const uint8_t* bst;
    unsigned seq;
    int* r_hdr; float* r_rxy; uint8_t* r_rst;
};
__device__ __forceinline__ void klt_stereo(const KltStereoArgs& A, unsigned* s_w) {
    int matched = 0;
    if (A.on) {
        const int n = klt_clamp(*A.n, A.cap);
        matched = klt_compact(n, s_w,
            [&](int i) {   // (called once per track: the outputs of the unmatched tracks are written here too)
                const bool ok = klt_track_ok(A, i);
                A.r_rxy[2 * i] = A.fwd[2 * i]; A.r_rxy[2 * i + 1] = A.fwd[2 * i + 1];
                A.r_rst[i] = ok ? 1 : 0;
                return ok;
            },
            [](int, int) {});
    }
    if (threadIdx.x == 0) A.r_hdr[7] = matched;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store((unsigned*)(A.r_hdr + 10), A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ __launch_bounds__(KT) void k_klt_stereo(KltStereoArgs A) {
    __shared__ unsigned s_w[KW];
    BACKEND_PRIO();
    klt_stereo(A, s_w);
}

// Stage 9 (pmv_klt_set_observe): the list after the append - ages and xy are the state, the previous position of a survivor lies in the list
// the append read, a new track (age 1, at and beyond n3) has none - lifted through the tracker's camera; the velocity is the float32 difference of
// the two rounded lifts over dt, divided in double. right: a stereo call whose tracker has a right camera and a right frame - stage 8's
// positions (S.fwd) are lifted through the right camera and stage 8's rule is asked again for the status. Everything goes to the result
// block; the observe completion word (header word 11) is the last store of the chain.
struct KltObserveArgs {
    int on, cap, right;
    const int* cnt;                 // C_N3 and the append's C_NOUT
    const int* age; const float* xy; const float* prev;
    const LiftCam* cam; const LiftCam* rcam;
    double dt;
    unsigned seq;
    int* r_hdr; float* r_un; float* r_vel; uint8_t* r_ok; float* r_run; uint8_t* r_rok;
};
__device__ __forceinline__ void klt_observe(const KltObserveArgs& A, const KltStereoArgs& S) {
    const int n = klt_clamp(A.cnt[C_NOUT], A.cap), n3 = klt_clamp(A.cnt[C_N3], n);
    const LiftCam cam = *A.cam;
    for (int i = threadIdx.x; i < n; i += KT) {
        float ux, uy, vx = 0.f, vy = 0.f;
        const bool ok = lift_point_f(cam, A.xy[2 * i], A.xy[2 * i + 1], &ux, &uy);
        if (i < n3 && A.age[i] > 1 && ok) {
            float px, py;
            if (lift_point_f(cam, A.prev[2 * i], A.prev[2 * i + 1], &px, &py)) {
                vx = (float)((double)__fsub_rn(ux, px) / A.dt); vy = (float)((double)__fsub_rn(uy, py) / A.dt);
            }
        }
        A.r_un[2 * i] = ux; A.r_un[2 * i + 1] = uy; A.r_ok[i] = ok ? 1 : 0;
        A.r_vel[2 * i] = vx; A.r_vel[2 * i + 1] = vy;
    }
    if (A.right) {
        const LiftCam rcam = *A.rcam;
        for (int i = threadIdx.x; i < n; i += KT) {
            float rx, ry;
            const bool rok = lift_point_f(rcam, S.fwd[2 * i], S.fwd[2 * i + 1], &rx, &ry);
            A.r_run[2 * i] = rx; A.r_run[2 * i + 1] = ry;
            A.r_rok[i] = klt_track_ok(S, i) && rok ? 1 : 0;
        }
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store((unsigned*)(A.r_hdr + 11), A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ __launch_bounds__(KT) void k_klt_observe(KltObserveArgs A, KltStereoArgs S) {
    BACKEND_PRIO();
    klt_observe(A, S);
}

// Stage 3 on undistorted points (the observation setting's undistorted_f): for the n1 survivors the filter left in list 0, previous and
// current position as points of the virtual camera, q = ((float)(f xd + w / 2), (float)(f yd + h / 2)) of the lift's doubles (product and
// sum separate double operations; hw = w / 2.0, hh = h / 2.0 from the host); a track with a lift that is not finite gets (0, 0) twice. One
// lane per survivor; the launch is sized by n0 (= cap, which also bounds p1 and p2) and reads n1 from the counts.
struct KltLiftFArgs {
    int on, cap;
    const int* n1;
    const float* prev; const float* cur;
    const LiftCam* cam;
    double f, hw, hh;
    float* p1; float* p2;
};
__device__ __forceinline__ void klt_lift_f(const KltLiftFArgs& A, int chunk) {
    const int n1 = klt_clamp(*A.n1, A.cap), i = chunk * KT + (int)threadIdx.x;
    if (i >= n1) return;
    const LiftCam cam = *A.cam;
    double ax, ay, bx, by;
    const bool oka = lift_point(cam, A.prev[2 * i], A.prev[2 * i + 1], &ax, &ay), okb = lift_point(cam, A.cur[2 * i], A.cur[2 * i + 1], &bx, &by);
    const bool ok = oka && okb;
    A.p1[2 * i] = ok ? (float)(A.f * ax + A.hw) : 0.f; A.p1[2 * i + 1] = ok ? (float)(A.f * ay + A.hh) : 0.f;
    A.p2[2 * i] = ok ? (float)(A.f * bx + A.hw) : 0.f; A.p2[2 * i + 1] = ok ? (float)(A.f * by + A.hh) : 0.f;
}
__global__ __launch_bounds__(KT) void k_klt_lift_f(KltLiftFArgs A) {
    BACKEND_PRIO();
    klt_lift_f(A, blockIdx.x);
}

// Stage 1 of a predicted step (pmv_klt_set_prediction): the guess of state track i < n0 is the projection of the prediction point with the
// track's id, where the list (n_list entries, ids ascending) has one and project_point accepts it, else the track's own position. emit(i,
// gx, gy) takes it: the initial-flow array of the single step, the LK record of a group. The workgroup leaves the number of projected guesses
// in *joined and arms the pair of the LK launches: no success yet, min_succ wanted. n0 and n_list are the host's.
struct KltPredictArgs {
    int on, n_list, top, back_top, min_succ, slot;   // slot: the tracker's pair in a group's table (0 in a single step)
    const int* ids; const double* xyz; const LiftCam* cam;
    int* pred; int* joined;
    float* guess;                   // a single step: 2 n0 floats
};
template <class Emit>
__device__ __forceinline__ void klt_predict(const KltPredictArgs& P, int n0, const int* __restrict__ id, const float* __restrict__ xy, unsigned* s_w, Emit emit) {
    const LiftCam cam = *P.cam;
    if (threadIdx.x == 0) s_w[0] = 0u;
    __syncthreads();
    unsigned mine = 0;
    for (int i = threadIdx.x; i < n0; i += KT) {
        float gx = xy[2 * i], gy = xy[2 * i + 1];
        const int want = id[i];
        int lo = 0, hi = P.n_list;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.ids[mid] < want) lo = mid + 1; else hi = mid; }
        if (lo < P.n_list && P.ids[lo] == want) {
            float u, v;
            if (project_point(cam, P.xyz[3 * lo], P.xyz[3 * lo + 1], P.xyz[3 * lo + 2], &u, &v)) { gx = u; gy = v; mine++; }
        }
        emit(i, gx, gy);
    }
    if (mine) atomicAdd(&s_w[0], mine);
    __syncthreads();
    if (threadIdx.x == 0) { *P.joined = (int)s_w[0]; P.pred[0] = 0; P.pred[1] = P.min_succ; }
    __syncthreads();   // (s_w is the caller's again)
}
__global__ __launch_bounds__(KT) void k_klt_predict(KltPredictArgs P, int n0, const int* __restrict__ id, const float* __restrict__ xy) {
    __shared__ unsigned s_w[KW];
    BACKEND_PRIO();
    klt_predict(P, n0, id, xy, s_w, [&](int i, float gx, float gy) { P.guess[2 * i] = gx; P.guess[2 * i + 1] = gy; });
}

// ---- pmv_klt_step_many: the same three stages as a grid over the trackers of a group ----------------------------------------------------
// blockIdx.x selects the tracker's argument record in device memory, which holds what the Klt*Args hold; one workgroup serves one tracker and
// no workgroup waits for another. What the host learns only after the first wait does not change the records: `cur` (which of the two lists
// holds the group's tracks: 1 once a rejectWithF stage has been launched for the group) is a launch argument, and f_run (one word per
// tracker, null when the group made no F launch) says whose F stage ran.
struct KltManyRec {
    KltFilterArgs filter;
    KltCompactArgs by_f, by_keep;    // in / out: set by the kernel from lst[cur], lst[cur ^ 1]
    KltAppendArgs append;            // in: lst[cur]; f_info: set by the kernel
    KltList lst[2];
    const int* f_info;               // (found, drawn) of the tracker's F result block
    unsigned long long prev_off, next_off;   // byte offsets of the tracker's two frame slots
    int lk_base, lk_flags;           // first index of the tracker's share of the launch's LK records and results; LKX_FB or 0
    // a stereo many-call (stereo.on): stage 8's arguments, the right frame slot, and the tracker's share of stage 8's one LK launch - `cap`
    // records from st_base on, sized by the bound since the count is the device's
    KltStereoArgs stereo;
    unsigned long long right_off;
    int st_base, st_flags;
    // a tracker with an observation setting (observe.on): stage 9's arguments (prev: set by the kernel from lst[cur]) and, with
    // undistorted_f in a call that may run the tracker's F stage (lift_f.on), those of the lift in front of stage 3
    KltObserveArgs observe;
    KltLiftFArgs lift_f;
    // a tracker with a pending prediction and tracks (predict.on): what k_klt_lk_records joins and projects for its share of the records
    KltPredictArgs predict;
};
// LK's records for the whole group, written where the tracks are: block lk_base + i tracks state position i of its tracker (geometry entry 0
// of the call's own one-entry table). The host sized the shares from the n0 it holds; `total` = their sum bounds every store.
// ext2 (a call in which a tracker has a pending prediction, else null): the records of the fall-back launch over the same blocks - void for a
// tracker without a prediction, gated by the tracker's pair for one with; the first launch's records of such a tracker start at the guesses
// on the capped levels and count.
__global__ __launch_bounds__(KT) void k_klt_lk_records(const KltManyRec* __restrict__ recs, LKBlock* __restrict__ blocks, LKExt* __restrict__ ext, LKExt* __restrict__ ext2,
                                                       int total) {
    __shared__ unsigned s_w[KW];
    BACKEND_PRIO();
    const KltManyRec& R = recs[blockIdx.x];
    const int base = R.lk_base, n0 = klt_clamp(R.filter.n0, total - base);
    const float* __restrict__ xy = R.filter.prev;
    auto block_of = [&](int i) {
        LKBlock b;
        b.prev_off = R.prev_off; b.next_off = R.next_off; b.x = xy[2 * i]; b.y = xy[2 * i + 1]; b.track = base + i; b.geom = 0;
        blocks[base + i] = b;
    };
    if (R.predict.on && ext2) {   // workgroup-uniform
        const KltPredictArgs P = R.predict;
        klt_predict(P, n0, R.filter.id, xy, s_w, [&](int i, float gx, float gy) {
            block_of(i);
            ext[base + i] = LKExt{gx, gy, R.lk_flags | LKX_INIT, lkext_opt(P.top, P.back_top, P.slot, LKP_COUNT)};
            ext2[base + i] = LKExt{0.f, 0.f, R.lk_flags, lkext_opt(-1, P.back_top, P.slot, LKP_GATE)};
        });
        return;
    }
    for (int i = threadIdx.x; i < n0; i += KT) {
        block_of(i);
        ext[base + i] = LKExt{0.f, 0.f, R.lk_flags, 0};
        if (ext2) ext2[base + i] = LKExt{0.f, 0.f, LKX_VOID, 0};
    }
}
// Stage 8's records: block st_base + i tracks position i of the tracker's list after the append, from its current left frame into its right
// frame; the records at and beyond the list's count (C_NOUT) are void. `total` = the sum of the shares bounds every store.
__global__ __launch_bounds__(KT) void k_klt_stereo_records(const KltManyRec* __restrict__ recs, LKBlock* __restrict__ blocks, LKExt* __restrict__ ext, int total) {
    BACKEND_PRIO();
    const KltManyRec& R = recs[blockIdx.x];
    if (!R.stereo.on) return;
    const int base = R.st_base, share = klt_clamp(R.stereo.cap, total - base), n = klt_clamp(*R.stereo.n, share);
    const float* __restrict__ xy = R.stereo.prev;
    for (int i = threadIdx.x; i < share; i += KT) {
        LKBlock b;
        b.prev_off = R.next_off; b.next_off = R.right_off; b.track = base + i; b.geom = 0;
        b.x = i < n ? xy[2 * i] : 0.f; b.y = i < n ? xy[2 * i + 1] : 0.f;
        blocks[base + i] = b;
        ext[base + i] = LKExt{0.f, 0.f, i < n ? R.st_flags : LKX_VOID, 0};
    }
}
__global__ __launch_bounds__(KT) void k_klt_stereo_many(const KltManyRec* __restrict__ recs) {
    __shared__ unsigned s_w[KW];
    BACKEND_PRIO();
    const KltStereoArgs A = recs[blockIdx.x].stereo;
    klt_stereo(A, s_w);
}
// gx workgroups per tracker: workgroup b serves chunk b % gx of tracker b / gx
__global__ __launch_bounds__(KT) void k_klt_lift_f_many(const KltManyRec* __restrict__ recs, int gx) {
    BACKEND_PRIO();
    const KltLiftFArgs A = recs[blockIdx.x / gx].lift_f;
    if (!A.on) return;
    klt_lift_f(A, blockIdx.x % gx);
}
__global__ __launch_bounds__(KT) void k_klt_observe_many(const KltManyRec* __restrict__ recs, int cur) {
    BACKEND_PRIO();
    const KltManyRec& R = recs[blockIdx.x];
    KltObserveArgs A = R.observe;
    if (!A.on) return;
    A.prev = R.lst[cur & 1].prev;
    const KltStereoArgs S = R.stereo;
    klt_observe(A, S);
}
__global__ __launch_bounds__(KT) void k_klt_filter_many(const KltManyRec* __restrict__ recs) {
    __shared__ unsigned s_w[KW];
    BACKEND_PRIO();
    const KltFilterArgs A = recs[blockIdx.x].filter;
    klt_filter(A, s_w);
}
__global__ __launch_bounds__(KT) void k_klt_compact_many(const KltManyRec* __restrict__ recs, int by_keep, int cur, const int* __restrict__ f_run) {
    __shared__ unsigned s_w[KW];
    BACKEND_PRIO();
    const KltManyRec& R = recs[blockIdx.x];
    KltCompactArgs A = by_keep ? R.by_keep : R.by_f;
    A.in = R.lst[cur & 1]; A.out = R.lst[(cur & 1) ^ 1];
    if (!by_keep && !f_run[blockIdx.x]) A.mask = nullptr;
    klt_compact_by<true>(A, s_w);
}
__global__ __launch_bounds__(KT) void k_klt_append_many(const KltManyRec* __restrict__ recs, int cur, const int* __restrict__ f_run) {
    BACKEND_PRIO();
    const KltManyRec& R = recs[blockIdx.x];
    KltAppendArgs A = R.append;
    A.in = R.lst[cur & 1];
    A.f_info = f_run && f_run[blockIdx.x] ? R.f_info : nullptr;
    klt_append(A);
}

// ---- the tracker's blocks, each described once ---------------------------------------------------------------------------------------
// device block: state | identity order | LK results | the two lists of the chain | refill tables | F result | counts | corners | refined corners
struct KltDev {
    Carved<int> s_id, s_age; Carved<float> s_xy;
    Carved<int> order;
    Carved<float> lk_xy, lk_err, bk_xy, bk_err; Carved<uint8_t> lk_st, bk_st;
    Carved<int> l_id[2], l_age[2]; Carved<float> l_prev[2], l_cur[2];
    Carved<unsigned> pos; Carved<int> prio; Carved<uint8_t> flag, keep;
    Carved<char> f_out;
    Carved<int> cnt, ixy;
    Carved<float> sp_xy; Carved<uint8_t> sp_it, sp_fl;
    Carved<float> pr_guess;         // the initial flow of a predicted single step
};
KltDev klt_dev_block(Carve& c, size_t cap) {
    KltDev D;
    const size_t cp = refill_pad((int)cap), c8 = (cap + 7) / 8 * 8;
    D.s_id = c.take<int>(cap, 16); D.s_age = c.take<int>(cap, 16); D.s_xy = c.take<float>(2 * cap, 16);
    D.order = c.take<int>(c8, 16);
    D.lk_xy = c.take<float>(2 * cap, 16); D.lk_err = c.take<float>(cap, 16); D.bk_xy = c.take<float>(2 * cap, 16); D.bk_err = c.take<float>(cap, 16);
    D.lk_st = c.take<uint8_t>(cap, 16); D.bk_st = c.take<uint8_t>(cap, 16);
    for (int k = 0; k < 2; k++) {
        D.l_id[k] = c.take<int>(cap, 16); D.l_age[k] = c.take<int>(cap, 16); D.l_prev[k] = c.take<float>(2 * cap, 16); D.l_cur[k] = c.take<float>(2 * cap, 16);
    }
    D.pos = c.take<unsigned>(cp, 16); D.prio = c.take<int>(cp, 16); D.flag = c.take<uint8_t>(cp, 16); D.keep = c.take<uint8_t>(cp, 16);
    D.f_out = c.take<char>(ESS_OUT_HDR + cap, 64);
    D.cnt = c.take<int>(C_COUNT, 64); D.ixy = c.take<int>(2 * cap, 16);
    D.sp_xy = c.take<float>(2 * cap, 16); D.sp_it = c.take<uint8_t>(cap, 16); D.sp_fl = c.take<uint8_t>(cap, 16);
    D.pr_guess = c.take<float>(2 * cap, 16);
    return D;
}
// the prediction list of a tracker in device memory: [n ids, ascending | their n points, 3 doubles each, 16-byte aligned]
inline size_t klt_pr_xyz_off(size_t n) { return (n * sizeof(int) + 15) & ~(size_t)15; }
// record block, pinned mirror and device copy: refill record | half-width table | frame request || F problem | F iteration table. The
// front part goes up with every step, the part behind `front` only in front of a k_fundamental_ransac launch.
struct KltRecs { Carved<RefillRec> rrec; Carved<uint8_t> hw; Carved<int> grec; size_t front; Carved<char> fprob; Carved<double> ftab; };
KltRecs klt_rec_block(Carve& c, size_t cap) {
    KltRecs R;
    R.rrec = c.take<RefillRec>(1, 16); R.hw = c.take<uint8_t>(REFILL_HW, 16); R.grec = c.take<int>(CELL_STRIDE, 16);
    c.skip_to(64);
    R.front = c.bytes();
    R.fprob = c.take<char>(ESS_HDR, 64); R.ftab = c.take<double>(cap + 2, 16);
    return R;
}
// result block (mapped pinned): n1's word | header (counts8, out_n, completion word, stereo completion word, observe completion word) | ids |
// ages | xy | prev xy | right xy | right status (the last two are written by stereo steps only) | normalised xy | velocities | lift ok |
// normalised right xy | right observation ok (the last five are written by stage 9 only, the last two of them in stereo calls only; a
// tracker in a group has the same block: the group keeps no result block of its own)
struct KltRes {
    Carved<int> n1, hdr, id, age; Carved<float> xy, prev, right_xy; Carved<uint8_t> right_st;
    Carved<float> un_xy, vel; Carved<uint8_t> un_ok; Carved<float> right_un; Carved<uint8_t> right_un_ok;
};
KltRes klt_res_block(Carve& c, size_t cap) {
    KltRes R;
    R.n1 = c.take<int>(16, 64); R.hdr = c.take<int>(16, 64);
    R.id = c.take<int>(cap, 16); R.age = c.take<int>(cap, 16); R.xy = c.take<float>(2 * cap, 16); R.prev = c.take<float>(2 * cap, 16);
    R.right_xy = c.take<float>(2 * cap, 16); R.right_st = c.take<uint8_t>(cap, 16);
    R.un_xy = c.take<float>(2 * cap, 16); R.vel = c.take<float>(2 * cap, 16); R.un_ok = c.take<uint8_t>(cap, 16);
    R.right_un = c.take<float>(2 * cap, 16); R.right_un_ok = c.take<uint8_t>(cap, 16);
    return R;
}

}  // namespace

struct KltTracker {
    pmv_klt_params p;
    int cap = 0, n = 0, next_id = 0;
    unsigned seq = 0;
    float thr2 = 0.f;
    bool st_on = false;             // pmv_klt_set_stereo: the setting of stage 8 and its thr2
    pmv_klt_stereo_params st{};
    float st_thr2 = 0.f;
    bool obs_on = false;            // pmv_klt_set_observe: the setting of stage 9 and the device table entries of its cameras
    pmv_klt_observe_params obs{};
    const LiftCam* obs_cam = nullptr; const LiftCam* obs_rcam = nullptr;
    // what pmv_klt_get_observations finds: 0 no step since pmv_klt_create / pmv_klt_set_tracks, 1 the last step ran with the setting off,
    // 2 with it on - then obs_right says whether that step wrote right observations (armed: of the chain in flight)
    int obs_state = 0;
    bool obs_right = false, obs_right_armed = false;
    // pmv_klt_set_prediction: the pending prediction - its setting, its camera's device table entry, the list in device memory [ids ascending |
    // their points, 3 doubles each] - and {consumed, joined, succ, fell_back} of the last step
    bool pr_on = false;
    pmv_klt_predict_params pr{};
    const LiftCam* pr_cam = nullptr;
    int pr_n = 0;
    Buf<uint8_t> d_pr;
    int pr_res[4] = {0, 0, 0, 0};
    Buf<uint8_t> d_mem, d_rec, h_rec{MEM_PINNED}, h_res{MEM_MAPPED};
    KltDev D; KltRecs R; KltRes O;
};

namespace {
// ---- the blocks of a group (pmv_klt_step_many), each described once; n = trackers, sum = the sum of their targets, pad = the sum of their
// refill_pad(target), cap = the largest target ---------------------------------------------------------------------------------------------
// record block, pinned mirror and device copy: argument records | refill records | half-width tables | frame requests | the sub-pixel
// launch's slots | the call's one-entry geometry table || F flags | F problems | F iteration tables. The front part goes up with every call,
// the used part behind `front` only in front of a k_fundamental_ransac launch.
struct KltGroupRecs {
    Carved<KltManyRec> rec; Carved<RefillRec> rrec; Carved<uint8_t> hw; Carved<int> grec, slots; Carved<PyrLayout> geom; size_t front;
    Carved<int> f_run; Carved<FundamentalProblem> fprob; Carved<double> ftab;
};
KltGroupRecs klt_group_recs(Carve& c, size_t n, size_t sum) {
    KltGroupRecs R;
    R.rec = c.take<KltManyRec>(n, 64); R.rrec = c.take<RefillRec>(n, 16); R.hw = c.take<uint8_t>(n * REFILL_HW, 16); R.grec = c.take<int>(n * CELL_STRIDE, 16);
    R.slots = c.take<int>(n, 16); R.geom = c.take<PyrLayout>(1, 64);
    c.skip_to(64);
    R.front = c.bytes();
    R.f_run = c.take<int>(n, 64); R.fprob = c.take<FundamentalProblem>(n, 64); R.ftab = c.take<double>(sum + 2 * n, 16);
    return R;
}
// device block: LK records and results of the one launch | refill tables | the selection pass's words (found, statistics, wanted) | corners |
// refined corners - each tracker's share starts where the host's record says
struct KltGroupDev {
    Carved<LKBlock> lkb; Carved<LKExt> lkx;
    Carved<float> lk_xy, lk_err, bk_xy, bk_err; Carved<uint8_t> lk_st, bk_st;
    Carved<unsigned> pos; Carved<int> prio; Carved<uint8_t> flag, keep;
    Carved<int> m, stat, want, ixy;
    Carved<float> sp_xy; Carved<uint8_t> sp_it, sp_fl;
    Carved<LKExt> lkx2; Carved<int> pred;   // predicted steps: the fall-back launch's records, the trackers' (successes, wanted) pairs
};
KltGroupDev klt_group_dev(Carve& c, size_t n, size_t sum, size_t pad, size_t cap) {
    KltGroupDev D;
    D.lkb = c.take<LKBlock>(sum, 64); D.lkx = c.take<LKExt>(sum, 16);
    D.lk_xy = c.take<float>(2 * sum, 16); D.lk_err = c.take<float>(sum, 16); D.bk_xy = c.take<float>(2 * sum, 16); D.bk_err = c.take<float>(sum, 16);
    D.lk_st = c.take<uint8_t>(sum, 16); D.bk_st = c.take<uint8_t>(sum, 16);
    D.pos = c.take<unsigned>(pad, 16); D.prio = c.take<int>(pad, 16); D.flag = c.take<uint8_t>(pad, 16); D.keep = c.take<uint8_t>(pad, 16);
    D.m = c.take<int>(n, 16); D.stat = c.take<int>(2 * n, 16); D.want = c.take<int>(n, 16); D.ixy = c.take<int>(2 * n * cap, 16);
    D.sp_xy = c.take<float>(2 * n * cap, 16); D.sp_it = c.take<uint8_t>(n * cap, 16); D.sp_fl = c.take<uint8_t>(n * cap, 16);
    D.lkx2 = c.take<LKExt>(sum, 16); D.pred = c.take<int>(2 * n, 16);
    return D;
}
}  // namespace

struct KltGroup {
    Buf<uint8_t> d_rec, h_rec{MEM_PINNED}, d_mem;
};

bool klt_camera_in_use(pmv_ctx* ctx, int cam_id) {
    std::lock_guard<std::mutex> lk(ctx->klt_mu);
    for (const auto* t : ctx->klt)
        if (t && t->obs_on && (t->obs.cam_id == cam_id || t->obs.right_cam_id == cam_id)) return true;
    return false;
}

bool klt_camera_predicted(pmv_ctx* ctx, int cam_id) {
    std::lock_guard<std::mutex> lk(ctx->klt_mu);
    for (const auto* t : ctx->klt)
        if (t && t->pr_on && t->pr.cam_id == cam_id) return true;
    return false;
}

void klt_destroy_all(pmv_ctx* ctx) {
    for (auto& t : ctx->klt) { delete t; t = nullptr; }
    delete ctx->klt_group;
    ctx->klt_group = nullptr;
}

}  // namespace pmv

using namespace pmv;

#define CKC(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(ctx, "%s: %s", #x, hipGetErrorString(e_)); return PMV_ERR_HIP; } } while (0)
#define REQ(cond, code, ...) do { if (!(cond)) { set_err(ctx, __VA_ARGS__); return code; } } while (0)

static int klt_find(pmv_ctx* ctx, const char* who, int id, KltTracker** out) {
    std::lock_guard<std::mutex> lk(ctx->klt_mu);
    REQ(id >= 0 && id < PMV_KLT_MAX_TRACKERS && ctx->klt[id], PMV_ERR_INVALID, "%s: tracker %d does not exist (pmv_klt_create)", who, id);
    *out = ctx->klt[id];
    return PMV_OK;
}

extern "C" {

int pmv_klt_create(pmv_ctx* ctx, const pmv_klt_params* p, int* out_id) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_create: null argument");
    REQ(p && out_id, PMV_ERR_INVALID, "pmv_klt_create: null argument");
    const int max_n = std::min(ctx->max_tracks, PMV_REFILL_MAX_TRACKS);
    REQ(p->target >= 1, PMV_ERR_INVALID, "pmv_klt_create: target = %d is below 1", p->target);
    REQ(p->target <= max_n, PMV_ERR_CAPACITY, "pmv_klt_create: target = %d is above %d (max_tracks, PMV_REFILL_MAX_TRACKS)", p->target, max_n);
    REQ(p->border >= 0 && p->border <= 64, PMV_ERR_INVALID, "pmv_klt_create: border = %d is outside 0..64", p->border);
    REQ(p->fb_max_dist < 0.0 || p->fb_max_dist <= 1e3, PMV_ERR_INVALID, "pmv_klt_create: fb_max_dist = %g is not finite or above 1e3", p->fb_max_dist);   // (a NaN fails both)
    REQ(p->reject_f == 0 || p->reject_f == 1, PMV_ERR_INVALID, "pmv_klt_create: reject_f = %d is neither 0 nor 1", p->reject_f);
    REQ(p->subpix == 0 || p->subpix == 1, PMV_ERR_INVALID, "pmv_klt_create: subpix = %d is neither 0 nor 1", p->subpix);
    REQ(p->radius >= 0 && p->radius <= PMV_REFILL_MAX_RADIUS, PMV_ERR_INVALID, "pmv_klt_create: radius = %d is outside 0..%d", p->radius, PMV_REFILL_MAX_RADIUS);
    int dummy_i = 0;
    if (p->reject_f) {   // the rules of the call the fields belong to, on 15 points at the origin
        static const float zeros[30] = {};
        double f9[9]; uint8_t m15[15];
        if (const int rc = fundamental_check(ctx, "pmv_klt_create", zeros, zeros, 15, p->f_threshold, p->f_confidence, f9, m15, &dummy_i, &dummy_i)) return rc;
    }
    if (const int rc = gftt_ex_check(ctx, "pmv_klt_create", &p->gftt, &dummy_i, &dummy_i)) return rc;
    if (p->subpix) if (const int rc = subpix_params_check(ctx, "pmv_klt_create", &p->subpix_params)) return rc;
    std::lock_guard<std::mutex> lk(ctx->klt_mu);
    int id = 0;
    while (id < PMV_KLT_MAX_TRACKERS && ctx->klt[id]) id++;
    REQ(id < PMV_KLT_MAX_TRACKERS, PMV_ERR_CAPACITY, "pmv_klt_create: the context holds %d trackers already (pmv_klt_destroy one)", PMV_KLT_MAX_TRACKERS);
    CKC(hipSetDevice(ctx->device));
    KltTracker* t = new KltTracker();
    t->p = *p; t->cap = p->target;
    t->thr2 = p->fb_max_dist >= 0.0 ? (float)(p->fb_max_dist * p->fb_max_dist) : 0.f;
    const size_t cap = (size_t)t->cap;
    Carve nd, nr, no;
    klt_dev_block(nd, cap); klt_rec_block(nr, cap); klt_res_block(no, cap);
    hipError_t e = t->d_mem.ensure(nd.bytes() + 64);
    if (e == hipSuccess) e = t->d_rec.ensure(nr.bytes() + 64);
    if (e == hipSuccess) e = t->h_rec.ensure(nr.bytes() + 64);
    if (e == hipSuccess) e = t->h_res.ensure(no.bytes() + 64);
    if (e == hipSuccess) e = hipMemset(t->d_mem, 0, nd.bytes());
    if (e == hipSuccess) {
        Carve cd(nullptr, t->d_mem.p, t->d_mem.cap), cr(t->h_rec.p, t->d_rec.p, t->h_rec.cap), co = carve_of(t->h_res);
        t->D = klt_dev_block(cd, cap); t->R = klt_rec_block(cr, cap); t->O = klt_res_block(co, cap);
        memset(t->h_rec, 0, nr.bytes()); memset(t->h_res, 0, no.bytes());
        refill_halfwidths(p->radius, t->R.hw.h);
        std::vector<int> order((cap + 7) / 8 * 8);   // the identity: a block beyond the launch's n leaves at once
        for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
        e = hipMemcpy(t->D.order.d, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { delete t; set_err(ctx, "pmv_klt_create: %s", hipGetErrorString(e)); return PMV_ERR_HIP; }
    ctx->klt[id] = t;
    *out_id = id;
    return PMV_OK;
}

int pmv_klt_destroy(pmv_ctx* ctx, int id) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_destroy: null argument");
    std::lock_guard<std::mutex> lk(ctx->klt_mu);
    REQ(id >= 0 && id < PMV_KLT_MAX_TRACKERS && ctx->klt[id], PMV_ERR_INVALID, "pmv_klt_destroy: tracker %d does not exist", id);
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    delete ctx->klt[id];
    ctx->klt[id] = nullptr;
    return PMV_OK;
}

int pmv_klt_set_tracks(pmv_ctx* ctx, int id, const int* ids, const int* ages, const float* xy, int n, int next_id) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_set_tracks: null argument");
    KltTracker* t;
    if (const int rc = klt_find(ctx, "pmv_klt_set_tracks", id, &t)) return rc;
    REQ(n >= 0 && n <= t->cap, PMV_ERR_CAPACITY, "pmv_klt_set_tracks: n = %d is outside 0..%d (the tracker's target)", n, t->cap);
    REQ(n == 0 || (ids && ages && xy), PMV_ERR_INVALID, "pmv_klt_set_tracks: null argument");
    REQ(next_id >= 0, PMV_ERR_INVALID, "pmv_klt_set_tracks: next_id = %d is negative", next_id);
    for (int i = 0; i < 2 * n; i++)   // (a NaN fails the comparison too)
        REQ(fabsf(xy[i]) <= 1e6f, PMV_ERR_INVALID, "pmv_klt_set_tracks: track %d (%g, %g) is not finite or beyond 1e6", i / 2, (double)xy[i & ~1], (double)xy[i | 1]);
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    if (n > 0) {
        CKC(hipMemcpy(t->D.s_id.d, ids, (size_t)n * 4, hipMemcpyHostToDevice));
        CKC(hipMemcpy(t->D.s_age.d, ages, (size_t)n * 4, hipMemcpyHostToDevice));
        CKC(hipMemcpy(t->D.s_xy.d, xy, (size_t)n * 8, hipMemcpyHostToDevice));
    }
    t->n = n; t->next_id = next_id; t->obs_state = 0;
    return PMV_OK;
}

int pmv_klt_get_tracks(pmv_ctx* ctx, int id, int* ids, int* ages, float* xy, int cap, int* out_n) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_get_tracks: null argument");
    KltTracker* t;
    if (const int rc = klt_find(ctx, "pmv_klt_get_tracks", id, &t)) return rc;
    REQ(out_n && (t->n == 0 || (ids && ages && xy)), PMV_ERR_INVALID, "pmv_klt_get_tracks: null argument");
    REQ(cap >= t->n, PMV_ERR_CAPACITY, "pmv_klt_get_tracks: cap = %d is below the %d tracks held", cap, t->n);
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));
    if (t->n > 0) {
        CKC(hipMemcpy(ids, t->D.s_id.d, (size_t)t->n * 4, hipMemcpyDeviceToHost));
        CKC(hipMemcpy(ages, t->D.s_age.d, (size_t)t->n * 4, hipMemcpyDeviceToHost));
        CKC(hipMemcpy(xy, t->D.s_xy.d, (size_t)t->n * 8, hipMemcpyDeviceToHost));
    }
    *out_n = t->n;
    return PMV_OK;
}

}  // extern "C"

// ---- what pmv_klt_step and pmv_klt_step_many share on the host ------------------------------------------------------------------------
// Where a tracker's parts of a chain's per-launch tables live: its own buffers in a single step, its shares of the group's blocks in a
// many-call.
struct KltLkOut { float* xy; float* bk_xy; uint8_t* st; uint8_t* bk_st; };   // what the stage kernels read of an LK launch's results
struct KltShares {
    KltLkOut lk; KltRefillIn rf; uint8_t* keep;   // stage 1's results for the tracker's state | what k_track_select reads, with the refill record | the keep bytes it leaves
    int* want; int* m; int* stat;                 // the selection pass's words: corners wanted, corners found, its two statistics
    int* ixy; float* sp_xy;                       // the corner list and the refined corners
    unsigned long long prev_off, next_off; int lk_base;   // a many-call: byte offsets of the two frame slots, first index of the share of stage 1's LK records
    // a stereo call: stage 8's results (the LK result arrays of stage 1 are free again by then), whether the tracker has a right frame in this
    // call, and for a many-call the right slot's offset and the share's first index
    bool stereo; int right_on; KltLkOut st; unsigned long long right_off; int st_base;
    int* pred; int pred_slot;                     // a predicted step: the tracker's (successes, wanted) pair and its index in the launch's table
};
// THE description of what the stage kernels of tracker t are given in its next chain, which begins here: the completion words are armed
// before anything is launched. The many-call stores the record in its block, the single step passes its members as kernel arguments.
// by_keep.in / out, append.in and observe.prev are written for list 0 and append.f_info is null: which list holds the tracks and whether F ran is known
// after stage 3 - k_klt_compact_many and k_klt_append_many patch them on the device, klt_step_run on the host.
static KltManyRec klt_stage_args(KltTracker* t, const PyrLayout& L, const KltShares& sh) {
    if (++t->seq == 0) t->seq = 1;
    t->O.hdr.h[9] = 0; t->O.hdr.h[10] = 0;
    const pmv_klt_params& p = t->p;
    const KltDev& D = t->D; const KltRes& O = t->O;
    const bool fb = p.fb_max_dist >= 0.0;
    int* cnt = D.cnt.d;
    KltManyRec M{};
    for (int k = 0; k < 2; k++) { M.lst[k].id = D.l_id[k].d; M.lst[k].age = D.l_age[k].d; M.lst[k].prev = D.l_prev[k].d; M.lst[k].cur = D.l_cur[k].d; }
    KltFilterArgs& F = M.filter;
    F.n0 = t->n; F.fb = fb ? 1 : 0; F.border = p.border; F.w = L.w[0]; F.h = L.h[0]; F.thr2 = t->thr2;
    F.id = D.s_id.d; F.age = D.s_age.d; F.prev = D.s_xy.d; F.fwd = sh.lk.xy; F.back = sh.lk.bk_xy; F.st = sh.lk.st; F.bst = sh.lk.bk_st;
    F.out = M.lst[0]; F.rf = sh.rf; F.cnt = cnt; F.h_n1 = O.n1.d;
    KltCompactArgs& BF = M.by_f;
    BF.in = M.lst[0]; BF.out = M.lst[1]; BF.mask = (const uint8_t*)(D.f_out.d + ESS_OUT_HDR); BF.n_in = cnt + C_N1;
    BF.cap = t->cap; BF.cnt_out = C_N2; BF.target = 0; BF.rf = sh.rf; BF.cnt = cnt; BF.want = sh.want;
    KltCompactArgs& BK = M.by_keep;   // (rf stays null: nothing is written for k_track_select)
    BK.in = M.lst[0]; BK.out = M.lst[1]; BK.mask = sh.keep; BK.n_in = cnt + C_N2;
    BK.cap = t->cap; BK.cnt_out = C_N3; BK.target = t->cap; BK.cnt = cnt; BK.want = sh.want;
    KltAppendArgs& A = M.append;
    A.in = M.lst[0]; A.cnt = cnt; A.m = sh.m; A.ixy = sh.ixy; A.sp_xy = p.subpix ? sh.sp_xy : nullptr; A.f_info = nullptr;
    A.n0 = t->n; A.next_id = t->next_id; A.target = t->cap; A.seq = t->seq; A.s_id = D.s_id.d; A.s_age = D.s_age.d; A.s_xy = D.s_xy.d;
    A.r_hdr = O.hdr.d; A.r_id = O.id.d; A.r_age = O.age.d; A.r_xy = O.xy.d; A.r_prev = O.prev.d; A.n_out = sh.stereo ? cnt + C_NOUT : nullptr;
    M.f_info = (const int*)(D.f_out.d + ESS_OUT_INFO);
    M.prev_off = sh.prev_off; M.next_off = sh.next_off; M.lk_base = sh.lk_base; M.lk_flags = fb ? LKX_FB : 0;
    if (t->pr_on && t->n > 0) {   // (with no track the prediction is consumed on the host alone)
        KltPredictArgs& Q = M.predict;
        Q.on = 1; Q.n_list = t->pr_n; Q.top = t->pr.top_level; Q.back_top = t->pr.back_top_level; Q.min_succ = t->pr.min_succ; Q.slot = sh.pred_slot;
        Q.ids = (const int*)t->d_pr.p; Q.xyz = (const double*)((const uint8_t*)t->d_pr.p + klt_pr_xyz_off((size_t)t->pr_n)); Q.cam = t->pr_cam;
        Q.pred = sh.pred; Q.joined = cnt + C_JOINED; Q.guess = D.pr_guess.d;
        A.joined = Q.joined; A.pred = Q.pred;
    }
    if (sh.stereo) {
        const bool sfb = sh.right_on && t->st.fb_max_dist >= 0.0;
        KltStereoArgs& S = M.stereo;
        S.n = cnt + C_NOUT; S.cap = t->cap; S.on = sh.right_on ? 1 : 0; S.fb = sfb ? 1 : 0; S.border = t->st.border; S.w = L.w[0]; S.h = L.h[0]; S.thr2 = t->st_thr2;
        S.prev = D.s_xy.d; S.fwd = sh.st.xy; S.back = sh.st.bk_xy; S.st = sh.st.st; S.bst = sh.st.bk_st;
        S.seq = t->seq; S.r_hdr = O.hdr.d; S.r_rxy = O.right_xy.d; S.r_rst = O.right_st.d;
        M.right_off = sh.right_off; M.st_base = sh.st_base; M.st_flags = sfb ? LKX_FB : 0;
    }
    if (t->obs_on) {
        t->O.hdr.h[11] = 0;
        A.n_out = cnt + C_NOUT;
        KltObserveArgs& V = M.observe;
        V.on = 1; V.cap = t->cap; V.right = sh.stereo && sh.right_on && t->obs_rcam ? 1 : 0;
        V.cnt = cnt; V.age = D.s_age.d; V.xy = D.s_xy.d; V.prev = M.lst[0].prev;
        V.cam = t->obs_cam; V.rcam = t->obs_rcam; V.dt = t->obs.dt; V.seq = t->seq;
        V.r_hdr = O.hdr.d; V.r_un = O.un_xy.d; V.r_vel = O.vel.d; V.r_ok = O.un_ok.d; V.r_run = O.right_un.d; V.r_rok = O.right_un_ok.d;
        t->obs_right_armed = V.right != 0;
        if (t->obs.undistorted_f && p.reject_f && t->n >= 15) {   // the F stage may run: its points are written under the wait for n1
            KltLiftFArgs& Q = M.lift_f;
            Q.on = 1; Q.cap = t->n; Q.n1 = cnt + C_N1; Q.prev = D.l_prev[0].d; Q.cur = D.l_cur[0].d; Q.cam = t->obs_cam;
            Q.f = t->obs.f_focal; Q.hw = L.w[0] / 2.0; Q.hh = L.h[0] / 2.0;
            Q.p1 = sh.lk.xy; Q.p2 = sh.lk.bk_xy;   // stage 1's results are consumed by the filter; a share holds 2 n0 floats each
        }
    }
    return M;
}
// one launch of a glue kernel (KT threads per workgroup), booked under the detector's selection class
template <class... P, class... A> static hipError_t klt_launch(void (*kernel)(P...), int grid, hipStream_t s, A... args) {
    ProfScope ps(K_GFTT_PICK, s);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(KT), 0, s, args...);
    return hipGetLastError();
}
// rejectWithF's problem for the n1 tracks the filter left in the tracker's list 0 - their pixels, or with Q.on the virtual-camera points
// k_klt_lift_f wrote - and libm's iteration table (n1 + 2 doubles) at tab_h
static FundamentalProblem klt_f_problem(const KltTracker* t, const KltLiftFArgs& Q, int n1, double* tab_h, const double* tab_d) {
    vo::ransac_iters_table(n1, t->p.f_confidence, 7, tab_h + 1, tab_h);
    return whole_problem<float>(Q.on ? Q.p1 : t->D.l_prev[0].d, Q.on ? Q.p2 : t->D.l_cur[0].d, tab_d, t->D.f_out.d, n1, t->p.f_threshold, WHOLE_MAX_ITERS, 1);
}
// after the final wait: the header of the tracker's result block (`who`: pmv_klt_step or pmv_klt_step_many; j >= 0: tracker j of a group)
static int klt_result_check(pmv_ctx* ctx, const KltTracker* t, bool stereo, const char* who, int j) {
    const int* hdr = t->O.hdr.h;
    const int n = hdr[8], m = hdr[4];
    char of[48] = "";
    if (j >= 0) snprintf(of, sizeof(of), " of tracker %d of the group", j);
    REQ((unsigned)hdr[9] == t->seq && n >= 0 && n <= t->cap && m >= 0 && m <= n, PMV_ERR_HIP, "%s: the result block%s is incomplete (n = %d, m = %d)", who, of, n, m);
    REQ(!stereo || ((unsigned)hdr[10] == t->seq && hdr[7] >= 0 && hdr[7] <= n), PMV_ERR_HIP, "%s_stereo: the result block%s is incomplete (n = %d, matched = %d)", who, of, n,
        hdr[7]);
    REQ(!t->obs_on || (unsigned)hdr[11] == t->seq, PMV_ERR_HIP, "%s: the observations of the result block%s are incomplete (n = %d)", who, of, n);
    REQ(hdr[12] >= 0 && hdr[12] <= hdr[0] && hdr[13] >= 0 && hdr[13] <= hdr[0], PMV_ERR_HIP, "%s: the prediction words of the result block%s are out of range (joined = %d, succ = %d of %d)",
        who, of, hdr[12], hdr[13], hdr[0]);
    return PMV_OK;
}
// ... and the copy-out of a checked block to the caller's arrays, which begin at the tracker's place; the state's length and next id follow
// it. right: null in a call without stage 8; slot < 0: the tracker has no right frame in this (many-)call - status zeros, xy untouched.
struct KltRightOut { int slot; float* xy; uint8_t* st; };
static void klt_result_copy(KltTracker* t, int* ids, int* ages, float* xy, float* prev_xy_or_null, int* out_n, int* counts8, const KltRightOut* right) {
    const KltRes& O = t->O;
    const int n = O.hdr.h[8], m = O.hdr.h[4];
    memcpy(ids, O.id.h, (size_t)n * 4);
    memcpy(ages, O.age.h, (size_t)n * 4);
    memcpy(xy, O.xy.h, (size_t)n * 8);
    if (prev_xy_or_null) memcpy(prev_xy_or_null, O.prev.h, (size_t)n * 8);
    memcpy(counts8, O.hdr.h, 8 * sizeof(int));
    *out_n = n;
    if (right && right->slot >= 0) {
        memcpy(right->xy, O.right_xy.h, (size_t)n * 8);
        memcpy(right->st, O.right_st.h, (size_t)n);
    } else if (right) memset(right->st, 0, (size_t)n);
    t->n = n; t->next_id += m;
    // the step succeeded: a pending prediction is consumed by it (with no track to join: {1, 0, 0, 0}, the header words are 0 then)
    t->pr_res[0] = t->pr_on ? 1 : 0; t->pr_res[1] = t->pr_on ? O.hdr.h[12] : 0; t->pr_res[2] = t->pr_on ? O.hdr.h[13] : 0; t->pr_res[3] = t->pr_on ? O.hdr.h[14] : 0;
    t->pr_on = false;
    t->obs_state = t->obs_on ? 2 : 1; t->obs_right = t->obs_on && t->obs_right_armed;
}
// the closing statistics of a step (n_trk = 0) or of a many-call on n_trk trackers; the mask at the front of the scratch is now the region's
// of this call (a group's: tracker 0's)
struct KltObserveBook { bool on; int observe, lift; };   // a tracker of the call has an observation setting | the launches made for stage 9 | for stage 3
static void klt_book(pmv_ctx* ctx, const int* roi, int n_trk, bool stereo, long long waits, long long launches, const KltObserveBook& ob) {
    ctx->refill_last[0] = roi[2]; ctx->refill_last[1] = roi[3];
    if (ob.on) { ctx->klt_observe_stats[0]++; ctx->klt_observe_stats[1] += ob.observe; ctx->klt_observe_stats[2] += ob.lift; ctx->klt_observe_stats[3] += waits; }
    if (stereo) { ctx->klt_stereo_stats[n_trk ? 1 : 0]++; ctx->klt_stereo_stats[2] += waits; ctx->klt_stereo_stats[3] += launches; }
    else if (n_trk) { ctx->klt_many_stats[0]++; ctx->klt_many_stats[1] += n_trk; ctx->klt_many_stats[2] += waits; ctx->klt_many_stats[3] += launches; }
    else { ctx->klt_stats[0]++; ctx->klt_stats[1] += waits; ctx->klt_stats[2] += launches; }
}

// pmv_klt_step and, with `right`, pmv_klt_step_stereo: the same chain, refused in the same words; the stereo form appends stage 8
static int klt_step_run(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int* out_ids, int* out_ages, float* out_xy, float* out_prev_xy_or_null, int out_cap, int* out_n,
                        int* out_counts8, const KltRightOut* right) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_step: null argument");
    KltTracker* t;
    if (const int rc = klt_find(ctx, "pmv_klt_step", id, &t)) return rc;
    REQ(out_ids && out_ages && out_xy && out_n && out_counts8, PMV_ERR_INVALID, "pmv_klt_step: null argument");
    REQ(!right || (right->xy && right->st), PMV_ERR_INVALID, "pmv_klt_step_stereo: null argument");
    REQ(out_cap >= t->cap, PMV_ERR_CAPACITY, "pmv_klt_step: out_cap = %d is below the tracker's target %d", out_cap, t->cap);
    REQ(!right || t->st_on, PMV_ERR_INVALID, "pmv_klt_step_stereo: tracker %d has no stereo setting (pmv_klt_set_stereo)", id);
    const pmv_klt_params& p = t->p;
    const int n0 = t->n, cap = t->cap;
    // the slot rules of the calls the stages are: LK's for the pair (only when something is tracked), the frame detector's for cur_slot
    if (n0 > 0)
        if (const int rc = lk_check(ctx, true, prev_slot, cur_slot, out_xy, n0, out_xy, (const uint8_t*)out_ids, out_xy)) return rc;
    int roi[4], gcap;
    if (const int rc = gftt_frame_check(ctx, "pmv_klt_step", true, cur_slot, nullptr, cap, &p.gftt, nullptr, 0, out_ids, cap, out_n, roi, &gcap)) return rc;
    // stage 8's LK pair, before anything is launched: the length of the list it tracks is known only on the device
    if (right)
        if (const int rc = lk_check(ctx, true, cur_slot, right->slot, nullptr, 0, nullptr, nullptr, nullptr)) return rc;
    tl_prof = &ctx->prof; CKC(hipSetDevice(ctx->device));
    const PyrLayout& L = ctx->slot_layout[cur_slot];
    const size_t pix = (size_t)ctx->max_w * ctx->max_h, rpix = (size_t)roi[2] * roi[3];
    // the context's scratch of the refill and frame calls (rewritten by every call and every step); records and results are the tracker's
    FrameDetScratch& S = ctx->fds;
    CKC(S.lists(pix, 1)); CKC(S.masks(pix + S.PAINT_SLACK, 0)); CKC(S.refill(PMV_REFILL_MAX_TRACKS, 1));
    SubpixArgs SA{};
    if (p.subpix) CKC(subpix_table_ready(ctx, &p.subpix_params, &SA));
    hipStream_t s = ctx->s_front;
    const KltDev& D = t->D; const KltRecs& R = t->R; const KltRes& O = t->O;
    long long launches = 0, waits = 0;
    // records: the refill request (its n is written by the kernels), the frame request
    *R.rrec.h = RefillRec{0, p.radius, 0, roi[0], roi[1], roi[2], roi[3], 0u, 0, {0, 0, 0}};
    gftt_frame_record(R.grec.h, roi, cur_slot, 0, nullptr, 0, nullptr, 0);
    CKC(hipMemcpyAsync(t->d_rec, t->h_rec, R.front, hipMemcpyHostToDevice, s));
    // the stage arguments, from the tracker's own buffers
    KltShares sh{};
    sh.lk = KltLkOut{D.lk_xy.d, D.bk_xy.d, D.lk_st.d, D.bk_st.d};
    sh.rf = KltRefillIn{D.pos.d, D.prio.d, D.flag.d, R.rrec.d};
    sh.keep = D.keep.d; sh.want = D.cnt.d + C_WANT; sh.m = D.cnt.d + C_M; sh.stat = D.cnt.d + C_STAT0; sh.ixy = D.ixy.d; sh.sp_xy = D.sp_xy.d;
    sh.stereo = right != nullptr; sh.right_on = 1; sh.st = sh.lk;
    sh.pred = D.cnt.d + C_SUCC; sh.pred_slot = 0;
    KltManyRec M = klt_stage_args(t, L, sh);
    // 1. track; with a pending prediction from the projected guesses on the capped levels, counting the forward successes, and then the
    // gated launch over the full pyramid, whose workgroups leave at once unless the successes fell short
    if (n0 > 0) {
        const PyrLayout& Lp = ctx->slot_layout[prev_slot];
        const uint8_t* const ps = ctx->d_slots + (size_t)prev_slot * Lp.slot_bytes;
        const uint8_t* const cs = ctx->d_slots + (size_t)cur_slot * Lp.slot_bytes;
        const int nb = (n0 + 7) / 8 * 8;
        if (M.predict.on) {
            const KltPredictArgs& Q = M.predict;
            CKC(klt_launch(k_klt_predict, 1, s, Q, n0, (const int*)D.s_id.d, (const float*)D.s_xy.d));
            CKC(launch_lk_ex(s, ps, cs, Lp, D.s_xy.d, Q.guess, D.order.d, nb, n0, M.lk_flags | LKX_INIT, lk_launch_params(ctx), D.lk_xy.d, D.lk_st.d, D.lk_err.d, nullptr, D.bk_xy.d,
                             D.bk_st.d, D.bk_err.d, Q.top, Q.back_top, Q.pred, LKP_COUNT));
            CKC(launch_lk_ex(s, ps, cs, Lp, D.s_xy.d, nullptr, D.order.d, nb, n0, M.lk_flags, lk_launch_params(ctx), D.lk_xy.d, D.lk_st.d, D.lk_err.d, nullptr, D.bk_xy.d, D.bk_st.d,
                             D.bk_err.d, -1, Q.back_top, Q.pred, LKP_GATE));
            launches += 3;
        } else {
            CKC(launch_lk_ex(s, ps, cs, Lp, D.s_xy.d, nullptr, D.order.d, nb, n0, M.lk_flags, lk_launch_params(ctx), D.lk_xy.d, D.lk_st.d, D.lk_err.d, nullptr, D.bk_xy.d, D.bk_st.d,
                             D.bk_err.d));
            launches++;
        }
    }
    // 2. filter
    CKC(klt_launch(k_klt_filter, 1, s, M.filter)); launches++;
    // 3. rejectWithF: the host reads n1 (the iteration table is libm's) and sends the table with the launches of the second half; with
    // undistorted_f the lift of the survivors runs under that wait
    KltObserveBook ob{t->obs_on, 0, 0};
    int cur = 0; bool f_ran = false;
    if (p.reject_f && n0 >= 15) {
        if (M.lift_f.on) { CKC(klt_launch(k_klt_lift_f, (n0 + KT - 1) / KT, s, M.lift_f)); launches++; ob.lift++; }
        CKC(hipStreamSynchronize(s));
        waits++;
        const int n1 = *O.n1.h;
        REQ(n1 >= 0 && n1 <= n0, PMV_ERR_HIP, "pmv_klt_step: the filter left n1 = %d of %d tracks", n1, n0);
        if (n1 >= 15) {
            const FundamentalProblem P = klt_f_problem(t, M.lift_f, n1, R.ftab.h, R.ftab.d);
            memset(R.fprob.h, 0, ESS_HDR);
            memcpy(R.fprob.h, &P, sizeof(P));
            const size_t fbytes = (size_t)((const char*)(R.ftab.h + n1 + 2) - R.fprob.h);
            CKC(hipMemcpyAsync((char*)t->d_rec.p + R.fprob.off, R.fprob.h, fbytes, hipMemcpyHostToDevice, s));
            CKC(launch_fundamental_ransac(s, (const FundamentalProblem*)R.fprob.d, 1));
            CKC(klt_launch(k_klt_compact, 1, s, M.by_f));
            launches += 2; cur = 1; f_ran = true;
        }
    }
    // what the many-kernels decide on the device: the later stages read the list the tracks are in now, and F's info only if F ran
    M.by_keep.in = M.lst[cur]; M.by_keep.out = M.lst[cur ^ 1];
    M.append.in = M.lst[cur ^ 1];
    M.append.f_info = f_ran ? M.f_info : nullptr;
    // 4. thin: setMask's walk and painting on the list, then the compaction by its keep bytes, which leaves the number of corners wanted
    CKC(launch_track_refill(s, R.rrec.d, 1, rpix, D.pos.d, D.prio.d, D.flag.d, R.hw.d, D.keep.d, S.d_refill_kept, S.d_refill_nkept, S.d_gfr_mask));
    launches += 2;
    CKC(klt_launch(k_klt_compact, 1, s, M.by_keep)); launches++;
    // 5. refill: the frame call's two passes with the painted mask; the selection takes its cap from the counts
    const GfttExt X = gftt_ext(p.gftt.block_size, p.gftt.use_harris, p.gftt.k);
    CKC(launch_gftt_frame(s, ctx->d_slots, L, R.grec.d, 1, gftt_frame_grid_x(roi[2], roi[3]), cap, p.gftt.quality, p.gftt.min_dist, 0, &X, S.d_gfr_mask.get(), S.d_gfr_val,
                          S.d_gfr_idx, S.d_gfr_info, S.d_gfr_keys, D.ixy.d, sh.m, sh.stat, sh.want));
    launches += 2;
    // 6. refine
    if (p.subpix) {
        CKC(launch_corner_subpix_dev(s, ctx->d_slots, L, D.ixy.d, cur_slot, cap, sh.m, ctx->d_subpix_tab, SA, D.sp_xy.d, D.sp_it.d, D.sp_fl.d));
        launches++;
    }
    // 7. append
    CKC(klt_launch(k_klt_append, 1, s, M.append)); launches++;
    // 8. stereo: the new state from the current left frame into the right frame - `cap` workgroups, of which the device's count work (the LK
    // result arrays of stage 1 are free again) - then the rule, which ends the chain with its own completion word
    if (right) {
        CKC(launch_lk_ex_dev(s, ctx->d_slots + (size_t)cur_slot * L.slot_bytes, ctx->d_slots + (size_t)right->slot * L.slot_bytes, L, D.s_xy.d, D.cnt.d + C_NOUT, cap,
                             M.st_flags, lk_launch_params(ctx), D.lk_xy.d, D.lk_st.d, D.lk_err.d, D.bk_xy.d, D.bk_st.d, D.bk_err.d));
        CKC(klt_launch(k_klt_stereo, 1, s, M.stereo));
        launches += 2;
    }
    // 9. observe: the lifts and velocities of the list the step returns; then this kernel ends the chain
    if (M.observe.on) {
        M.observe.prev = M.lst[cur ^ 1].prev;
        CKC(klt_launch(k_klt_observe, 1, s, M.observe, M.stereo)); launches++; ob.observe++;
    }
    CKC(hipStreamSynchronize(s));
    waits++;
    if (const int rc = klt_result_check(ctx, t, right != nullptr, "pmv_klt_step", -1)) return rc;
    klt_result_copy(t, out_ids, out_ages, out_xy, out_prev_xy_or_null, out_n, out_counts8, right);
    klt_book(ctx, roi, 0, right != nullptr, waits, launches, ob);
    return PMV_OK;
}

extern "C" {

int pmv_klt_step(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int* out_ids, int* out_ages, float* out_xy, float* out_prev_xy_or_null, int out_cap, int* out_n,
                 int* out_counts8) {
    return klt_step_run(ctx, id, prev_slot, cur_slot, out_ids, out_ages, out_xy, out_prev_xy_or_null, out_cap, out_n, out_counts8, nullptr);
}

int pmv_klt_step_stereo(pmv_ctx* ctx, int id, int prev_slot, int cur_slot, int right_slot, int* out_ids, int* out_ages, float* out_xy, float* out_prev_xy_or_null,
                        float* out_right_xy, uint8_t* out_right_status, int out_cap, int* out_n, int* out_counts8) {
    const KltRightOut right{right_slot, out_right_xy, out_right_status};
    return klt_step_run(ctx, id, prev_slot, cur_slot, out_ids, out_ages, out_xy, out_prev_xy_or_null, out_cap, out_n, out_counts8, &right);
}

int pmv_klt_set_stereo(pmv_ctx* ctx, int id, const pmv_klt_stereo_params* p_or_null) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_set_stereo: null argument");
    KltTracker* t;
    if (const int rc = klt_find(ctx, "pmv_klt_set_stereo", id, &t)) return rc;
    if (!p_or_null) { t->st_on = false; return PMV_OK; }
    const pmv_klt_stereo_params& p = *p_or_null;
    REQ(std::isfinite(p.fb_max_dist) && p.fb_max_dist <= 1e3, PMV_ERR_INVALID, "pmv_klt_set_stereo: fb_max_dist = %g is not finite or above 1e3", p.fb_max_dist);
    REQ(p.border >= 0 && p.border <= 64, PMV_ERR_INVALID, "pmv_klt_set_stereo: border = %d is outside 0..64", p.border);
    t->st = p; t->st_on = true;
    t->st_thr2 = p.fb_max_dist >= 0.0 ? (float)(p.fb_max_dist * p.fb_max_dist) : 0.f;
    return PMV_OK;
}

int pmv_klt_set_prediction(pmv_ctx* ctx, int id, const pmv_klt_predict_params* p_or_null, const int* ids, const double* xyz, int n) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_set_prediction: null argument");
    KltTracker* t;
    if (const int rc = klt_find(ctx, "pmv_klt_set_prediction", id, &t)) return rc;
    if (!p_or_null || n == 0) { t->pr_on = false; return PMV_OK; }
    const pmv_klt_predict_params& p = *p_or_null;
    REQ(n > 0, PMV_ERR_INVALID, "pmv_klt_set_prediction: n = %d is negative", n);
    REQ(n <= PMV_REFILL_MAX_TRACKS, PMV_ERR_CAPACITY, "pmv_klt_set_prediction: n = %d is above %d (PMV_REFILL_MAX_TRACKS)", n, PMV_REFILL_MAX_TRACKS);
    REQ(ids && xyz, PMV_ERR_INVALID, "pmv_klt_set_prediction: null argument");
    const LiftCam* cam = camera_entry(ctx, p.cam_id);
    REQ(cam, PMV_ERR_INVALID, "pmv_klt_set_prediction: cam_id = %d: the camera does not exist (pmv_camera_create)", p.cam_id);
    REQ(p.top_level >= 0 && p.top_level < MAX_LEVELS, PMV_ERR_INVALID, "pmv_klt_set_prediction: top_level = %d is outside 0..%d", p.top_level, MAX_LEVELS - 1);
    REQ(p.back_top_level >= -1 && p.back_top_level < MAX_LEVELS, PMV_ERR_INVALID, "pmv_klt_set_prediction: back_top_level = %d is outside -1..%d", p.back_top_level, MAX_LEVELS - 1);
    REQ(p.min_succ >= 0, PMV_ERR_INVALID, "pmv_klt_set_prediction: min_succ = %d is negative", p.min_succ);
    // the list sorted by id, once: the kernels search it. A point of any value is legal (one that cannot be projected predicts nothing).
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return ids[a] < ids[b]; });
    for (int i = 1; i < n; i++)
        REQ(ids[order[(size_t)i]] != ids[order[(size_t)i - 1]], PMV_ERR_INVALID, "pmv_klt_set_prediction: id %d is named twice (entries %d and %d)", ids[order[(size_t)i]],
            std::min(order[(size_t)i - 1], order[(size_t)i]), std::max(order[(size_t)i - 1], order[(size_t)i]));
    const size_t xoff = klt_pr_xyz_off((size_t)n), bytes = xoff + (size_t)n * 3 * sizeof(double);
    std::vector<uint8_t> host(bytes, 0);
    int* hid = (int*)host.data(); double* hx = (double*)(host.data() + xoff);
    for (int i = 0; i < n; i++) {
        const int k = order[(size_t)i];
        hid[i] = ids[k]; hx[3 * i] = xyz[3 * k]; hx[3 * i + 1] = xyz[3 * k + 1]; hx[3 * i + 2] = xyz[3 * k + 2];
    }
    CKC(hipSetDevice(ctx->device));
    CKC(hipStreamSynchronize(ctx->s_front));   // (no chain in flight reads the old list)
    if (bytes > t->d_pr.cap) t->pr_on = false;   // (growing frees the old list first: should that fail, nothing is pending)
    CKC(t->d_pr.ensure(bytes));
    t->pr_on = false;
    CKC(hipMemcpy(t->d_pr.p, host.data(), bytes, hipMemcpyHostToDevice));
    t->pr = p; t->pr_cam = cam; t->pr_n = n; t->pr_on = true;
    return PMV_OK;
}

int pmv_klt_get_prediction_result(pmv_ctx* ctx, int id, int* out4) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_get_prediction_result: null argument");
    KltTracker* t;
    if (const int rc = klt_find(ctx, "pmv_klt_get_prediction_result", id, &t)) return rc;
    REQ(out4, PMV_ERR_INVALID, "pmv_klt_get_prediction_result: null argument");
    memcpy(out4, t->pr_res, sizeof(t->pr_res));
    return PMV_OK;
}

int pmv_klt_get_stereo(pmv_ctx* ctx, int id, pmv_klt_stereo_params* out, int* out_on) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_get_stereo: null argument");
    KltTracker* t;
    if (const int rc = klt_find(ctx, "pmv_klt_get_stereo", id, &t)) return rc;
    REQ(out && out_on, PMV_ERR_INVALID, "pmv_klt_get_stereo: null argument");
    *out = t->st; *out_on = t->st_on ? 1 : 0;
    return PMV_OK;
}

}  // extern "C"

// a check of a single call failed for tracker j of a group: its message, with the tracker named behind it
static int klt_many_blame(pmv_ctx* ctx, int rc, int j, int id) {
    char msg[400];
    snprintf(msg, sizeof(msg), "%s", thread_error());
    set_err(ctx, "%s (tracker %d of the group, id %d)", msg, j, id);
    return rc;
}

// pmv_klt_step_many and, with `right`, pmv_klt_step_many_stereo (right->slots[j] < 0: tracker j has no right frame in this call)
struct KltRightManyOut { const int* slots; float* xy; uint8_t* st; };
static int klt_step_many_run(pmv_ctx* ctx, int n_trk, const int* ids, const int* prev_slots, const int* cur_slots, int* out_ids, int* out_ages, float* out_xy,
                             float* out_prev_xy_or_null, int out_stride, int* out_n, int* out_counts8, const KltRightManyOut* right) {
    const char* who = "pmv_klt_step_many";
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_step_many: null argument");
    REQ(n_trk >= 1, PMV_ERR_INVALID, "%s: n_trk = %d is below 1", who, n_trk);
    REQ(n_trk <= PMV_KLT_MAX_TRACKERS, PMV_ERR_CAPACITY, "%s: n_trk = %d is above %d (PMV_KLT_MAX_TRACKERS)", who, n_trk, PMV_KLT_MAX_TRACKERS);
    REQ(ids && prev_slots && cur_slots && out_ids && out_ages && out_xy && out_n && out_counts8, PMV_ERR_INVALID, "%s: null argument", who);
    REQ(!right || (right->slots && right->xy && right->st), PMV_ERR_INVALID, "pmv_klt_step_many_stereo: null argument");
    KltTracker* T[PMV_KLT_MAX_TRACKERS];
    int cap_max = 0;
    for (int j = 0; j < n_trk; j++) {
        if (const int rc = klt_find(ctx, who, ids[j], &T[j])) return klt_many_blame(ctx, rc, j, ids[j]);
        for (int i = 0; i < j; i++) REQ(ids[i] != ids[j], PMV_ERR_INVALID, "%s: tracker id %d is named twice (trackers %d and %d of the group)", who, ids[j], i, j);
        cap_max = std::max(cap_max, T[j]->cap);
    }
    REQ(out_stride >= cap_max, PMV_ERR_CAPACITY, "%s: out_stride = %d is below the largest target of the group, %d", who, out_stride, cap_max);
    // the launch-wide fields: arguments of the detector's and the refinement's one launch
    const pmv_klt_params& p0 = T[0]->p;
    for (int j = 1; j < n_trk; j++) {
        const pmv_klt_params& p = T[j]->p;
        const char* field = p.gftt.quality != p0.gftt.quality ? "gftt.quality" : p.gftt.min_dist != p0.gftt.min_dist ? "gftt.min_dist"
                          : p.gftt.block_size != p0.gftt.block_size ? "gftt.block_size" : p.gftt.use_harris != p0.gftt.use_harris ? "gftt.use_harris"
                          : p.gftt.k != p0.gftt.k ? "gftt.k" : p.subpix != p0.subpix ? "subpix" : nullptr;
        if (!field && p0.subpix) {
            const pmv_subpix_params &a = p.subpix_params, &b = p0.subpix_params;
            if (a.win_w != b.win_w || a.win_h != b.win_h || a.zero_w != b.zero_w || a.zero_h != b.zero_h || a.max_iter != b.max_iter || a.eps != b.eps) field = "subpix_params";
        }
        REQ(!field, PMV_ERR_INVALID, "%s: tracker %d of the group (id %d) differs from tracker 0 in %s, which is an argument of the group's one launch", who, j, ids[j], field);
    }
    // the slot rules of pmv_klt_step, for every tracker; then one frame size for the group
    int roi[4] = {0, 0, 0, 0}, sum_cap = 0, sum_n0 = 0;
    size_t sum_pad = 0;
    bool any_f = false;
    KltObserveBook ob{false, 0, 0};
    int lift_n0 = 0;   // the largest n0 among the trackers whose F stage takes lifted points
    for (int j = 0; j < n_trk; j++) {
        const KltTracker* t = T[j];
        ob.on = ob.on || t->obs_on;
        if (t->obs_on && t->obs.undistorted_f && t->p.reject_f && t->n >= 15) lift_n0 = std::max(lift_n0, t->n);
        int r[4], gcap;
        if (t->n > 0)
            if (const int rc = lk_check(ctx, true, prev_slots[j], cur_slots[j], out_xy, t->n, out_xy, (const uint8_t*)out_ids, out_xy)) return klt_many_blame(ctx, rc, j, ids[j]);
        if (const int rc = gftt_frame_check(ctx, who, true, cur_slots[j], nullptr, t->cap, &t->p.gftt, nullptr, 0, out_ids, t->cap, out_n, r, &gcap))
            return klt_many_blame(ctx, rc, j, ids[j]);
        if (j == 0) memcpy(roi, r, sizeof(roi));
        REQ(r[2] == roi[2] && r[3] == roi[3], PMV_ERR_INVALID, "%s: tracker %d of the group (id %d) differs from tracker 0 in the frame size of its cur_slot (%dx%d, not %dx%d)", who,
            j, ids[j], r[2], r[3], roi[2], roi[3]);
        sum_cap += t->cap; sum_n0 += t->n; sum_pad += refill_pad(t->cap);
        any_f = any_f || (t->p.reject_f && t->n >= 15);
    }
    // stage 8's LK pairs, before anything is launched: the lengths of the lists it tracks are known only on the device
    int sum_st = 0;
    for (int j = 0; right && j < n_trk; j++) {
        if (right->slots[j] < 0) continue;
        if (!T[j]->st_on) {
            set_err(ctx, "pmv_klt_step_many_stereo: tracker %d has no stereo setting (pmv_klt_set_stereo)", ids[j]);
            return klt_many_blame(ctx, PMV_ERR_INVALID, j, ids[j]);
        }
        if (const int rc = lk_check(ctx, true, cur_slots[j], right->slots[j], nullptr, 0, nullptr, nullptr, nullptr)) return klt_many_blame(ctx, rc, j, ids[j]);
        sum_st += T[j]->cap;
    }
    tl_prof = &ctx->prof; CKC(hipSetDevice(ctx->device));
    const PyrLayout& L = ctx->slot_layout[cur_slots[0]];
    const size_t n = (size_t)n_trk, pix = (size_t)ctx->max_w * ctx->max_h, rpix = (size_t)roi[2] * roi[3], mstride = (rpix + 3) & ~(size_t)3;
    REQ(n * mstride + 64 <= 0xffffffffull, PMV_ERR_CAPACITY, "%s: the group's %d masks of %zu bytes do not fit a 32-bit offset", who, n_trk, rpix);
    // the context's scratch of the refill and frame calls, one share per tracker; records and results are the group's and the trackers'
    FrameDetScratch& S = ctx->fds;
    CKC(S.lists(std::max(pix, n * rpix), n)); CKC(S.masks(std::max(pix, n * mstride) + S.PAINT_SLACK, 0)); CKC(S.refill(std::max((size_t)PMV_REFILL_MAX_TRACKS, sum_pad), n));
    const pmv_klt_params& p = p0;
    SubpixArgs SA{};
    if (p.subpix) CKC(subpix_table_ready(ctx, &p.subpix_params, &SA));
    // the group's own blocks, grown to the largest group seen
    if (!ctx->klt_group) ctx->klt_group = new KltGroup();
    KltGroup* G = ctx->klt_group;
    Carve nr, nd;
    klt_group_recs(nr, n, (size_t)sum_cap); klt_group_dev(nd, n, (size_t)sum_cap, sum_pad, (size_t)cap_max);
    hipStream_t s = ctx->s_front;
    if (nr.bytes() + 64 > G->d_rec.cap || nd.bytes() + 64 > G->d_mem.cap) CKC(hipStreamSynchronize(s));   // (nothing of an earlier call reads the old blocks)
    CKC(G->d_rec.ensure(nr.bytes() + 64)); CKC(G->h_rec.ensure(nr.bytes() + 64)); CKC(G->d_mem.ensure(nd.bytes() + 64));
    Carve cr(G->h_rec.p, G->d_rec.p, G->h_rec.cap), cd(nullptr, G->d_mem.p, G->d_mem.cap);
    const KltGroupRecs R = klt_group_recs(cr, n, (size_t)sum_cap);
    const KltGroupDev D = klt_group_dev(cd, n, (size_t)sum_cap, sum_pad, (size_t)cap_max);
    long long launches = 0, waits = 0;
    // records: per tracker its arguments, its refill request (n is written by the kernels) and its frame request; the geometry entry
    const unsigned long long pitch = ctx->cap.slot_bytes;
    *R.geom.h = L;
    size_t lk_base = 0, pad_off = 0, st_base = 0;
    bool any_pred = false;   // a tracker of the group has a pending prediction and tracks: the records carry it, and the gated launch follows
    for (int j = 0; j < n_trk; j++) {
        KltTracker* t = T[j];
        R.rrec.h[j] = RefillRec{0, t->p.radius, (int)pad_off, roi[0], roi[1], roi[2], roi[3], (unsigned)((size_t)j * mstride), 0, {0, 0, 0}};
        memcpy(R.hw.h + (size_t)j * REFILL_HW, t->R.hw.h, REFILL_HW);
        int* g = R.grec.h + (size_t)j * CELL_STRIDE;
        gftt_frame_record(g, roi, cur_slots[j], (size_t)j * rpix, nullptr, 0, nullptr, 0);
        g[5] = (int)(unsigned)((size_t)j * mstride);
        R.slots.h[j] = cur_slots[j];
        // the stage arguments, from the tracker's shares of the group's tables
        KltShares sh{};
        sh.lk = KltLkOut{D.lk_xy.d + 2 * lk_base, D.bk_xy.d + 2 * lk_base, D.lk_st.d + lk_base, D.bk_st.d + lk_base};
        sh.rf = KltRefillIn{D.pos.d + pad_off, D.prio.d + pad_off, D.flag.d + pad_off, R.rrec.d + j};
        sh.keep = D.keep.d + pad_off; sh.want = D.want.d + j; sh.m = D.m.d + j; sh.stat = D.stat.d + 2 * j;
        sh.ixy = D.ixy.d + (size_t)2 * j * cap_max; sh.sp_xy = D.sp_xy.d + (size_t)2 * j * cap_max;
        sh.prev_off = (unsigned long long)(t->n > 0 ? prev_slots[j] : cur_slots[j]) * pitch; sh.next_off = (unsigned long long)cur_slots[j] * pitch;
        sh.lk_base = (int)lk_base;
        sh.pred = D.pred.d + 2 * j; sh.pred_slot = j;
        any_pred = any_pred || (t->pr_on && t->n > 0);
        lk_base += (size_t)t->n; pad_off += refill_pad(t->cap);
        if (right) {   // stage 8: the tracker's share of the bound-sized launch
            const bool on = right->slots[j] >= 0;
            sh.stereo = true; sh.right_on = on ? 1 : 0;
            sh.st = KltLkOut{D.lk_xy.d + 2 * st_base, D.bk_xy.d + 2 * st_base, D.lk_st.d + st_base, D.bk_st.d + st_base};
            sh.right_off = (unsigned long long)(on ? right->slots[j] : cur_slots[j]) * pitch;
            sh.st_base = (int)st_base;
            if (on) st_base += (size_t)t->cap;
        }
        R.rec.h[j] = klt_stage_args(t, L, sh);
    }
    CKC(hipMemcpyAsync(G->d_rec, G->h_rec, R.front, hipMemcpyHostToDevice, s));
    // 1. track: the records are written on the device, where the positions are, and the whole group is one launch
    if (sum_n0 > 0) {
        CKC(klt_launch(k_klt_lk_records, n_trk, s, R.rec.d, D.lkb.d, D.lkx.d, any_pred ? D.lkx2.d : (LKExt*)nullptr, sum_n0));
        CKC(launch_lk_batch_ex(s, ctx->d_slots, D.lkb.d, D.lkx.d, sum_n0, R.geom.d, lk_launch_params(ctx), D.lk_xy.d, D.lk_st.d, D.lk_err.d, nullptr, D.bk_xy.d, D.bk_st.d,
                               D.bk_err.d, any_pred ? D.pred.d : nullptr, n_trk));
        launches += 2;
        if (any_pred) {   // the fall-back over the full pyramid: every workgroup of a tracker whose predicted pass had successes enough leaves at once
            CKC(launch_lk_batch_ex(s, ctx->d_slots, D.lkb.d, D.lkx2.d, sum_n0, R.geom.d, lk_launch_params(ctx), D.lk_xy.d, D.lk_st.d, D.lk_err.d, nullptr, D.bk_xy.d,
                                   D.bk_st.d, D.bk_err.d, D.pred.d, n_trk));
            launches++;
        }
    }
    // 2. filter
    CKC(klt_launch(k_klt_filter_many, n_trk, s, R.rec.d)); launches++;
    // 3. rejectWithF: the host reads every n1 (the iteration tables are libm's); one copy and one launch serve the trackers that have the stage
    int cur = 0; const int* f_run = nullptr;
    if (any_f) {
        if (lift_n0 > 0) {
            const int gx = (lift_n0 + KT - 1) / KT;
            CKC(klt_launch(k_klt_lift_f_many, n_trk * gx, s, R.rec.d, gx)); launches++; ob.lift++;
        }
        CKC(hipStreamSynchronize(s));
        waits++;
        int n_f = 0; size_t tab = 0;
        for (int j = 0; j < n_trk; j++) {
            const KltTracker* t = T[j];
            R.f_run.h[j] = 0;
            if (!(t->p.reject_f && t->n >= 15)) continue;
            const int n1 = *t->O.n1.h;
            REQ(n1 >= 0 && n1 <= t->n, PMV_ERR_HIP, "%s: the filter left n1 = %d of %d tracks (tracker %d of the group)", who, n1, t->n, j);
            if (n1 < 15) continue;
            R.fprob.h[n_f++] = klt_f_problem(t, R.rec.h[j].lift_f, n1, R.ftab.h + tab, R.ftab.d + tab);
            tab += (size_t)n1 + 2;
            R.f_run.h[j] = 1;
        }
        if (n_f > 0) {
            const size_t b0 = R.f_run.off, b1 = R.ftab.off + tab * sizeof(double);
            CKC(hipMemcpyAsync((char*)G->d_rec.p + b0, (const char*)G->h_rec.p + b0, b1 - b0, hipMemcpyHostToDevice, s));
            CKC(launch_fundamental_ransac(s, R.fprob.d, n_f));
            f_run = R.f_run.d;
            CKC(klt_launch(k_klt_compact_many, n_trk, s, R.rec.d, 0, 0, f_run));
            launches += 2; cur = 1;
        }
    }
    // 4. thin
    CKC(launch_track_refill(s, R.rrec.d, n_trk, rpix, D.pos.d, D.prio.d, D.flag.d, R.hw.d, D.keep.d, S.d_refill_kept, S.d_refill_nkept, S.d_gfr_mask));
    launches += 2;
    CKC(klt_launch(k_klt_compact_many, n_trk, s, R.rec.d, 1, cur, f_run)); launches++; cur ^= 1;
    // 5. refill: every tracker's selection takes its cap from its own word
    const GfttExt X = gftt_ext(p.gftt.block_size, p.gftt.use_harris, p.gftt.k);
    CKC(launch_gftt_frame(s, ctx->d_slots, L, R.grec.d, n_trk, gftt_frame_grid_x(roi[2], roi[3]), cap_max, p.gftt.quality, p.gftt.min_dist, 0, &X, S.d_gfr_mask.get(),
                          S.d_gfr_val, S.d_gfr_idx, S.d_gfr_info, S.d_gfr_keys, D.ixy.d, D.m.d, D.stat.d, D.want.d));
    launches += 2;
    // 6. refine
    if (p.subpix) {
        CKC(launch_corner_subpix_dev(s, ctx->d_slots, L, D.ixy.d, 0, cap_max, D.m.d, ctx->d_subpix_tab, SA, D.sp_xy.d, D.sp_it.d, D.sp_fl.d, R.slots.d, n_trk));
        launches++;
    }
    // 7. append: every workgroup stores its tracker's completion word last
    CKC(klt_launch(k_klt_append_many, n_trk, s, R.rec.d, cur, f_run)); launches++;
    // 8. stereo: the records of every share from the lists and counts the append left, one LK launch over the sum of the bounds (a record
    // beyond its list's count is void), then the rule; every workgroup of it stores its tracker's stereo completion word last
    if (right) {
        if (sum_st > 0) {
            CKC(klt_launch(k_klt_stereo_records, n_trk, s, R.rec.d, D.lkb.d, D.lkx.d, sum_st));
            CKC(launch_lk_batch_ex(s, ctx->d_slots, D.lkb.d, D.lkx.d, sum_st, R.geom.d, lk_launch_params(ctx), D.lk_xy.d, D.lk_st.d, D.lk_err.d, nullptr, D.bk_xy.d, D.bk_st.d,
                                   D.bk_err.d));
            launches += 2;
        }
        CKC(klt_launch(k_klt_stereo_many, n_trk, s, R.rec.d)); launches++;
    }
    // 9. observe: one workgroup per tracker; those of the trackers with the setting store their observe completion word last
    if (ob.on) { CKC(klt_launch(k_klt_observe_many, n_trk, s, R.rec.d, cur)); launches++; ob.observe++; }
    CKC(hipStreamSynchronize(s));
    waits++;
    for (int j = 0; j < n_trk; j++)
        if (const int rc = klt_result_check(ctx, T[j], right != nullptr, who, j)) return rc;
    for (int j = 0; j < n_trk; j++) {
        const size_t o = (size_t)j * out_stride;
        const KltRightOut r{right ? right->slots[j] : -1, right ? right->xy + 2 * o : nullptr, right ? right->st + o : nullptr};
        klt_result_copy(T[j], out_ids + o, out_ages + o, out_xy + 2 * o, out_prev_xy_or_null ? out_prev_xy_or_null + 2 * o : nullptr, out_n + j, out_counts8 + 8 * j,
                        right ? &r : nullptr);
    }
    klt_book(ctx, roi, n_trk, right != nullptr, waits, launches, ob);
    return PMV_OK;
}

extern "C" {

int pmv_klt_step_many(pmv_ctx* ctx, int n_trk, const int* ids, const int* prev_slots, const int* cur_slots, int* out_ids, int* out_ages, float* out_xy,
                      float* out_prev_xy_or_null, int out_stride, int* out_n, int* out_counts8) {
    return klt_step_many_run(ctx, n_trk, ids, prev_slots, cur_slots, out_ids, out_ages, out_xy, out_prev_xy_or_null, out_stride, out_n, out_counts8, nullptr);
}

int pmv_klt_step_many_stereo(pmv_ctx* ctx, int n_trk, const int* ids, const int* prev_slots, const int* cur_slots, const int* right_slots, int* out_ids, int* out_ages,
                             float* out_xy, float* out_prev_xy_or_null, float* out_right_xy, uint8_t* out_right_status, int out_stride, int* out_n, int* out_counts8) {
    const KltRightManyOut right{right_slots, out_right_xy, out_right_status};
    return klt_step_many_run(ctx, n_trk, ids, prev_slots, cur_slots, out_ids, out_ages, out_xy, out_prev_xy_or_null, out_stride, out_n, out_counts8, &right);
}

int pmv_klt_set_observe(pmv_ctx* ctx, int id, const pmv_klt_observe_params* p_or_null) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_set_observe: null argument");
    KltTracker* t;
    if (const int rc = klt_find(ctx, "pmv_klt_set_observe", id, &t)) return rc;
    if (!p_or_null) { t->obs_on = false; return PMV_OK; }
    const pmv_klt_observe_params& p = *p_or_null;
    const LiftCam* cam = camera_entry(ctx, p.cam_id);
    REQ(cam, PMV_ERR_INVALID, "pmv_klt_set_observe: cam_id = %d: the camera does not exist (pmv_camera_create)", p.cam_id);
    const LiftCam* rcam = p.right_cam_id == -1 ? nullptr : camera_entry(ctx, p.right_cam_id);
    REQ(p.right_cam_id == -1 || rcam, PMV_ERR_INVALID, "pmv_klt_set_observe: right_cam_id = %d is neither -1 nor a camera (pmv_camera_create)", p.right_cam_id);
    REQ(std::isfinite(p.dt) && p.dt > 0.0, PMV_ERR_INVALID, "pmv_klt_set_observe: dt = %g is not finite or not above 0", p.dt);
    REQ(p.undistorted_f == 0 || p.undistorted_f == 1, PMV_ERR_INVALID, "pmv_klt_set_observe: undistorted_f = %d is neither 0 nor 1", p.undistorted_f);
    REQ(!p.undistorted_f || (std::isfinite(p.f_focal) && p.f_focal > 0.0), PMV_ERR_INVALID, "pmv_klt_set_observe: f_focal = %g is not finite or not above 0", p.f_focal);
    t->obs = p; t->obs_on = true; t->obs_cam = cam; t->obs_rcam = rcam;
    return PMV_OK;
}

int pmv_klt_get_observe(pmv_ctx* ctx, int id, pmv_klt_observe_params* out, int* out_on) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_get_observe: null argument");
    KltTracker* t;
    if (const int rc = klt_find(ctx, "pmv_klt_get_observe", id, &t)) return rc;
    REQ(out && out_on, PMV_ERR_INVALID, "pmv_klt_get_observe: null argument");
    *out = t->obs; *out_on = t->obs_on ? 1 : 0;
    return PMV_OK;
}

// a host copy out of the tracker's result block: no device work
int pmv_klt_get_observations(pmv_ctx* ctx, int id, float* out_un_xy, float* out_vel, uint8_t* out_ok, float* out_right_un_xy_or_null, uint8_t* out_right_ok_or_null, int cap,
                             int* out_n) {
    REQ(ctx, PMV_ERR_INVALID, "pmv_klt_get_observations: null argument");
    KltTracker* t;
    if (const int rc = klt_find(ctx, "pmv_klt_get_observations", id, &t)) return rc;
    REQ(out_un_xy && out_vel && out_ok && out_n, PMV_ERR_INVALID, "pmv_klt_get_observations: null argument");
    REQ(t->obs_state != 0, PMV_ERR_INVALID, "pmv_klt_get_observations: tracker %d has not stepped since pmv_klt_create or pmv_klt_set_tracks", id);
    REQ(t->obs_state == 2, PMV_ERR_INVALID, "pmv_klt_get_observations: the last step of tracker %d ran with the observation setting off (pmv_klt_set_observe)", id);
    const int n = t->n;
    REQ(cap >= n, PMV_ERR_CAPACITY, "pmv_klt_get_observations: cap = %d is below the %d tracks of the last step", cap, n);
    const KltRes& O = t->O;
    memcpy(out_un_xy, O.un_xy.h, (size_t)n * 8);
    memcpy(out_vel, O.vel.h, (size_t)n * 8);
    memcpy(out_ok, O.un_ok.h, (size_t)n);
    if (t->obs_right) {
        if (out_right_un_xy_or_null) memcpy(out_right_un_xy_or_null, O.right_un.h, (size_t)n * 8);
        if (out_right_ok_or_null) memcpy(out_right_ok_or_null, O.right_un_ok.h, (size_t)n);
    } else if (out_right_ok_or_null) memset(out_right_ok_or_null, 0, (size_t)n);
    *out_n = n;
    return PMV_OK;
}

int pmv_debug_klt_observe_stats(pmv_ctx* ctx, long long* out4) {
    REQ(ctx && out4, PMV_ERR_INVALID, "pmv_debug_klt_observe_stats: null argument");
    for (int i = 0; i < 4; i++) out4[i] = ctx->klt_observe_stats[i].load();
    return PMV_OK;
}

int pmv_debug_klt_stereo_stats(pmv_ctx* ctx, long long* out4) {
    REQ(ctx && out4, PMV_ERR_INVALID, "pmv_debug_klt_stereo_stats: null argument");
    for (int i = 0; i < 4; i++) out4[i] = ctx->klt_stereo_stats[i].load();
    return PMV_OK;
}

int pmv_debug_klt_many_stats(pmv_ctx* ctx, long long* out4) {
    REQ(ctx && out4, PMV_ERR_INVALID, "pmv_debug_klt_many_stats: null argument");
    for (int i = 0; i < 4; i++) out4[i] = ctx->klt_many_stats[i].load();
    return PMV_OK;
}

int pmv_debug_klt_stats(pmv_ctx* ctx, long long* out4) {
    REQ(ctx && out4, PMV_ERR_INVALID, "pmv_debug_klt_stats: null argument");
    for (int i = 0; i < 3; i++) out4[i] = ctx->klt_stats[i].load();
    std::lock_guard<std::mutex> lk(ctx->klt_mu);
    long long alive = 0;
    for (const auto* t : ctx->klt) alive += t != nullptr;
    out4[3] = alive;
    return PMV_OK;
}

}  // extern "C"
