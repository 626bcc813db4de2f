// Who lays out what in the back-end's staging blocks: ONE function per call kind. A call's in-block sits at the start of the workspace
// set's mapped pinned block (h_stage) and is mirrored at the same offsets in the device block named below; its out-block follows in h_stage
// at the next multiple of 64 bytes and is written by the kernels through the mapped alias. *_prepare, *_finish, the completion-word
// accessors and the single calls take every offset from the layout value; backend_caps evaluates the same functions at capacity for
// backend_alloc. Host-only and pure C++ (tests/twin/block_layout_check.cpp compiles it alone).
#pragma once
#include "pmv_block.h"

namespace pmv {

constexpr int MAX_HYP = 1024;      // PnP hypotheses per call at most
constexpr int FP_MAX_HYP = 64;     // five-point hypotheses per round at most
constexpr size_t PNP_HDR = 384;    // bytes: K (10 doubles) + 33 powers of ten + padding
constexpr size_t ESS_HDR = 64;     // bytes: the problem record in front of a whole-RANSAC request's input block

// ---- result-block headers the kernels write (device code names these offsets) ----
struct PnPResultHdr { double rt[6]; int info[3]; unsigned done; };   // info: inlier count, LM passes + 1, unused; the inlier list follows
constexpr size_t PNP_OUT_INFO = offsetof(PnPResultHdr, info), PNP_OUT_DONE = offsetof(PnPResultHdr, done), PNP_OUT_INLIERS = sizeof(PnPResultHdr);
static_assert(PNP_OUT_INFO == 48 && PNP_OUT_DONE == 60 && PNP_OUT_INLIERS == 64, "the PnP result block is [rt 48 | info 16 | inliers]");
struct WholeResultHdr { double M[9]; double pad0; int found, samples_drawn, best_count; unsigned done; char pad1[32]; };   // E or F; the mask follows
constexpr size_t ESS_OUT_INFO = offsetof(WholeResultHdr, found), ESS_OUT_DONE = offsetof(WholeResultHdr, done), ESS_OUT_HDR = sizeof(WholeResultHdr);
static_assert(ESS_OUT_INFO == 80 && ESS_OUT_DONE == 92 && ESS_OUT_HDR == 128, "the whole-RANSAC result block is [M 72 | .. | info at 80 | mask at 128]");
constexpr int BA_SUM_SLOTS = 8, BA_SUM_DONE = 7;   // BA summary: 8 doubles in front of [cams | pts]; the low word of slot 7 is the completion word

// ---- pmv_pnp_ransac: d_pnp_in mirrors the in-block; the out-block has d_pnp_out's layout ----
struct PnPLayout { size_t K, obj, img, samples, in_bytes, out, info, done, inliers, total; };
inline PnPLayout pnp_layout(size_t m, size_t iterations) {
    Carve c; PnPLayout L;
    L.K = c.take<char>(PNP_HDR).off; L.obj = c.take<float>(3 * m).off; L.img = c.take<float>(2 * m).off; L.samples = c.take<int>(5 * iterations).off;
    L.in_bytes = c.bytes();
    L.out = c.take<PnPResultHdr>(1, 64).off; L.info = L.out + PNP_OUT_INFO; L.done = L.out + PNP_OUT_DONE;
    L.inliers = c.take<int>(m).off;
    L.total = c.bytes();
    return L;
}
// ---- pmv_ba_solve: d_ba_io mirrors the whole block; the result [summary | cams | pts] comes back at its start ----
struct BaIoLayout { size_t summary, cams, pts, obs, K, cam_idx, pt_idx, pstart, plist, cstart, clist, erec, io_bytes, done, out_bytes, total; };
inline BaIoLayout ba_io_layout(size_t nc, size_t np, size_t n_obs) {
    Carve c; BaIoLayout L;
    L.summary = c.take<double>(BA_SUM_SLOTS).off; L.cams = c.take<double>(6 * nc).off; L.pts = c.take<double>(3 * np).off;
    L.out_bytes = c.bytes();
    L.obs = c.take<double>(2 * n_obs).off; L.K = c.take<double>(10).off;
    L.cam_idx = c.take<int>(n_obs).off; L.pt_idx = c.take<int>(n_obs).off;
    L.pstart = c.take<int>(np + 1).off; L.plist = c.take<int>(n_obs).off; L.cstart = c.take<int>(nc + 1).off; L.clist = c.take<int>(n_obs).off;
    L.erec = c.take<int>(4 * n_obs, 16).off;   // 16-byte records (observation, camera, point, dup flag)
    L.io_bytes = L.total = c.bytes();
    L.done = L.summary + BA_SUM_DONE * sizeof(double);
    return L;
}
// ---- pmv_triangulate_candidates: d_tri_in mirrors the in-block; out-block [Q 16n doubles | mask 4n bytes] ----
struct DltLayout { size_t P, q1, q2, mask_in, in_bytes, out, Q, mask, total; };
inline DltLayout dlt_layout(size_t n) {
    Carve c; DltLayout L;
    L.P = c.take<double>(48).off; L.q1 = c.take<double>(2 * n).off; L.q2 = c.take<double>(2 * n).off; L.mask_in = c.take<uint8_t>(n).off;
    L.in_bytes = c.bytes();
    L.out = L.Q = c.take<double>(16 * n, 64).off; L.mask = c.take<uint8_t>(4 * n).off;
    L.total = c.bytes();
    return L;
}
// ---- pmv_fivepoint_hypotheses: d_tri_in mirrors the in-block; out-block [models 90 n_hyp doubles | n_models n_hyp | counts 10 n_hyp ints] ----
struct FivePointLayout { size_t q1, q2, samples, in_bytes, out, models, n_models, counts, total; };
inline FivePointLayout fivepoint_layout(size_t n, size_t n_hyp) {
    Carve c; FivePointLayout L;
    L.q1 = c.take<double>(2 * n).off; L.q2 = c.take<double>(2 * n).off; L.samples = c.take<int>(5 * n_hyp).off;
    L.in_bytes = c.bytes();
    L.out = L.models = c.take<double>(90 * n_hyp, 64).off; L.n_models = c.take<int>(n_hyp).off; L.counts = c.take<int>(10 * n_hyp).off;
    L.total = c.bytes();
    return L;
}
// ---- pmv_find_essential_mat (points: doubles, d_ess_in) and pmv_find_fundamental_mat (points: floats, d_fund_in): in-block
// [problem record ESS_HDR | p1 2n | p2 2n | iteration table n + 2 doubles], out-block [WholeResultHdr | mask n bytes] ----
struct WholeLayout { size_t rec, p1, p2, iters, in_bytes, out, info, done, mask, total; };
template <class Pt> inline WholeLayout whole_layout(size_t n) {
    Carve c; WholeLayout L;
    L.rec = c.take<char>(ESS_HDR).off; L.p1 = c.take<Pt>(2 * n).off; L.p2 = c.take<Pt>(2 * n).off; L.iters = c.take<double>(n + 2).off;
    L.in_bytes = c.bytes();
    L.out = c.take<WholeResultHdr>(1, 64).off; L.info = L.out + ESS_OUT_INFO; L.done = L.out + ESS_OUT_DONE;
    L.mask = c.take<uint8_t>(n).off;
    L.total = c.bytes();
    return L;
}
inline WholeLayout essential_layout(size_t n) { return whole_layout<double>(n); }
inline WholeLayout fundamental_layout(size_t n) { return whole_layout<float>(n); }
// ---- pmv_triangulate_tracks: d_tt_in mirrors the in-block [problem record TT_HDR | P 12 nc | camera centres 3 nc | observations re-ordered
// into per-landmark runs: xy 2 n_obs doubles, cameras n_obs ints | run starts np + 1 ints | the workgroup counter, zero], out-block
// [completion word in TT_OUT_HDR bytes | xyz 3 np | err np doubles | status np bytes] (the kernel derives the three tables from np) ----
constexpr size_t TT_HDR = 128;        // bytes: the problem record in front of the input block
constexpr size_t TT_OUT_HDR = 64, TT_OUT_DONE = 0;
struct TriTracksLayout { size_t rec, P, C, obs, cam, start, counter, in_bytes, out, done, xyz, err, status, total; };
inline TriTracksLayout tri_tracks_layout(size_t nc, size_t np, size_t n_obs) {
    Carve c; TriTracksLayout L;
    L.rec = c.take<char>(TT_HDR).off; L.P = c.take<double>(12 * nc).off; L.C = c.take<double>(3 * nc).off; L.obs = c.take<double>(2 * n_obs).off;
    L.cam = c.take<int>(n_obs).off; L.start = c.take<int>(np + 1).off; L.counter = c.take<unsigned>(4, 16).off;
    L.in_bytes = c.bytes();
    L.out = c.take<char>(TT_OUT_HDR, 64).off; L.done = L.out + TT_OUT_DONE;
    L.xyz = c.take<double>(3 * np).off; L.err = c.take<double>(np).off; L.status = c.take<uint8_t>(np).off;
    L.total = c.bytes();
    return L;
}

// ---- the blocks' sizes: the layouts at capacity plus the slack terms the allocation always had ----
constexpr size_t BLOCK_SLACK = 64;   // behind every device block: the 16-byte granules of the stage-in copies may read past the last field
inline size_t fund_in_cap(size_t max_tracks) { return fundamental_layout(max_tracks).in_bytes + BLOCK_SLACK; }   // d_fund_in, made lazily (fundamental_prepare)
struct BackendCaps { size_t ba_io, pnp_in, pnp_out, tri_in, tri_out, ess_in, fund_in, h_stage, tt_in; };
inline BackendCaps backend_caps(int max_tracks, int max_ba_cams, int max_ba_points, int max_ba_obs) {
    constexpr size_t SLACK = BLOCK_SLACK;
    const size_t mt = (size_t)max_tracks;
    const size_t nc = (size_t)(max_ba_cams > 1 ? max_ba_cams : 1), np = (size_t)(max_ba_points > 1 ? max_ba_points : 1), no = (size_t)(max_ba_obs > 1 ? max_ba_obs : 1);
    const size_t n = 6 * nc + 3 * np;
    auto max2 = [](size_t a, size_t b) { return a > b ? a : b; };
    const PnPLayout pnp = pnp_layout(mt, MAX_HYP);
    const DltLayout dlt = dlt_layout(mt);
    const FivePointLayout fp = fivepoint_layout(mt, FP_MAX_HYP);
    const WholeLayout ess = essential_layout(mt);
    const TriTracksLayout tt = tri_tracks_layout(nc, np, no);   // (every table grows with its own count: the largest is at the maxima)
    BackendCaps C;
    // the io block keeps the formula it always had: 24 bytes of index slack and 128 behind it more than ba_io_layout(nc, np, no).total needs
    // (the layout's alignment gap in front of the 16-byte records is at most 12 of them)
    C.ba_io = (8 + nc * 6 + np * 3 + no * 2 + 10) * 8 + (no * 8 + np + nc + 8) * 4 + 128;
    C.pnp_in = pnp.in_bytes + SLACK;
    C.pnp_out = pnp.total - pnp.out + SLACK;
    // d_tri_in serves the DLT and the five-point round. Sized by the DLT alone (as it was up to here) it is too small for a five-point round
    // of FP_MAX_HYP samples over max_tracks points wherever max_tracks < 832, and such a call was refused; above that the DLT's size governs.
    C.tri_in = max2(dlt.in_bytes, fp.in_bytes) + SLACK;
    C.tri_out = dlt.total - dlt.out + SLACK;
    C.ess_in = ess.in_bytes + SLACK;
    C.fund_in = fund_in_cap(mt);
    C.tt_in = tt.in_bytes + SLACK;
    // the staging block holds the largest in + out pair of any call. The first three terms are older than the single-copy blocks and no
    // layout needs them today; they stay because the block's size stays.
    const size_t pairs[] = {no * 18 * 8 + no * 2 * 8, n * 8 + no * 32 + (np + nc + 2) * 4, mt * 32 + MAX_HYP * 20 + 4096,
                            C.ba_io, C.pnp_in + C.pnp_out, C.tri_in + C.tri_out,
                            C.tri_in + (fp.total - fp.out) + 256,           // five-point round in + out
                            C.ess_in + (ess.total - ess.out) + SLACK,       // whole findEssentialMat in + out (findFundamentalMat's is smaller)
                            tt.total + SLACK};                              // N-view triangulation in + out
    C.h_stage = 0;
    for (size_t v : pairs) C.h_stage = max2(C.h_stage, v);
    return C;
}

}  // namespace pmv
