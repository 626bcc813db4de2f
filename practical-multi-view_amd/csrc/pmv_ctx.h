// Internal context definition shared by the C-ABI translation units.
#pragma once
#include <atomic>
#include "pmv_device.h"
#include "pmv_mem.h"
#include "pmv_block.h"
#include "pmv_prof.h"
#include "pmv_lift.h"
#include "../../include/pmv_hip.h"
#include <algorithm>
#include <utility>
#include <vector>
#include <mutex>

namespace pmv {
struct BatchEngine;                 // multi-sequence combiners (batch_engine.hip)
struct BatchSession;                // plugin-level callers of the engine: pmv_batch_open .. pmv_batch_close (batch_session.hip)
struct BatchIngest;                 // the feeder: background pyramid builds of frame slots, from host memory or in place (ingest_batch.hip)
// what a frame slot holds (pmv_ctx::slot_state); written only while the slot has no reader: by the synchronous calls, and by the feeder
// before the sequences it serves start and after they end
enum SlotState : uint8_t { SLOT_EMPTY = 0, SLOT_STAGED, SLOT_BUILT };   // SLOT_STAGED: level 0 only (pmv_frames_stage)
constexpr int MAX_CELLS = 64;       // 1920x1080 -> 8x5 = 40 cells of 255x255
constexpr int MAX_PER_CELL = 4096;    // also the capacity of an "unlimited" (max_per_cell <= 0) goodFeaturesToTrack call
struct BackendBuffers;              // PnP / BA device workspaces (backend.hip)
struct KltTracker;                  // a device-resident KLT tracker (frontend_klt.hip)
struct KltGroup;                    // what a pmv_klt_step_many call keeps in the context (frontend_klt.hip)

// The scratch of the launches that serve whole-frame detector requests (launch_gftt_frame) and the refill in front of them
// (launch_track_refill): one per owner - the context for its single calls and its KLT steps (GROW_EXACT), the engine's detector combiner for
// its rounds (GROW_SLACK). A launch serves n_req requests; every part is made by the first caller that asks for it and grown to the largest
// launch seen. h_gfr, h_refill: the launch's gftt_frame_block and refill_block (mapped pinned, carved below). d_gfr_val, _idx: the record
// lists (value, pixel index); _keys: the key list of the selection's slower path; _info: one (maximum, count) pair per request. d_gfr_mask:
// the regions' packed masks, where the refill paints them and pass 1 reads them; h_gfr_mask: the host's mirror (`mirror`: pinned where a
// copy call reads it, mapped in the engine, whose scratch is of one kind). d_refill_kept, _nkept: k_track_select's kept lists and counts.
struct FrameDetScratch {
    Buf<uint8_t> h_gfr, h_refill, d_gfr_mask, h_gfr_mask;
    Buf<float> d_gfr_val; Buf<unsigned> d_gfr_idx, d_gfr_info, d_refill_kept; Buf<unsigned long long> d_gfr_keys; Buf<int> d_refill_nkept;
    static constexpr size_t PAINT_SLACK = 64;   // asked for behind a painted mask's regions: a dword of the painting may end behind a region's last byte
    static constexpr size_t BLOCK_SLACK = 64;   // behind a mapped block: the carvers align their parts
    FrameDetScratch(MemGrow g, MemKind mirror) : h_gfr(MEM_MAPPED, g), h_refill(MEM_MAPPED, g), d_gfr_mask(MEM_DEVICE, g), h_gfr_mask(mirror, g), d_gfr_val(MEM_DEVICE, g),
        d_gfr_idx(MEM_DEVICE, g), d_gfr_info(MEM_DEVICE, g), d_refill_kept(MEM_DEVICE, g), d_gfr_keys(MEM_DEVICE, g), d_refill_nkept(MEM_DEVICE, g) {}
    // in front of launch_gftt_frame. entries: the pixels of the launch's regions - a flat positive plateau makes every pixel a record, so no
    // smaller list is safe; the context passes at least max_w * max_h, so that its single calls allocate once. block_bytes: the bytes of the
    // launch's gftt_frame_block, 0 when the caller keeps records and results in buffers of its own (the KLT steps).
    hipError_t lists(size_t entries, size_t n_req, size_t block_bytes = 0) {
        hipError_t e = block_bytes ? h_gfr.ensure(block_bytes + BLOCK_SLACK) : hipSuccess;
        if (!e) e = d_gfr_val.ensure(entries * sizeof(float)); if (!e) e = d_gfr_idx.ensure(entries * sizeof(unsigned));
        if (!e) e = d_gfr_keys.ensure(entries * sizeof(unsigned long long));
        return e ? e : d_gfr_info.ensure(n_req * 2 * sizeof(unsigned));
    }
    // in front of a launch that reads a mask. device_bytes: the packed regions, uploaded or painted (then + PAINT_SLACK); host_mirror_bytes:
    // what the caller packs on the host - 0 without a host mask, and a call without one makes no mirror
    hipError_t masks(size_t device_bytes, size_t host_mirror_bytes) {
        const hipError_t e = d_gfr_mask.ensure(device_bytes);
        return e ? e : h_gfr_mask.ensure(host_mirror_bytes);
    }
    // in front of launch_track_refill. kept_entries: the track entries of the launch (the sum of the requests' refill_pad(n)); the context
    // passes at least PMV_REFILL_MAX_TRACKS, the most a single request holds. block_bytes: of the launch's refill_block, as for lists().
    hipError_t refill(size_t kept_entries, size_t n_req, size_t block_bytes = 0) {
        hipError_t e = block_bytes ? h_refill.ensure(block_bytes + BLOCK_SLACK) : hipSuccess;
        if (!e) e = d_refill_kept.ensure(kept_entries * sizeof(unsigned));
        return e ? e : d_refill_nkept.ensure(n_req * sizeof(int));
    }
};
}

// In-memory log of the back-end plugin calls (pmv_record_*): every pmv_pnp_ransac / pmv_ba_solve / pmv_triangulate_candidates
// call made while recording is on leaves one self-describing blob (layout: include/pmv_hip.h) with its inputs AND outputs, so a
// test can replay exactly the calls a pipeline run made through another implementation. Back-end thread only.
struct pmv_call_log {
    bool on = false;
    std::mutex mu;                          // several back-end threads log in batch mode
    std::vector<std::vector<char>> blobs;
    static void put(std::vector<char>& b, const void* p, size_t n) { const char* c = (const char*)p; b.insert(b.end(), c, c + n); }
};

struct pmv_ctx {
    int device = 0;
    int max_w = 0, max_h = 0, n_slots = 0, max_tracks = 0, max_ba_cams = 0, max_ba_points = 0, max_ba_obs = 0;
    hipStream_t s_front = nullptr, s_back = nullptr;
    pmv::PyrLayout cap;                       // geometry of the largest frame; cap.slot_bytes = slot pitch
    std::vector<pmv::PyrLayout> slot_layout;  // per slot: geometry of the frame it holds ...
    std::vector<uint8_t> slot_state;          // ... and what of it is there (pmv::SlotState)
    pmv::Buf<uint8_t> d_slots;                // cap >= cap.slot_bytes * n_slots; grows when pmv_set_lk_params asks for a deeper pyramid
    // Geometry table of the batched launches (pmv_device.h): one PyrLayout per distinct frame size of the current batched run, slot_bytes =
    // the capacity pitch; host mirror and device copy. Rewritten by run_batch before its feeder and sequence threads start (the context is
    // synchronised there); during the run it is only read - by the combiners and the feeder on the host, by the kernels through scalar loads.
    static constexpr int MAX_GEOM = 256;      // (a batch has at most 256 sequences)
    std::vector<pmv::PyrLayout> geom;
    pmv::Buf<pmv::PyrLayout> d_geom;
    int geom_index(int w, int h) const { for (size_t i = 0; i < geom.size(); i++) if (geom[i].w[0] == w && geom[i].h[0] == h) return (int)i; return -1; }
    // launches of the batched legs since the context was created: k_lk_batch, k_knn_round (combiners), k_pad_level0[_bgr], k_pyrdown (feeder of
    // pmv_pipeline_run_batch[_streamed]) - pmv_debug_batch_launches; the profiler's per-class event pools are not made for two LK lanes
    std::atomic<long long> batch_launches[4];
    // rounds of whole-RANSAC requests the five-point combiner has served since the context was created (pmv_debug_whole_rounds):
    // k_fundamental_ransac launches, k_essential_ransac launches, rounds that made both
    std::atomic<long long> whole_rounds[3];
    // k_homography_ransac launches since the context was created and the requests they served (pmv_debug_homography_launches)
    std::atomic<long long> homography_launches[2];
    // k_tri_tracks / k_tri_tracks_batch launches since the context was created and the requests they served (pmv_debug_tri_tracks_launches)
    std::atomic<long long> tri_tracks_launches[2];
    // landing area of the synchronous calls' host frames on their way into the slots: TIGHT_FRAMES tight gray frames, or a third as many BGR ones (H2D copies are contiguous; k_pad_level0 takes
    // level 0 from here). A 2-D copy straight into the padded level is a DMA per image row: 128 x 1101 frames did not finish in 200 s.
    static constexpr int TIGHT_FRAMES = 64;
    pmv::Buf<uint8_t> d_tight;
    // LK
    pmv::Buf<float> d_prev_xy, d_out_xy, d_err;
    pmv::Buf<uint8_t> d_status;
    pmv::Buf<float> h_prev_xy, h_out_xy, h_err;  // h_out_xy, h_status, h_err: mapped pinned, the kernels write the results through .dm()
    pmv::Buf<uint8_t> h_status;
    pmv::Buf<int> h_knn, d_knn;                  // kNN matcher coordinates: [src 2n | cmp 2m] ints, 2 * max_tracks pairs
    pmv::Buf<unsigned long long> d_lk_stamps;    // diagnostic (PMV_LK_STAMPS=1), made by the first LK call that finds it set
    pmv::Buf<uint16_t> h_work;                   // per-track LK work of pmv_lk_track (mapped pinned, see launch_lk)
    // pmv_lk_track_ex / _fb: the extra inputs and outputs, one mapped pinned block made by the first such call (a context that never makes
    // one pays nothing): [initial flow 2 nt floats | back positions 2 nt floats | back err nt floats | back status nt bytes], nt = max_tracks
    pmv::Buf<uint8_t> h_lkx{pmv::MEM_MAPPED};
    std::atomic<unsigned long long> lk_work[3];  // host-side sums: LK iterations, level passes, tracks (pmv_lk_counters)
    void add_lk_work(const uint16_t* w, size_t n) { unsigned long long it = 0, lv = 0; for (size_t i = 0; i < n; i++) { it += w[i] & 0xffu; lv += w[i] >> 8; } lk_work[0] += it; lk_work[1] += lv; lk_work[2] += n; }
    // detectors
    pmv::Buf<int> d_cells;
    pmv::Buf<int> h_cells;    // pinned staging of the device cell records
    pmv::Buf<double> d_eig;
    pmv::Buf<void> d_cellmax;
    pmv::Buf<unsigned> d_spill;    // detector candidates beyond the LDS lists: MAX_CELLS * CELL_PIX pixel indices
    pmv::Buf<int> d_det_xy, d_det_count, d_flags;
    pmv::Buf<double> d_det_score;
    pmv::Buf<int> h_det_xy, h_det_count;
    pmv::Buf<double> h_det_score;
    // pmv_detect_gftt_ex: the cells' mask sub-views, packed tightly one after the other by the host (pinned) and copied to HBM - only the
    // bytes under the cells cross the bus. MAX_CELLS * CELL_PIX bytes each, made by the first extended call with a mask.
    pmv::Buf<uint8_t> h_gmask{pmv::MEM_PINNED}, d_gmask;
    int gftt_general = 0;                // pmv_debug_gftt_general
    // pmv_detect_gftt_frame, pmv_detect_gftt_refill and stages 4 and 5 of the pmv_klt_step* calls: their scratch, rewritten by every call
    pmv::FrameDetScratch fds{pmv::GROW_EXACT, pmv::MEM_PINNED};
    // pmv_debug_gftt_frame_stats: frame calls served by the single entry point | session rounds with a frame request | launch pairs made for
    // them | records above the threshold in the last request served | of those kept off-chip
    std::atomic<long long> gftt_frame_stats[5];
    int refill_last[2] = {0, 0};         // width and height of the region of the last single refill call (pmv_debug_refill_mask)
    // pmv_debug_refill_stats: single refill calls | session rounds with a refill request | select + paint launch pairs made for them | bytes of
    // mask copied host -> device by refill calls (base masks only)
    std::atomic<long long> refill_stats[4];
    // pmv_corner_subpix, made by the first call (a context that never makes one pays nothing): one mapped pinned block [point records nt x 16 |
    // positions 2 nt floats | updates nt bytes | flags nt bytes], nt = max_tracks, and the weight table in HBM with the window and (effective)
    // zero zone it was computed for - a caller keeps its parameters, so the table crosses the bus once
    pmv::Buf<uint8_t> h_subpix{pmv::MEM_MAPPED};
    pmv::Buf<float> d_subpix_tab, h_subpix_tab{pmv::MEM_PINNED};
    int subpix_tab_key[4] = {0, 0, 0, 0};
    // pmv_debug_subpix_launches: launches of the single call | session rounds with a subpix request | launches made for them
    std::atomic<long long> subpix_launches[3];
    // pmv_frames_clahe, made by the first call (a context that never makes one pays nothing): a chunk's frame records and the geometry table
    // they index, [ClaheRec x CLAHE_CHUNK | PyrLayout x CLAHE_CHUNK], in pinned host memory and in HBM, and the chunk's LUT blocks in HBM. The
    // table is the call's own: the context's geometry table belongs to a session or a batched run, and this call stays legal beside a session.
    static constexpr int CLAHE_CHUNK = 64;   // frames per pair of launches: the scratch is sized by this, not by the call's n
    pmv::Buf<uint8_t> h_clahe{pmv::MEM_PINNED}, d_clahe, d_clahe_lut;
    // pmv_debug_clahe_launches: LUT + apply launch pairs of pmv_frames_clahe | session upload rounds with a CLAHE request | launch pairs made for them
    std::atomic<long long> clahe_launches[3];
    // pmv_remap_map_create: at most MAX_REMAP_MAPS packed maps (remap_pack's layout, pmv_device.h) in HBM, one per camera; id = index. remap_mu
    // guards the table: a session's callers look a map up while another thread may create one (destroy is refused while a session is open).
    static constexpr int MAX_REMAP_MAPS = 16;
    struct RemapMap { int w = 0, h = 0; const uint8_t* d = nullptr; };   // what a caller of remap_check takes away
    RemapMap remap_maps[MAX_REMAP_MAPS];
    pmv::Buf<uint8_t> remap_mem[MAX_REMAP_MAPS];   // the storage behind remap_maps[i].d
    std::mutex remap_mu;
    // pmv_frames_remap, made by the first call: a chunk's tables [RemapRec x REMAP_CHUNK | PyrListEntry x REMAP_CHUNK | PyrLayout x REMAP_CHUNK]
    // in pinned host memory and in HBM (the call's own geometry table, as for pmv_frames_clahe), and the chunk's tight destination frames in
    // HBM: REMAP_CHUNK blocks of remap_frame_bytes(max_w, max_h), not sized by the call's n
    static constexpr int REMAP_CHUNK = 64;
    pmv::Buf<uint8_t> h_remap{pmv::MEM_PINNED}, d_remap, d_remap_scratch;
    // pmv_debug_remap_launches: k_remap launches of pmv_frames_remap | session upload rounds with a remap request | k_remap launches made for them
    std::atomic<long long> remap_launches[3];
    // pmv_klt_create (frontend_klt.hip): the trackers of the context, id = index; each owns its state and its chain's buffers. klt_mu guards
    // the table. pmv_debug_klt_stats: steps | host waits inside steps | kernel launches inside steps
    pmv::KltTracker* klt[PMV_KLT_MAX_TRACKERS] = {};
    std::mutex klt_mu;
    std::atomic<long long> klt_stats[3];
    // pmv_klt_step_many: the group's record block, its shares of per-launch tables and its argument records, made by the first many-call and
    // grown to the largest group seen (freed by klt_destroy_all). pmv_debug_klt_many_stats: many-calls | trackers stepped by them | host
    // waits inside them | kernel launches inside them
    pmv::KltGroup* klt_group = nullptr;
    std::atomic<long long> klt_many_stats[4];
    // pmv_debug_klt_stereo_stats: stereo steps | stereo many-calls | host waits inside both | kernel launches inside both (the counters above
    // do not move for stereo calls)
    std::atomic<long long> klt_stereo_stats[4];
    // pmv_debug_klt_observe_stats: step calls (of any form) in which a tracker's observation setting was on | k_klt_observe[_many] launches |
    // k_klt_lift_f[_many] launches | host waits inside those calls
    std::atomic<long long> klt_observe_stats[4];
    // pmv_camera_create (frontend_lift.hip): at most PMV_MAX_CAMERAS cameras, id = index; d_cams is their device table (LiftCam entries),
    // made by the first create and released with the last camera, like h_lift, the mapped pinned block of pmv_undistort_points [points |
    // lifted points | ok bytes], max_tracks of each, made by the first such call, and h_proj, the block of pmv_project_points [camera-frame
    // points (3 doubles) | pixels | ok bytes]. cam_mu guards the table.
    bool cam_used[PMV_MAX_CAMERAS] = {};
    pmv_camera_params cam_params[PMV_MAX_CAMERAS] = {};
    pmv::Buf<pmv::LiftCam> d_cams;
    pmv::Buf<uint8_t> h_lift{pmv::MEM_MAPPED};
    pmv::Buf<uint8_t> h_proj{pmv::MEM_MAPPED};
    std::mutex cam_mu;
    pmv::BackendBuffers* be = nullptr;
    // second back-end lane (own workspace + stream) for work a helper thread runs ahead of the back-end: pmv_triangulate_candidates_ahead
    pmv::BackendBuffers* be_ahead = nullptr;
    hipStream_t s_ahead = nullptr;
    std::mutex ahead_mu;
    // pmv_set_ba_mode: 0 = the multi-kernel LM chain (shortest latency for ONE solve: every phase spread over many CUs),
    // 1 = the whole solve in one workgroup per problem (k_ba_lm / k_ba_lm_batch: ONE launch per solve or per round of B solves).
    // Both are checked against the oracle to the same bars; their floating-point sums are ordered differently, so runs are compared
    // bit for bit only within one mode.
    int ba_mode = 0;
    // pmv_set_frame_format: what the host frames of pmv_frames_stage, pmv_frames_stream_begin and the streamed runs hold (pmv_frame_format)
    int frame_format = PMV_FRAMES_GRAY;
    // pmv_set_frame_preproc: remap and / or CLAHE of every host frame that enters a slot through a feeder (the bracket and the two streamed
    // runs); all zero = off. A feed takes a snapshot (batch_ingest_begin); changed only while no bracket or batched run is open. A map that it
    // names cannot be destroyed.
    pmv_frame_preproc preproc = {};
    // pmv_debug_preproc_launches: feeder rounds that preprocessed | gather launches | CLAHE launch pairs | in-place border launches made for them
    std::atomic<long long> preproc_launches[4];
    // pmv_set_lk_params: the window and level cap shape every layout made from now on (layout_for, cap), the stop criteria go to the LK
    // launches as they are (lk_launch_params). Changed only while no bracket, batched run or session is open, so the launches read them freely.
    pmv_lk_params lk = {pmv::LK_WIN, 4, 30, 0.01, 1e-4f};
    int lk_general = 0;                  // pmv_debug_lk_general
    std::atomic<int> batch_open{0};      // a batched run is inside run_batch (the format must not change under it)
    pmv::BatchEngine* engine = nullptr; // created by the first pmv_pipeline_run_batch or pmv_batch_open
    // The engine and the geometry table have ONE owner at a time: a batched run (batch_open > 0) or a batch session. owner_mu makes the
    // two checks and the claim one step. session_state: 0 none, 1 open, 2 closing; session_calls: session calls in flight (pmv_batch_close).
    std::mutex owner_mu;
    pmv::BatchSession* session = nullptr;
    std::atomic<int> session_state{0}, session_calls{0};
    pmv::BatchIngest* ingest = nullptr;  // feeder of pmv_frames_stream_begin .. _end brackets (created by the first; stream, buffers kept)
    pmv::BatchIngest* bingest = nullptr; // feeder of pmv_pipeline_run_batch[_streamed] (created by the first that needs one)
    double bingest_stats[PMV_BATCH_INGEST_STATS] = {};   // counters of the last pmv_pipeline_run_batch_streamed (pmv_batch_ingest_stats)
    pmv::Profiler prof;
    pmv_call_log log;
    std::mutex err_mu;                  // set_err from several host threads (batch engine)
    char err[512] = "";
};

namespace pmv {
void set_err(pmv_ctx* c, const char* fmt, ...);
const char* thread_error();         // the last message set_err wrote on the calling thread
PyrLayout make_layout(int w, int h, int win, int max_level);   // orc::build_pyramid's level rule for cv::Size(win, win), maxLevel
LKParams lk_launch_params(const pmv_ctx* ctx);                 // the context's LK setting as the launchers take it (stamps = null)
int backend_create(pmv_ctx* c);     // allocates PnP/BA workspaces
void backend_destroy(pmv_ctx* c);
PyrLayout layout_for(pmv_ctx* ctx, int w, int h);
// replaces the context's geometry table by the distinct sizes among (w[b], h[b]), b < B, on the host and on the device (synchronous)
int geom_table_set(pmv_ctx* ctx, const int* w, const int* h, int B);
// The readiness rule of frame slot `slot`: every reader of a pyramid goes through it (the synchronous calls, the batch engine's sequence
// threads and its combiners). When `feed` covers the slot (for sequence `seq` of the feed), waits on the host until the feed round that
// builds the frame is enqueued; then `s`, if given, waits for that round on the GPU, and *round, if given, receives it (-1: none). Then the
// slot must hold a built pyramid (PMV_ERR_INVALID).
int slot_ready(pmv_ctx* ctx, int slot, BatchIngest* feed = nullptr, int seq = 0, hipStream_t s = nullptr, int* round = nullptr);
void batch_ingest_destroy(BatchIngest*& g);
void batch_engine_destroy(pmv_ctx* ctx);
void batch_session_destroy(pmv_ctx* ctx);   // joins the upload thread, frees the session (no session call may be in flight)
// The argument checks of the front-end calls, one copy for every form of a call: the single-sequence entry points (bracket = true: a slot
// of an open pmv_frames_stream_begin bracket first waits for its round on the front-end stream) and the engine's request entries (bracket =
// false; batch_engine.h, "who checks what"). ctx is not null. max_per_cell of detect_check: already >= 1.
int lk_check(pmv_ctx* ctx, bool bracket, int prev_slot, int next_slot, const float* prev_xy, int n, const float* out_xy, const uint8_t* out_status, const float* out_err);
// the extended calls (`who` names the call in the messages): the back outputs of a forward-backward call (fb), lk_check, the flag bits, and
// with PMV_LK_USE_INITIAL_FLOW every initial coordinate (finite, |v| <= 1e6)
int lkx_check(pmv_ctx* ctx, const char* who, bool bracket, int prev_slot, int next_slot, const float* prev_xy, int n, const float* next_xy, int flags,
              const uint8_t* out_status, const float* out_err, bool fb, const float* back_xy, const uint8_t* back_status, const float* back_err);
int knn_check(pmv_ctx* ctx, bool bracket, int src_slot, int cmp_slot, const int* src_xy, int n, const int* cmp_xy, int m, int n_neighbours, int window, const int* out_best,
              const float* out_err);
int detect_check(pmv_ctx* ctx, bool bracket, int slot, const int* cells, int n_cells, int max_per_cell);
// pmv_detect_shitomasi with max_per_cell <= 0 (the reference takes nothing then): the counts are checked and zeroed, nothing is launched
int shitomasi_nothing(pmv_ctx* ctx, const int* cells, int n_cells, int* out_count);
// (x0, y0, w, h) -> device cell records of that frame slot
void pack_cells(int* dst, const int* cells, int n_cells, int slot);
// pmv_detect_gftt_ex / pmv_batch_detect_gftt_ex: the parameter checks (before detect_check), the mask stride against the slot's frame (after
// it), and the packing of the cells' mask sub-views behind byte `pos` of dst (returns the new end; writes each offset into its cell record)
int gftt_ex_check(pmv_ctx* ctx, const char* who, const pmv_gftt_params* p, const int* out_xy, const int* out_count);
int gftt_mask_check(pmv_ctx* ctx, const char* who, int slot, const uint8_t* mask, int mask_stride);
size_t gftt_pack_mask(uint8_t* dst, size_t pos, int* cell_recs, const int* cells, int n_cells, const uint8_t* mask, int mask_stride);
// pmv_detect_gftt_frame / pmv_batch_detect_gftt_frame: every check of the contract, in its order (`who` names the call in the messages). On
// success roi4 holds the region (the whole frame for a null roi4_or_null) and *cap the capacity of the call's corner list.
int gftt_frame_check(pmv_ctx* ctx, const char* who, bool bracket, int slot, const int* roi4_or_null, int max_corners, const pmv_gftt_params* p, const uint8_t* mask,
                     int mask_stride, const int* out_xy, int out_cap, const int* out_count, int* roi4, int* cap);
// a frame request's device record at list entry `list_off`; with a mask its region's bytes go behind byte `pos` of dst (returns the new end)
size_t gftt_frame_record(int* rec, const int* roi4, int slot, size_t list_off, uint8_t* dst, size_t pos, const uint8_t* mask, int mask_stride);
// pmv_detect_gftt_refill / pmv_batch_detect_gftt_refill, after gftt_frame_check (with the base mask as its mask): the checks of the track
// list, the radius and out_keep (`who` names the call in the messages)
int refill_check(pmv_ctx* ctx, const char* who, int slot, const float* track_xy, int n_tracks, int radius, const uint8_t* out_keep);
// pmv_corner_subpix / pmv_batch_corner_subpix: every check of the contract, in its order (`who` names the call in the messages)
int subpix_check(pmv_ctx* ctx, const char* who, bool bracket, int slot, const float* xy, int n, const pmv_subpix_params* p);
int subpix_params_check(pmv_ctx* ctx, const char* who, const pmv_subpix_params* p);   // its window, iteration and eps rules alone (p is not null)
// the context's weight table made ready for p on the front-end stream, and *A the launch arguments for p (frontend_subpix.hip)
hipError_t subpix_table_ready(pmv_ctx* ctx, const pmv_subpix_params* p, SubpixArgs* A);
const LiftCam* camera_entry(pmv_ctx* ctx, int id);   // the device table entry of camera `id`, or null when there is none (frontend_lift.hip)
bool klt_camera_in_use(pmv_ctx* ctx, int cam_id);    // a tracker's observation setting names the camera (frontend_klt.hip)
bool klt_camera_predicted(pmv_ctx* ctx, int cam_id); // a tracker's pending prediction names the camera (frontend_klt.hip)
void klt_destroy_all(pmv_ctx* ctx);   // frees the trackers that are left (pmv_ctx_destroy, after the streams were synchronised)
// the zero zone as cv::cornerSubPix applies it: (-1, -1) unless it lies strictly inside the window
inline void subpix_zero_zone(const pmv_subpix_params* p, int* zw, int* zh) {
    const bool on = p->zero_w >= 0 && p->zero_h >= 0 && 2 * p->zero_w + 1 < 2 * p->win_w + 1 && 2 * p->zero_h + 1 < 2 * p->win_h + 1;
    *zw = on ? p->zero_w : -1; *zh = on ? p->zero_h : -1;
}
// pmv_frames_clahe / pmv_batch_frame_upload_clahe: the parameter checks of the contract (`who` names the call in the messages)
int clahe_check(pmv_ctx* ctx, const char* who, const pmv_clahe_params* p);
// pmv_frames_remap / pmv_batch_frame_upload_remap: the map id and the border value of the contract; on success *map is a copy of the map's entry
int remap_check(pmv_ctx* ctx, const char* who, int map_id, int border_value, pmv_ctx::RemapMap* map);
// pmv_detect_fast: the count / null checks and, for max_per_cell <= 0 (the reference takes nothing then), zero counts - the caller returns
// without a launch; then, for max_per_cell >= 1, the rest of the checks
int fast_counts(pmv_ctx* ctx, const int* cells, int n_cells, int max_per_cell, int* out_count);
int fast_check(pmv_ctx* ctx, bool bracket, int slot, const int* cells, int n_cells, int max_per_cell, const int* out_xy, const float* out_response);
// XCD-aware block order of an LK launch: workgroup b runs on XCD b % 8 and every XCD has its own L2, so the tracks (which arrive in hash
// order, i.e. spatially random) are dealt out by x position: the k-th track of equal-count stripe s goes to block 8k + s. Each L2 then
// fetches one vertical stripe of the two pyramids instead of all of them (measured: 5x less HBM traffic). order: (n + 7) / 8 * 8 entries,
// -1 = padding.
inline void lk_xcd_order(const float* prev_xy, int n, int* order) {
    static thread_local std::vector<std::pair<float, int>> byx;
    const int nb = (n + 7) / 8 * 8;
    byx.resize(n);
    for (int i = 0; i < n; i++) byx[i] = {prev_xy[2 * i], i};
    std::sort(byx.begin(), byx.end());
    for (int b = 0; b < nb; b++) order[b] = -1;
    for (int i = 0; i < n; i++) {
        const int s8 = (int)((long)i * 8 / n), first = (int)(((long)s8 * n + 7) / 8);   // stripe and its first sorted index
        order[(i - first) * 8 + s8] = byx[i].second;
    }
}
// ---- mapped pinned blocks that a launch fills and the host reads after the wait: described once, for the single call and the engine's round.
// Each carves from the caller's cursor: a dry run (Carve()) gives the bytes to ensure(), carve_of(block) the pointers; the kernels get .d, the
// host reads .h.
inline Carve carve_of(const Growable& g) { return Carve(g.p, g.dev, g.cap); }
// corner sub-pixel block of `cap` points: [point records | positions | iterations | flags]
struct SubpixBlock { Carved<SubpixRec> rec; Carved<float> xy; Carved<uint8_t> iters, flags; };
inline SubpixBlock subpix_block(Carve& c, size_t cap) { return {c.take<SubpixRec>(cap), c.take<float>(2 * cap), c.take<uint8_t>(cap), c.take<uint8_t>(cap)}; }
// back results of `cap` forward-backward tracks: [positions | err | status]
struct LkBackBlock { Carved<float> xy, err; Carved<uint8_t> status; };
inline LkBackBlock lk_back_block(Carve& c, size_t cap) { return {c.take<float>(2 * cap), c.take<float>(cap), c.take<uint8_t>(cap)}; }
// block of a launch of n_req frame requests of `cap` corners each: [request records | counts | (records, off-chip) pairs | corner lists]
struct GfttFrameBlock { Carved<int> rec, count, stats, xy; };
inline GfttFrameBlock gftt_frame_block(Carve& c, size_t n_req, size_t cap) {
    return {c.take<int>(n_req * CELL_STRIDE), c.take<int>(n_req), c.take<int>(2 * n_req), c.take<int>(2 * n_req * cap, 16)};
}
// tables of a launch of n_req refill requests with n_trk track entries in all (the sum of the requests' refill_pad(n)):
// [request records | positions | priorities | base flags | half-width tables | keep bytes]
struct RefillBlock { Carved<RefillRec> rec; Carved<unsigned> pos; Carved<int> prio; Carved<uint8_t> flag, hw, keep; };
inline RefillBlock refill_block(Carve& c, size_t n_req, size_t n_trk) {
    return {c.take<RefillRec>(n_req, 16), c.take<unsigned>(n_trk), c.take<int>(n_trk), c.take<uint8_t>(n_trk), c.take<uint8_t>(n_req * REFILL_HW), c.take<uint8_t>(n_trk, 4)};
}
// request i of a refill block: its record (tracks at entry trk_off, region roi4, packed mask at byte mask_off), the rounded positions, the
// priorities (null: all equal), the flag of every track (the base byte under it is 255; no base mask: all set) and the half-width table
void refill_fill(const RefillBlock& B, size_t i, size_t trk_off, const int* roi4, size_t mask_off, const float* track_xy, const int* track_prio_or_null, int n_tracks,
                 int radius, const uint8_t* base_mask_or_null, int base_stride);
hipError_t frontend_prepare_device();   // per-device kernel attributes (LDS opt-in), called with the context's device current
hipError_t backend_prepare_device();
}
