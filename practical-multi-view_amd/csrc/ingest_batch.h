// The feeder (ingest_batch.hip): builds the pyramids of B sequences' frame slots on its own stream while the sequences already read them.
// Users: pmv_pipeline_run_batch_streamed (host frames through recycled rings), pmv_pipeline_run_batch (frames staged in place) and the
// pmv_frames_stream_begin .. _end bracket (one sequence of host frames). Readers wait for a slot through pmv::slot_ready (pmv_ctx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/pmv_hip.h"
struct pmv_ctx;
namespace pmv {
struct BatchIngest;
// What a feed serves: it sets a sequence's frames per round (as each route had them before the feeder) and the default form.
enum FeedKind { FEED_STREAMED, FEED_STAGED, FEED_BRACKET };
// One sequence of a feed: frame f goes to slot first + f % ring. src: tight w x h host frames (pageable or pinned) in the feed's format, or null: the frames are
// already staged in their slots (ring = n), only the pad and the pyramid levels are left to do. w, h: the sequence's own frame size (the
// sequences of a feed may differ: the reference takes whatever cv::imread returns, Frame.cpp:31-42).
struct FeedSeq { int first, n, ring; const uint8_t* src; int w, h; };
// Validates nothing the caller has not (slot ranges, sizes; the rings of a feed that recycles slots are disjoint); creates *g on first use,
// marks every slot of the feed built with its sequence's geometry (its readers wait in slot_ready for the round that builds it) and starts the
// feeder thread. Staged ranges may overlap: a slot that several sequences cover is built once (the caller has checked that they agree on its
// size). A feed of several sequences (FEED_STREAMED, FEED_STAGED) finds every sequence's size in the context's geometry table (geom_table_set).
// `format` (pmv_frame_format) is what the host frames hold: gray, or tight BGR (3 w h bytes a frame) that level 0 converts on the way in.
// `pre` (pmv_set_frame_preproc; null or all zero: off) is copied: it governs the sequences with a host source. Each of them finds the map of
// its own size once, here; one without a map is PMV_ERR_INVALID before a slot changes or the thread starts. With a remap the feed takes the
// copy form whatever PMV_BATCH_INGEST says: the gather reads HBM only.
int batch_ingest_begin(pmv_ctx* ctx, BatchIngest*& g, FeedKind kind, const std::vector<FeedSeq>& seqs, int format = PMV_FRAMES_GRAY,
                       const pmv_frame_preproc* pre = nullptr);
bool batch_ingest_active(const BatchIngest* g);
// Combiner thread: make `s` wait on the GPU for feed round `round` (the feeder's stream is in order: every earlier round as well).
hipError_t batch_ingest_wait_gpu(BatchIngest* g, hipStream_t s, int round);
// Sequence `seq` no longer reads frames below `frame` (its front-end thread, after addFrame returned).
void batch_ingest_release(BatchIngest* g, int seq, int frame);
// Sequence `seq` has ended (finished or failed): its ring is free; a ring that recycles slots receives nothing more.
void batch_ingest_finish(BatchIngest* g, int seq);
// Joins the feeder thread (it ends once every frame that will be fed is enqueued) and waits for its stream. A slot that never received its
// frame goes back to empty (host source) or staged (staged source).
int batch_ingest_end(pmv_ctx* ctx, BatchIngest* g);
constexpr int BATCH_INGEST_STATS = PMV_BATCH_INGEST_STATS;
void batch_ingest_stats(const BatchIngest* g, double* out6);
}  // namespace pmv
