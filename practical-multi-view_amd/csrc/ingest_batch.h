// Streamed ingest of a batched run (ingest_batch.hip): B sequences' gray frames move from host memory into per-sequence rings of
// frame slots while the sequences track; pmv_pipeline_run_batch_streamed is its only user.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pmv_hip.h"
struct pmv_ctx;
namespace pmv {
struct BatchIngest;
// Validates nothing the caller has not (slot ranges, sizes); starts the ingest thread. `host_frames[b]`: n_frames[b] tight w x h frames.
int batch_ingest_begin(pmv_ctx* ctx, int B, const int* first_slot, const int* n_frames, const uint8_t* const* host_frames, int ring, int w, int h,
                       BatchIngest** out);
// Sequence `seq`'s own front-end thread, before an LK / detect request on `slot`: waits on the host until the frame the sequence needs in
// that slot has been enqueued, and returns the ingest round that builds it (for batch_ingest_wait_gpu).
int batch_ingest_acquire(BatchIngest* g, int seq, int slot, int* round);
// Combiner thread: make `s` wait on the GPU for ingest round `round` (the ingest stream is in order: every earlier round as well).
hipError_t batch_ingest_wait_gpu(void* g, hipStream_t s, int round);
// Sequence `seq` no longer reads frames below `frame` (its front-end thread, after addFrame returned).
void batch_ingest_release(BatchIngest* g, int seq, int frame);
// Sequence `seq` has ended (finished or failed): its whole ring is free, nothing more is ingested for it.
void batch_ingest_finish(BatchIngest* g, int seq);
// Joins the ingest thread and waits for its stream; sets ctx->slot_layout of every ring slot (built, or empty if it never received a frame).
int batch_ingest_end(pmv_ctx* ctx, BatchIngest* g);
constexpr int BATCH_INGEST_STATS = PMV_BATCH_INGEST_STATS;
void batch_ingest_stats(const BatchIngest* g, double* out6);
void batch_ingest_destroy(pmv_ctx* ctx);
}  // namespace pmv
