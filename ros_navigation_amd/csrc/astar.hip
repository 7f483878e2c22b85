// astar.hip -- host side of the batched grid A*: configuration (pipeline stages, pages per query, what fits HBM), the
// choice of a stage for each batch, chunking, the C ABI.  The search itself is astar_tile.hip (one workgroup per query,
// register-resident 64 x 16 tiles, an open list of tiles in LDS).
//
// Grid A* (DESIGN.md "Grid A* contract", restated by oracle/astar.c).  The reference has no grid
// search (AStarPlanner::makePlan walks a 9-vertex graph, mc/src/astar_planner.cpp:63-127); the
// contract is: 8-connected, integer costs 1000/1414, octile heuristic, no corner cutting, every cell
// with f <= f* settled, canonical predecessor = optimal neighbour with the lowest linear index.
// Because the path is a function of the exact distance field only, any label-correcting schedule
// that converges gives the CPU oracle's path bit for bit.
// Maps of more than 65 536 tiles (8192 x 8192 cells) are refused with RNA_EINVAL: tile numbers are 16 bits in the
// search's queue entries.  (Rounds 1-2 kept a cell-granular frontier kernel as a fallback for such maps; it did not
// handle moved maps, no configuration reached it, and it was removed in round 3.)
#include "engine.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <thread>
#include <vector>

using namespace rna;

namespace {

constexpr int COST_D = 1414;

// developer switch RNA_HOST_TRACE=1: host microseconds inside the segments of a pipelined batch launch, printed when the search
// state is released (where the host's share of a pass goes)
struct HostTrace {
  bool on = getenv("RNA_HOST_TRACE") != nullptr;
  double us[8] = {};
  long n = 0, queries = 0;
  std::chrono::steady_clock::time_point t;
  void start() { if (on) t = std::chrono::steady_clock::now(); }
  void lap(int k) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    us[k] += std::chrono::duration<double, std::micro>(now - t).count();
    t = now;
  }
  void dump() {
    if (!on || n == 0) return;
    fprintf(stderr, "[host trace] %ld pipelined launches, us each: wait for a free stage %.1f (%.2f hipEventQuery calls) | ring entry's old batch %.1f | "
            "enqueue (events, snapshot, launch order, search, flag copy) %.1f | done event + bookkeeping %.1f\n", n, us[0] / n, (double)queries / n,
            us[1] / n, us[2] / n, us[3] / n);
    for (double& v : us) v = 0;
    n = 0; queries = 0;
  }
};
HostTrace g_trace;
// (RNA_HOST_TRACE) a stage's cycle in GPU time: event A when the stage's stream reaches the new batch (it is idle: at enqueue),
// C when the search and what follows it on the stream have ended; host clock: enqueue and "noticed free".  (With a third event
// where the search's last wait ends -- in front of the search launch, a temporary hook -- round 6 measured 4.46 ms from enqueue
// until the search may start, 22.40 ms of search, 27.89 ms until the host has noticed: profiles/r06_host_trace.txt.)
struct StageTrace {
  hipEvent_t a[AstarDevice::MAX_DEPTH] = {}, c[AstarDevice::MAX_DEPTH] = {};
  std::chrono::steady_clock::time_point t_enq[AstarDevice::MAX_DEPTH];
  bool armed[AstarDevice::MAX_DEPTH] = {};
  double gpu_ms = 0, host_busy_ms = 0;
  long n = 0;
};
StageTrace g_stage;
void stage_trace_dump() {
  if (g_stage.n) fprintf(stderr, "[host trace] a stage's cycle, ms: from enqueue to the end of the search and what follows it on the stream %.2f (the search itself: roofline.avg_launch_ms) | "
                         "host: enqueue -> noticed free %.2f (%ld cycles)\n", g_stage.gpu_ms / g_stage.n, g_stage.host_busy_ms / g_stage.n, g_stage.n);
  g_stage.gpu_ms = g_stage.host_busy_ms = 0; g_stage.n = 0;
}

#define RNA_TRY(call) do { const int rc_try_ = (call); if (rc_try_ != RNA_OK) return rc_try_; } while (0)

// one stage of the configuration ensure_config settled on (a released stage: every member is at its default)
int alloc_stage(rna_engine* e, int d) {
  AstarDevice& a = e->astar;
  AstarStage& s = a.stage[d];
  RNA_TRY(dev_alloc(e, &s.pool, tsa_pool_bytes(a.max_queries, a.page_cap) / sizeof(unsigned)));
  RNA_TRY(dev_alloc(e, &s.rev, (size_t)a.rev_cap * a.max_queries));
  RNA_TRY(dev_alloc(e, &s.block, tsa_stage_bytes(e)));
  RNA_HIP(e, hipMemsetAsync(s.block, 0, tsa_stage_bytes(e), e->stream));
  RNA_TRY(tsa_stage_prepare(e, d));
  if (a.page_cap < tsa_tiles(e)) {   // a search may outgrow its share of pages: retry slots with a page per tile
    RNA_TRY(dev_alloc(e, &s.retry_pool, tsa_retry_pool_bytes(e) / sizeof(unsigned)));
    RNA_TRY(dev_alloc(e, &s.retry_block, tsa_retry_bytes(e)));
    RNA_HIP(e, hipMemsetAsync(s.retry_block, 0, tsa_retry_bytes(e), e->stream));
    RNA_TRY(tsa_retry_prepare(e, d));
  }
  if (a.depth == 1) return RNA_OK;
  // searches run at the lowest queue priority, the engine stream (map update, VFH+, field reset) at the highest:
  // its short kernels gate the next search launch and must not queue behind 1000 waiting search workgroups
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (getenv("RNA_NO_STREAM_PRIORITY")) prio_lo = prio_hi = 0;
  // The search streams may not use one CU in eight (ROCr deals the bits of a queue's CU mask round-robin to the
  // XCDs, so the first n bits are n / 8 CUs of every XCD).  A search workgroup holds its CU slot for a whole query
  // (milliseconds) and four of them fill a CU's registers, so a stream priority cannot make room for the engine
  // stream's short kernels (map update, VFH+, field reset) that gate the next search launch: without the reserve
  // they take 3 ms instead of 0.3 ms each and the step rate hangs on them (22 k instead of 33 k cycles/s when this
  // was introduced; with the final kernel 16 / 24 / 32 / 40 / 48 reserved CUs: 74.6 / 78.8 / 80.5 / 78.8 / 76.7 k).
  // RNA_SEARCH_CU_SKIP=n overrides the number of reserved CUs, 0 = no mask (stream priority only).
  int skip = e->cu_count / 8;
  if (const char* m = getenv("RNA_SEARCH_CU_SKIP")) skip = atoi(m);
  if (skip > 0 && skip < e->cu_count) {
    uint32_t mask[16] = {};
    const int words = (e->cu_count + 31) / 32 < 16 ? (e->cu_count + 31) / 32 : 16;
    for (int c = skip; c < e->cu_count && c < 512; ++c) mask[c >> 5] |= 1u << (c & 31);
    RNA_HIP(e, hipExtStreamCreateWithCUMask(&s.stream, (uint32_t)words, mask));
  } else {
    RNA_HIP(e, hipStreamCreateWithPriority(&s.stream, hipStreamNonBlocking, prio_lo));
  }
  RNA_HIP(e, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  RNA_HIP(e, hipEventCreateWithFlags(&s.snap_done, hipEventDisableTiming));
  return RNA_OK;
}

void free_stage(AstarStage& s) {
  dev_free(&s.pool); dev_free(&s.rev); dev_free(&s.block); dev_free(&s.retry_pool); dev_free(&s.retry_block);
  if (s.stream) (void)hipStreamDestroy(s.stream);
  if (s.done) (void)hipEventDestroy(s.done);
  if (s.snap_done) (void)hipEventDestroy(s.snap_done);
  s = AstarStage{};
}

// allocation of the whole configuration; errors are returned as they come, alloc_stages cleans up
int alloc_stages_impl(rna_engine* e) {
  AstarDevice& a = e->astar;
  for (int d = 0; d < a.depth; ++d) RNA_TRY(alloc_stage(e, d));
  if (a.depth > 1) {
    RNA_HIP(e, hipEventCreateWithFlags(&a.ev_init, hipEventDisableTiming));
    RNA_HIP(e, hipEventCreateWithFlags(&a.ev_prep, hipEventDisableTiming));
    a.ring_n = 2 * a.depth;
    a.ring_stride = tsa_ring_bytes(e);
    RNA_TRY(dev_alloc(e, &a.ring_mem, a.ring_stride * (size_t)a.ring_n));
    RNA_HIP(e, hipMemsetAsync(a.ring_mem, 0, a.ring_stride * (size_t)a.ring_n, e->stream));
    for (int r = 0; r < a.ring_n; ++r) RNA_HIP(e, hipEventCreateWithFlags(&a.ring[r].free, hipEventDisableTiming));
  }
  if (a.stage[0].retry_pool) {
    RNA_HIP(e, hipHostMalloc(reinterpret_cast<void**>(&a.retry_flag), AstarDevice::MAX_DEPTH * sizeof(int), hipHostMallocCoherent));
    for (int d = 0; d < AstarDevice::MAX_DEPTH; ++d) a.retry_flag[d] = 0;
    for (int d = 0; d < a.depth; ++d) a.stage[d].retry_flag = a.retry_flag + d;
  }
  a.launches = 0;
  RNA_TRY(dev_alloc(e, &a.queries_dev, (size_t)a.max_queries));
  RNA_TRY(dev_alloc(e, &a.results_dev, (size_t)a.max_queries));
  return RNA_OK;
}

// (whatever fails inside -- an allocation, a memset, a stream or an event -- nothing half-built is left behind: the next call starts
// from nothing again instead of finding stage 0 allocated and taking the configuration for complete; the first error's text is kept)
int alloc_stages(rna_engine* e) {
  const int rc = alloc_stages_impl(e);
  if (rc != RNA_OK) {
    const std::string why = e->err;
    (void)astar_release(e);
    e->err = why;
  }
  return rc;
}

int ensure_config(rna_engine* e) {
  AstarDevice& a = e->astar;
  if (a.live()) return RNA_OK;
  if (a.max_queries <= 0) a.max_queries = 256;
  if (!tsa_supported(e)) return fail(e, RNA_EINVAL, "grid A*: more than 65 536 tiles of 64 x 16 cells (8192 x 8192 cells): tile numbers are 16 bits");
  a.depth = std::clamp(a.depth, 1, (int)AstarDevice::MAX_DEPTH);
  // fit into free HBM (25 % headroom): fewer pages per query (half a map's worth), fewer pipeline stages, fewer pages
  // still -- a search that needs more than its share is searched again on a full-size retry slot (astar_tile.hip: eight
  // at a time, as many passes as it takes; status 5 is transient and never final) --, then fewer concurrent queries
  size_t free_b = 0, total_b = 0;
  RNA_HIP(e, hipMemGetInfo(&free_b, &total_b));
  const int ntile = tsa_tiles(e);
  a.page_cap = ntile;
  if (a.page_cap_request > 0 && a.page_cap_request < ntile) a.page_cap = a.page_cap_request;
  if (const char* c = getenv("RNA_ASTAR_PAGE_CAP")) { const int v = atoi(c); if (v > 0 && v < ntile) a.page_cap = v; }
  auto stage_bytes = [&]() -> double {
    return (double)tsa_pool_bytes(a.max_queries, a.page_cap) + (double)tsa_stage_bytes(e) + (double)a.rev_cap * 4.0 * a.max_queries +
           (a.page_cap < ntile ? (double)tsa_retry_pool_bytes(e) + (double)tsa_retry_bytes(e) : 0.0);
  };
  // (tile kernel) half a map's worth of pages per query first -- searches touch a few per cent of the map, and twelve
  // stages of 17.8 GB each at 4096^2 x 256 queries sit right at the budget --, then fewer stages, then fewer pages
  if (a.page_cap > 64 && a.page_cap > ntile / 2 && stage_bytes() * a.depth > 0.75 * (double)free_b) a.page_cap = (ntile + 1) / 2;
  while (a.depth > 1 && stage_bytes() * a.depth > 0.75 * (double)free_b) a.depth -= 1;
  while (a.page_cap > 64 && a.page_cap > ntile / 8 && stage_bytes() * a.depth > 0.75 * (double)free_b) a.page_cap /= 2;
  while (a.max_queries > 1 && stage_bytes() * a.depth > 0.75 * (double)free_b) a.max_queries /= 2;
  // HBM may have gone to another process between hipMemGetInfo and here: step down and try again
  for (;;) {
    const int rc = alloc_stages(e);
    if (rc != RNA_ENOMEM) return rc;
    if (a.page_cap > 64 && a.page_cap > ntile / 2) a.page_cap = (ntile + 1) / 2;
    else if (a.depth > 1) a.depth = a.depth > 2 ? a.depth * 3 / 4 : 1;
    else if (a.page_cap > 64 && a.page_cap > ntile / 8) a.page_cap /= 2;
    else if (a.max_queries > 1) a.max_queries /= 2;
    else return rc;
  }
}

hipStream_t stage_stream(rna_engine* e, int d) { return e->astar.depth > 1 ? e->astar.stage[d].stream : e->stream; }
// the stage's last batch may have something left to do: the host has not seen `done` complete; one stream: a second pass may be due
bool stage_pending(const AstarDevice& a, int d) { return a.depth > 1 ? a.stage[d].busy : a.stage[d].retry_armed; }

// The stage's search has finished (the host has seen its `done` event, or the engine stream, complete): if searches of that
// batch ran out of pages, their second pass goes out now (*sent) and `done` is recorded behind it again.
int stage_settled(rna_engine* e, int d, bool* sent) {
  AstarStage& s = e->astar.stage[d];
  *sent = false;
  if (!s.retry_armed) return RNA_OK;
  s.retry_armed = false;
  if (!s.retry_flag || *s.retry_flag == 0) return RNA_OK;
  const int count = *s.retry_flag;
  *s.retry_flag = 0;
  s.last_retried = count;
  RNA_TRY(tsa_retry_launch(e, d, stage_stream(e, d), count));
  if (e->astar.depth > 1) RNA_HIP(e, hipEventRecord(s.done, s.stream));
  *sent = true;
  return RNA_OK;
}

// The host waits for the stage's last batch, second passes included (as many as it takes; status 5 is never final).
int stage_wait(rna_engine* e, int d) {
  AstarStage& s = e->astar.stage[d];
  for (bool sent = true; sent;) {
    if (e->astar.depth > 1) RNA_HIP(e, hipEventSynchronize(s.done));
    else RNA_HIP(e, hipStreamSynchronize(e->stream));
    RNA_TRY(stage_settled(e, d, &sent));
  }
  s.busy = false;
  return RNA_OK;
}

// Which stage the next batch goes to (pipelined).  On return the host has seen the stage free (except under RNA_ASTAR_NOWAIT),
// and the batch that last read the ring entry this launch will write is over and settled.
int pick_stage(rna_engine* e, int* slot_out) {
  AstarDevice& a = e->astar;
  // Which stage: one that IS free, the one that has been free the longest -- not simply the next in turn.  A batch lasts
  // as long as its longest search; taking the stages strictly in turn, a new batch waits for the one slow batch while
  // the stages behind it have long finished (they sat idle 40 % of the time at thirteen stages).  If none is free the
  // HOST waits for one (a few hundred microseconds at the bench's load) -- enqueued blindly behind "the oldest", as in
  // round 2, a stage's stream sat idle 7 ms between two searches of 23 ms.
  static const bool nowait = getenv("RNA_ASTAR_NOWAIT") != nullptr;   // developer knob: the round-2 behaviour
  // A stage known to be free is taken without asking anybody; otherwise the stages are asked in the order of their launches
  // (they end roughly in that order), at most RNA_ASTAR_QUERIES_PER_LOOK (3) per look, and the first one found complete is
  // taken.  (Round 6 measured this loop, RNA_HOST_TRACE=1: the host spends 1.38 ms of a 1.57 ms pass here -- not in the
  // queries, which cost 5 us each, but because every stage IS taken: a stage's cycle is 4.5 ms from enqueue until its search
  // may start (the pass's map-update chain, snapshot and launch order), 22.4 ms of search and 1 ms until the host has
  // noticed; a completion flag written by the stream instead of the event changes nothing.)
  static const int per_look = getenv("RNA_ASTAR_QUERIES_PER_LOOK") ? std::max(1, atoi(getenv("RNA_ASTAR_QUERIES_PER_LOOK"))) : 3;   // developer knob
  int slot = -1;
  for (int spin = 0; slot < 0; ++spin) {
    int oldest = 0;
    for (int d = 0; d < a.depth; ++d) {
      if (a.stage[d].seq < a.stage[oldest].seq) oldest = d;
      if (!a.stage[d].busy && (slot < 0 || a.stage[d].seq < a.stage[slot].seq)) slot = d;
    }
    if (slot < 0) {
      // the busy stages by age; every eighth look asks all of them (a batch with one very long search must not hide the others)
      int order[AstarDevice::MAX_DEPTH], nb = 0;
      for (int d = 0; d < a.depth; ++d) if (a.stage[d].busy) order[nb++] = d;
      std::sort(order, order + nb, [&](int x, int y) { return a.stage[x].seq < a.stage[y].seq; });
      const int ask = (spin & 7) == 7 ? nb : std::min(nb, per_look);
      for (int k = 0; k < ask && slot < 0; ++k) {
        const int d = order[k];
        g_trace.queries += 1;
        if (hipEventQuery(a.stage[d].done) != hipSuccess) { (void)hipGetLastError(); continue; }   // hipErrorNotReady is not an error
        bool sent = false;
        RNA_TRY(stage_settled(e, d, &sent));
        if (sent) continue;   // a second pass went out: the stage stays busy
        a.stage[d].busy = false;
        slot = d;
        if (g_trace.on && g_stage.armed[d]) {
          float f = 0;
          if (hipEventElapsedTime(&f, g_stage.a[d], g_stage.c[d]) == hipSuccess) {
            g_stage.gpu_ms += f; g_stage.n += 1;
            g_stage.host_busy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_stage.t_enq[d]).count();
          }
          g_stage.armed[d] = false;
        }
      }
    }
    if (slot >= 0) break;
    if (nowait) { slot = oldest; break; }
    // (no stage free: the host SLEEPS between looks -- with thirteen launches in flight a stage that frees up 50 us before
    // the host notices costs nothing, and eight ranks of one node share the host's cores; round 5 yielded 64 times and then
    // slept 20 us, which kept a core busy: config.host_cores_used 0.98)
    static const int wait_us = getenv("RNA_ASTAR_WAIT_US") ? atoi(getenv("RNA_ASTAR_WAIT_US")) : 50;   // developer knob
    if (spin >= 2 && wait_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(wait_us));
    else std::this_thread::yield();
  }
  g_trace.lap(0);
  // the ring entry this launch writes: the batch that read it 2 x depth launches ago is over and settled
  const unsigned long long prev = a.launches + 1 >= (unsigned long long)a.ring_n ? a.launches + 1 - (unsigned long long)a.ring_n : 0;
  for (int d = 0; prev > 0 && d < a.depth; ++d)
    if (a.stage[d].busy && a.stage[d].seq == prev) RNA_TRY(stage_wait(e, d));
  *slot_out = slot;
  return RNA_OK;
}

// One batch (<= max_queries) on the stage pick_stage chose, or on the engine stream.  Pipelined, the mask snapshot and the launch
// order go to the side stream, behind an event of the engine stream and into an entry of the launch ring (whatever changes the
// masks next waits for the snapshot: side_join) -- on the stage's own stream these two short kernels waited up to a millisecond
// for CU slots among the searches' workgroups, and the engine stream's next map update with them --, then the search to the
// stage's stream.  The order of the calls below is the contract of a pipelined launch.
int launch_chunk(rna_engine* e, const rna_astar_query* q_dev, int n, int32_t* paths_dev, int max_len,
                 rna_astar_result* res_dev, int* slot_out) {
  AstarDevice& a = e->astar;
  const bool pipelined = a.depth > 1;
  int slot = 0, r = -1;
  g_trace.start();
  if (pipelined) RNA_TRY(pick_stage(e, &slot));
  g_trace.lap(1);
  if (!pipelined && stage_pending(a, 0)) RNA_TRY(stage_wait(e, 0));   // one stream: the batch before this one has to be complete before its slots are reused
  AstarStage& s = a.stage[slot];
  hipStream_t search = stage_stream(e, slot), prep = search;
  if (pipelined) {
    if (s.busy) RNA_HIP(e, hipStreamWaitEvent(search, s.done, 0));   // (RNA_ASTAR_NOWAIT only; the same stream anyway)
    if (g_trace.on) {
      if (!g_stage.a[slot]) { (void)hipEventCreate(&g_stage.a[slot]); (void)hipEventCreate(&g_stage.c[slot]); }
      (void)hipEventRecord(g_stage.a[slot], search);
      g_stage.t_enq[slot] = std::chrono::steady_clock::now();
    }
    r = (int)(a.launches % (unsigned long long)a.ring_n);
    RNA_TRY(side_stream(e, &prep));
    RNA_HIP(e, hipEventRecord(a.ev_init, e->stream));
    RNA_HIP(e, hipStreamWaitEvent(prep, a.ev_init, 0));
    if (a.ring[r].used) RNA_HIP(e, hipStreamWaitEvent(prep, a.ring[r].free, 0));   // (thirteen launches ago at least: long over)
  }
  RNA_TRY(tsa_snapshot(e, slot, r, prep));
  if (pipelined) {
    RNA_HIP(e, hipEventRecord(s.snap_done, prep));
    s.snap_pending = true;
  }
  RNA_TRY(tsa_order(e, slot, r, prep, q_dev, n));
  if (pipelined) {
    RNA_HIP(e, hipEventRecord(a.ev_prep, prep));
    RNA_HIP(e, hipStreamWaitEvent(search, a.ev_prep, 0));
  }
  if (s.retry_flag) *s.retry_flag = 0;
  // search kernel, the count of searches to repeat to pinned host memory, trace kernel: the trace kernel reads the ring entry's
  // launch order and masks, so the entry is free -- and the stage done -- only behind it
  RNA_TRY(tsa_search(e, slot, r, search, q_dev, n, paths_dev, max_len, res_dev));
  if (pipelined) {
    RNA_HIP(e, hipEventRecord(a.ring[r].free, search));
    a.ring[r].used = true;
    if (g_trace.on) { (void)hipEventRecord(g_stage.c[slot], search); g_stage.armed[slot] = true; }
  }
  g_trace.lap(2);
  if (pipelined) {
    RNA_HIP(e, hipEventRecord(s.done, search));
    s.busy = true;
  }
  a.launches += 1;
  s.seq = a.launches;
  a.last_queries = q_dev; a.last_results = res_dev; a.last_n = n; a.last_slot = slot;
  if (slot_out) *slot_out = slot;
  g_trace.lap(3);
  if (pipelined) g_trace.n += 1;
  return RNA_OK;
}

}  // namespace

namespace rna {
// every stream is idle (sync_all): second passes that are due go out and are waited for
int astar_settle(rna_engine* e) {
  AstarDevice& a = e->astar;
  for (int d = 0; d < a.depth && d < AstarDevice::MAX_DEPTH; ++d)
    if (stage_pending(a, d)) RNA_TRY(stage_wait(e, d));
  return RNA_OK;
}
int astar_release(rna_engine* e) {
  AstarDevice& a = e->astar;
  (void)sync_all(e);
  stage_trace_dump();
  g_trace.dump();
  for (AstarStage& s : a.stage) free_stage(s);
  if (a.ev_init) { (void)hipEventDestroy(a.ev_init); a.ev_init = nullptr; }
  if (a.ev_prep) { (void)hipEventDestroy(a.ev_prep); a.ev_prep = nullptr; }
  for (AstarRingEntry& r : a.ring) {
    if (r.free) (void)hipEventDestroy(r.free);
    r = AstarRingEntry{};
  }
  dev_free(&a.ring_mem);
  a.ring_n = 0;
  if (a.retry_flag) { (void)hipHostFree(a.retry_flag); a.retry_flag = nullptr; }
  dev_free(&a.queries_dev); dev_free(&a.results_dev); dev_free(&a.paths_dev);
  a.paths_cap = 0;
  a.last_queries = nullptr; a.last_results = nullptr; a.last_n = 0;
  return RNA_OK;
}
}  // namespace rna

extern "C" int rna_astar_configure(rna_engine* e, int max_queries, int queue_capacity, int bucket_width) {
  if (!e || max_queries < 0 || queue_capacity < 0 || bucket_width < 0) return RNA_EINVAL;
  if (bucket_width != 0 && bucket_width < 2 * COST_D) return fail(e, RNA_EINVAL, "bucket_width must be >= 2828");
  RNA_ENTER(e);
  RNA_HIP(e, hipStreamSynchronize(e->stream));
  AstarDevice& a = e->astar;
  if (max_queries || queue_capacity) astar_release(e);
  if (const char* d = getenv("RNA_ASTAR_PIPELINE")) {  // pipeline stages (1 = searches run on the engine stream)
    const int dd = atoi(d);
    if (dd >= 1 && dd != a.depth) { astar_release(e); a.depth = dd; }
  }
  if (max_queries) a.max_queries = max_queries;   // (queue_capacity: of the ABI, no longer used)
  if (bucket_width) a.bucket_width = bucket_width;
  return RNA_OK;
}

extern "C" int rna_astar_set_pipeline_depth(rna_engine* e, int depth) {
  if (!e || depth < 1 || depth > AstarDevice::MAX_DEPTH) return RNA_EINVAL;
  RNA_ENTER(e);
  if (depth != e->astar.depth) {
    astar_release(e);
    e->astar.depth = depth;
  }
  char advice[448];   // (the longest advice line is about 330 characters)
  if (rna_hw_queue_advice(depth, advice, sizeof(advice))) e->err = advice;   // (still RNA_OK: correct, only slower)
  return RNA_OK;
}

extern "C" int rna_astar_effective_config(const rna_engine* e, int* pipeline_depth, int* pages_per_query, int* max_queries) {
  if (!e) return RNA_EINVAL;
  const AstarDevice& a = e->astar;
  const bool live = a.live();
  if (pipeline_depth) *pipeline_depth = live ? a.depth : 0;
  if (pages_per_query) *pages_per_query = live ? a.page_cap : 0;
  if (max_queries) *max_queries = live ? a.max_queries : 0;
  return RNA_OK;
}

extern "C" int rna_astar_set_page_cap(rna_engine* e, int pages_per_query) {
  if (!e || pages_per_query < 0) return RNA_EINVAL;
  RNA_ENTER(e);
  if (pages_per_query != e->astar.page_cap_request) {
    astar_release(e);
    e->astar.page_cap_request = pages_per_query;
  }
  return RNA_OK;
}

extern "C" int rna_astar_batch_device(rna_engine* e, const rna_astar_query* queries, int n, int32_t* paths,
                                      int max_path_len, rna_astar_result* results) {
  if (!e || n < 0 || max_path_len <= 0 || (n > 0 && (!queries || !paths || !results))) return RNA_EINVAL;
  if (n == 0) return RNA_OK;
  RNA_ENTER_NOJOIN(e);   // (reads the neighbour masks only; map_prepare_nbr joins if it has to rebuild them)
  int rc = ensure_config(e);
  if (rc != RNA_OK) return rc;
  if ((rc = map_prepare_nbr(e)) != RNA_OK) return rc;
  const int chunk = e->astar.max_queries;
  for (int o = 0; o < n; o += chunk) {
    const int m = std::min(chunk, n - o);
    rc = launch_chunk(e, queries + o, m, paths + (size_t)o * max_path_len, max_path_len, results + o, nullptr);
    if (rc != RNA_OK) return rc;
  }
  return RNA_OK;
}

extern "C" int rna_astar_batch(rna_engine* e, const rna_astar_query* queries_host, int n, int32_t* paths_host,
                               int max_path_len, rna_astar_result* results_host) {
  if (!e || n < 0 || max_path_len <= 0 || (n > 0 && (!queries_host || !paths_host || !results_host))) return RNA_EINVAL;
  if (n == 0) return RNA_OK;
  RNA_ENTER(e);
  int rc = ensure_config(e);
  if (rc != RNA_OK) return rc;
  if ((rc = map_prepare_nbr(e)) != RNA_OK) return rc;
  AstarDevice& a = e->astar;
  const int chunk = a.max_queries;
  const size_t need = (size_t)chunk * max_path_len;
  if ((size_t)a.paths_cap < need) {
    if (need > 0x7fffffffULL) return fail(e, RNA_EINVAL, "max_path_len too large");
    if ((rc = dev_alloc(e, &a.paths_dev, need)) != RNA_OK) return rc;
    a.paths_cap = (int)need;
  }
  for (int o = 0; o < n; o += chunk) {
    const int m = std::min(chunk, n - o);
    RNA_HIP(e, hipMemcpyAsync(a.queries_dev, queries_host + o, (size_t)m * sizeof(rna_astar_query),
                              hipMemcpyHostToDevice, e->stream));
    int slot = 0;
    rc = launch_chunk(e, a.queries_dev, m, a.paths_dev, max_path_len, a.results_dev, &slot);
    if (rc != RNA_OK) return rc;
    if (stage_pending(a, slot) && (rc = stage_wait(e, slot)) != RNA_OK) return rc;
    RNA_HIP(e, hipMemcpyAsync(results_host + o, a.results_dev, (size_t)m * sizeof(rna_astar_result),
                              hipMemcpyDeviceToHost, e->stream));
    RNA_HIP(e, hipMemcpyAsync(paths_host + (size_t)o * max_path_len, a.paths_dev,
                              (size_t)m * max_path_len * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    RNA_HIP(e, hipStreamSynchronize(e->stream));
  }
  return RNA_OK;
}

extern "C" int rna_astar_download_nbr_mask(rna_engine* e, uint8_t* host, size_t n) {
  if (!e || !host || n != e->ncell) return RNA_EINVAL;
  RNA_ENTER(e);
  int rc = map_prepare_nbr(e);
  if (rc != RNA_OK) return rc;
  RNA_HIP(e, hipMemcpyAsync(host, e->nbr, n, hipMemcpyDeviceToHost, e->stream));
  RNA_HIP(e, hipStreamSynchronize(e->stream));
  return RNA_OK;
}

extern "C" int rna_astar_job_counters(rna_engine* e, uint64_t* counters_host, int reset) {
  if (!e || !counters_host) return RNA_EINVAL;
  AstarDevice& a = e->astar;
  if (!a.live()) return fail(e, RNA_ESTATE, "no A* batch has run yet");
  RNA_ENTER(e);
  int rc = sync_all(e);
  if (rc != RNA_OK) return rc;
  unsigned long long all[16];
  if ((rc = tsa_counters_read(e, all, reset != 0)) != RNA_OK) return rc;
  for (int k = 0; k < 8; ++k) counters_host[k] = all[k];
  return RNA_OK;
}

extern "C" int rna_astar_settled_counts(rna_engine* e, int32_t* counts_host, int n) {
  if (!e || !counts_host || n <= 0) return RNA_EINVAL;
  AstarDevice& a = e->astar;
  if (!a.live() || !a.last_queries || n != a.last_n) return fail(e, RNA_ESTATE, "no resident A* batch of that size");
  RNA_ENTER(e);
  int rc = sync_all(e);
  if (rc != RNA_OK) return rc;
  Staging st(e, "rna_astar_settled_counts");
  int32_t* d_counts = st.out(counts_host, (size_t)n);
  if (!st.ok()) return st.finish();
  rc = tsa_settled(e, a.last_slot, a.last_queries, a.last_results, n, d_counts);
  return rc != RNA_OK ? rc : st.finish();
}
