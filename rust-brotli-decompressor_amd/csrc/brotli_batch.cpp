// brotli_batch.cpp -- the batch object (include/brotli/batch.h) on top of the HIP decode kernel: it applies the launch planner's shapes
// (brotli_launch_plan.h), asks the device what kind a batch's streams are where the planner wants to know, runs the later passes for streams
// whose tables did not fit and the settle pass for streams that ran out of output.  It owns no decoder: all decoding happens in
// brotli_kernels.hip.  The host entry points (staging, packed decode) are in brotli_staging.cpp, the reference's C ABI in brotli_capi.cpp.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <new>

#include "brotli_host.h"

extern "C" hipError_t brotli_amd_launch_decode(const BrotliAmdStreamDesc* descs, BrotliAmdStreamStatus* status, uint32_t n_streams,
                                               uint32_t* queue, uint8_t* scratch, uint64_t scratch_per_block, uint32_t grid,
                                               uint32_t lds_arena_bytes, const uint8_t* dict, hipStream_t stream, int waves_per_block);
// (the same kernel with the gang's form of the path engine in it: the launches that give every stream a gang of blocks -- csrc/brotli_kernels.hip, brotli_amd_decode_kernel<true>)
extern "C" hipError_t brotli_amd_launch_decode_gang(const BrotliAmdStreamDesc* descs, BrotliAmdStreamStatus* status, uint32_t n_streams,
                                                    uint32_t* queue, uint8_t* scratch, uint64_t scratch_per_block, uint32_t grid,
                                                    uint32_t lds_arena_bytes, const uint8_t* dict, hipStream_t stream, int waves_per_block);
extern "C" uint32_t brotli_amd_lds_fixed_bytes(void);
extern "C" uint32_t brotli_amd_lds_helper_bytes(uint32_t waves);
extern "C" const uint8_t brotli_amd_dictionary[];  // dict_blob.c: data/dictionary.bin, 122784 bytes
// Test hook: the device's table builder alone (see brotli_amd_debug_build_tree_kernel).
extern "C" hipError_t brotli_amd_launch_debug_build_tree(const uint8_t* d_lengths, uint32_t n_sym, uint16_t* d_decoded, uint32_t* d_entries, hipStream_t stream);

namespace brotli_amd_host {

thread_local std::string g_last_error;
std::atomic<size_t> g_live_bytes[2];

bool hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  g_last_error = std::string(what) + ": " + hipGetErrorString(e);
  return false;
}

bool current_device(int* dev) {
  int count = 0;
  if (!hip_ok(hipGetDeviceCount(&count), "hipGetDeviceCount")) return false;
  if (count <= 0) { g_last_error = "no HIP device present"; return false; }
  return hip_ok(hipGetDevice(dev), "hipGetDevice");
}

}  // namespace brotli_amd_host

using namespace brotli_amd_host;
using namespace brotli_amd_plan;

namespace {

constexpr size_t kDictSize = 122784;
constexpr uint64_t kScratchPerBlock = (2u << 20) + BROTLI_AMD_SPEC_SCRATCH;  // worst-case table arena of one metablock + helper scratch
constexpr uint32_t kDefaultLdsPerBlock = 36 * 1024;
constexpr uint32_t kRoutingFlags = BROTLI_AMD_FLAG_ENGINE_ONLY | BROTLI_AMD_FLAG_DEFER;   // what submit() adds for an engine launch, and a later pass takes off

thread_local std::string g_last_note;   // what a call did differently without failing (engine blocks refused by the device: see launch())

// The environment's knobs (brotli_launch_plan.h says what each does).  The first group is read once per process; the second on every call:
// tests/test_gpu_gang.py flips those inside one process.
BrotliAmdPlanKnobs launch_knobs() {
  const auto num = [](const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; };
  const auto set = [](const char* name) { return getenv(name) != nullptr ? 1u : 0u; };
  static const BrotliAmdPlanKnobs once = [&] {
    BrotliAmdPlanKnobs k = {};
    k.max_blocks_per_cu = (uint32_t)num("BROTLI_AMD_MAX_BLOCKS_PER_CU", 14);
    k.min_small_arena = (uint32_t)num("BROTLI_AMD_MIN_SMALL_ARENA", 3584);
    k.no_scan = set("BROTLI_AMD_NO_SCAN");
    k.no_engine_queue = set("BROTLI_AMD_NO_ENGINE_QUEUE");
    k.engine_queue_max = (uint32_t)num("BROTLI_AMD_ENGINE_QUEUE_MAX", (int)kEngineQueueMaxPerCu);
    k.no_record_blocks = set("BROTLI_AMD_NO_RECORD_BLOCKS");
    k.no_order = set("BROTLI_AMD_NO_ORDER");
    return k;
  }();
  BrotliAmdPlanKnobs k = once;
  k.gang = num("BROTLI_AMD_GANG", -1);
  k.pool = num("BROTLI_AMD_POOL", -1);
  k.gang_no_helpers = set("BROTLI_AMD_GANG_NO_HELPERS");
  k.debug_probe = set("BROTLI_AMD_DEBUG_PROBE");
  return k;
}

// ---- per-device constant data (the static dictionary): lives as long as the process, outside the owned buffers and their count ----
std::mutex g_dict_mutex;
std::vector<uint8_t*> g_dict_by_device;

const uint8_t* device_dictionary(int dev) {
  std::lock_guard<std::mutex> lock(g_dict_mutex);
  if ((int)g_dict_by_device.size() <= dev) g_dict_by_device.resize(dev + 1, nullptr);
  if (!g_dict_by_device[dev]) {
    uint8_t* p = nullptr;
    if (!hip_ok(hipMalloc(&p, kDictSize + 64), "hipMalloc(dictionary)")) return nullptr;
    if (!hip_ok(hipMemcpy(p, brotli_amd_dictionary, kDictSize, hipMemcpyHostToDevice), "hipMemcpy(dictionary)")) { (void)hipFree(p); return nullptr; }
    g_dict_by_device[dev] = p;
  }
  return g_dict_by_device[dev];
}

bool ensure_scratch(BrotliAmdBatch* b, uint32_t grid) { return b->d_scratch.reserve((size_t)grid * kScratchPerBlock, "hipMalloc(table scratch)"); }

int launch(BrotliAmdBatch* b, hipStream_t stream) {
  // queue header (pull counter, order flag) and, for batches of more streams than blocks, the order
  b->h_order[0] = 0; b->h_order[1] = b->ordered ? 1u : 0u;
  for (int i = 2; i < 16; i++) b->h_order[i] = 0;
  if (b->gang > 1u) {
    const size_t need = (size_t)b->n * BROTLI_AMD_GANG_CTL_BYTES;
    if (!b->d_gang.reserve(need, "hipMalloc(gang control)")) return -1;
    if (!hip_ok(hipMemsetAsync(b->d_gang, 0, need, stream), "hipMemsetAsync(gang control)")) return -1;
    b->h_order[2] = b->gang; b->h_order[4] = (uint32_t)(uintptr_t)b->d_gang.get(); b->h_order[5] = (uint32_t)((uint64_t)(uintptr_t)b->d_gang.get() >> 32);
    b->h_order[6] = launch_knobs().gang_no_helpers;   // (tests: the helper blocks leave at once, the owners must find out and go on alone)
    b->h_order[8] = b->n;   // (a pool: the streams that are not done yet)
  }
  b->last_gang = b->gang;
  if (!hip_ok(hipMemcpyAsync(b->d_queue, b->h_order, sizeof(uint32_t) * (b->ordered ? 16 + (size_t)b->n : 16), hipMemcpyHostToDevice, stream), "hipMemcpyAsync(queue)")) return -1;
  if (!hip_ok(hipEventRecord(b->ev0, stream), "hipEventRecord")) return -1;
  hipError_t le = (b->gang > 1u ? brotli_amd_launch_decode_gang : brotli_amd_launch_decode)(b->d_descs, b->d_status, b->n, b->d_queue, b->d_scratch, kScratchPerBlock, b->grid, b->cur_arena,
                                                                                             b->d_dict, stream, (int)b->waves);
  if (b->waves == 16u && (le == hipErrorInvalidValue || le == hipErrorLaunchOutOfResources || le == hipErrorSharedObjectInitFailed || le == hipErrorInvalidConfiguration)) {
    // the device refused a block of sixteen waves with the engine's LDS although its properties allow one: this context goes
    // on with blocks of eight waves, and says so (BrotliAmdLastNote); streams are no longer sent back for engine blocks
    (void)hipGetLastError();
    g_last_note = std::string("engine blocks refused (") + hipGetErrorString(le) + "): eight-wave blocks from now on";   // (a note, not an error: the retry below decides)
    b->dev.engine_ok = 0;
    b->waves = 8;
    if (b->gang > 1u) {   // (the gangs' helper blocks go with the engine blocks)
      b->gang = 0; b->last_gang = 0; b->grid = std::min(b->n, b->grid);
      b->h_order[2] = 0;
      if (!hip_ok(hipMemcpyAsync(b->d_queue, b->h_order, sizeof(uint32_t) * 16, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(queue)")) return -1;
    }
    for (uint32_t i = 0; i < b->n; i++) b->h_descs[i].flags &= ~kRoutingFlags;
    if (!hip_ok(hipMemcpyAsync(b->d_descs, b->h_descs, sizeof(BrotliAmdStreamDesc) * b->n, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(descs)")) return -1;
    le = brotli_amd_launch_decode(b->d_descs, b->d_status, b->n, b->d_queue, b->d_scratch, kScratchPerBlock, b->grid, b->cur_arena, b->d_dict, stream, 8);
  }
  if (!hip_ok(le, "brotli_amd_decode_kernel launch")) return -1;
  if (!hip_ok(hipEventRecord(b->ev1, stream), "hipEventRecord")) return -1;
  b->last_stream = stream;
  b->launched = true;
  b->outputs = BrotliAmdBatch::Outputs::InFlight;
  return 0;
}

// What kind of stream is each of the batch's?  A launch of the shape at hand in which nothing is decoded: every stream's header is read up
// to the literal context map of its first compressed metablock (BROTLI_AMD_FLAG_PROBE) -- where that says 'an engine's kind', on through its literal codes
// and its first command code.  kind[i]: bit 0 there is such a metablock, bit 1 its literals do not depend on context, bit 2 it is large enough for a
// command engine, bit 3 (round 6) its commands are SHORT -- text: the engines' kind by the first three, and yet four such streams a CU on a wave each with
// the command records (lean_rec_commands) do 2.4 times what an engine block does with them one after the other: they are not sent to engine blocks.  (Round 4 guessed from the batch's size and its
// mean compressed size: 1024 x 1 MiB of engine-shaped streams went through one-wave blocks -- 129 GB/s where engine blocks do 148 --, and
// could not be told from 1024 context-modelled texts, which engine blocks take at half speed.  The probe costs a launch of some tens of
// microseconds and reads the facts.)
int probe_streams(BrotliAmdBatch* b, uint32_t n, hipStream_t stream, std::vector<uint8_t>& kind) {
  kind.assign(n, 0);
  if (!ensure_scratch(b, b->grid)) return -1;
  for (uint32_t i = 0; i < n; i++) b->h_descs[i].flags |= BROTLI_AMD_FLAG_PROBE;
  bool ok = hip_ok(hipMemcpyAsync(b->d_descs, b->h_descs, sizeof(BrotliAmdStreamDesc) * n, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(descs)");
  ok = ok && hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize(probe descs)");   // (pinned memory: the copy reads it when it runs, not when it is asked for)
  for (uint32_t i = 0; i < n; i++) b->h_descs[i].flags &= ~BROTLI_AMD_FLAG_PROBE;
  ok = ok && hip_ok(hipMemsetAsync(b->d_queue, 0, sizeof(uint32_t) * 16, stream), "hipMemsetAsync(queue)");
  ok = ok && hip_ok(brotli_amd_launch_decode(b->d_descs, b->d_status, n, b->d_queue, b->d_scratch, kScratchPerBlock, b->grid, b->cur_arena, b->d_dict, stream, (int)b->waves),
                    "brotli_amd_decode_kernel launch (probe)");
  ok = ok && hip_ok(hipMemcpyAsync(b->h_status, b->d_status, sizeof(BrotliAmdStreamStatus) * n, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(status)");
  ok = ok && hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize(probe)");
  if (!ok) return -1;
  for (uint32_t i = 0; i < n; i++) if (b->h_status[i].result == BROTLI_AMD_RESULT_PROBE) kind[i] = (uint8_t)(b->h_status[i].engine_commands & 15u);
  return 0;
}

void print_probe(const BrotliAmdBatch* b, uint32_t n, const std::vector<uint8_t>& kind) {   // BROTLI_AMD_DEBUG_PROBE
  uint64_t in_total = 0, in_engine = 0;
  uint32_t h[16] = {}, r[8] = {};
  for (uint32_t i = 0; i < n; i++) {
    in_total += b->h_descs[i].in_size;
    if (kind[i] == 7u) in_engine += b->h_descs[i].in_size;
    h[kind[i] & 15u]++; r[b->h_status[i].result < 8 ? b->h_status[i].result : 7]++;
  }
  fprintf(stderr, "probe: %u streams, kinds", n); for (int k = 0; k < 16; k++) if (h[k]) fprintf(stderr, " %d:%u", k, h[k]);
  fprintf(stderr, "; engine bytes %llu of %llu; results", (unsigned long long)in_engine, (unsigned long long)in_total);
  for (int k = 0; k < 8; k++) if (r[k]) fprintf(stderr, " %d:%u", k, r[k]);
  fprintf(stderr, "\n");
}

void apply_shape(BrotliAmdBatch* b, const BrotliAmdLaunchPlan& plan) {
  b->grid = plan.grid; b->waves = plan.waves; b->cur_arena = plan.arena; b->cur_per_cu = plan.cur_per_cu;
  b->gang = plan.gang; b->ordered = plan.ordered != 0u;
}

}  // namespace

// The planner says what the launch looks like (brotli_launch_plan.h: plan_launch); where it wants to know first what kind the streams are, and
// the same descriptors have not been asked about before, the device is asked in a launch of the shape the planner gave (probe_streams), and the
// planner is asked again with the answer.  Then the plan is applied: flags, order, scratch, upload, launch.
int brotli_amd_host::submit(BrotliAmdBatch* b, uint32_t n, hipStream_t stream) {  // h_descs[0..n) filled
  if (n == 0) { b->n = 0; b->launched = false; b->outputs = BrotliAmdBatch::Outputs::None; return 0; }
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  const BrotliAmdPlanKnobs knobs = launch_knobs();
  const auto size_at = [b](uint32_t i) { return (uint64_t)b->h_descs[i].in_size; };
  for (uint32_t i = 0; i < n; i++) b->h_descs[i].flags &= ~kRoutingFlags;
  b->last_probe_ms = 0.0f;
  b->n = n;
  std::vector<uint8_t> kind;
  BrotliAmdLaunchPlan plan = plan_launch(b->dev, knobs, b->per_cu_cap, n, size_at, nullptr);
  if (plan.want_probe) {   // ... but not twice for the same descriptors
    uint64_t key = 0xcbf29ce484222325ull ^ n;
    for (uint32_t i = 0; i < n; i++)
      for (uint64_t v : {(uint64_t)(uintptr_t)b->h_descs[i].in, (uint64_t)b->h_descs[i].in_size, (uint64_t)b->h_descs[i].flags,
                         (uint64_t)(uintptr_t)b->h_descs[i].dict, (uint64_t)b->h_descs[i].dict_size}) key = (key ^ v) * 0x100000001b3ull;
    if (b->probe_kind.size() == n && b->probe_key == key) kind = b->probe_kind;
    else {
      apply_shape(b, plan);
      if (!ensure_scratch(b, b->grid)) return -1;   // (a batch object's first launch allocates its blocks' scratch: not the probe's time)
      const auto t0 = std::chrono::steady_clock::now();
      if (probe_streams(b, n, stream, kind) != 0) return -1;
      b->last_probe_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
      b->probe_kind = kind; b->probe_key = key;
    }
    if (knobs.debug_probe) print_probe(b, n, kind);
    plan = plan_launch(b->dev, knobs, b->per_cu_cap, n, size_at, kind.data());
  }
  apply_shape(b, plan);
  if (plan.engine_queue)
    for (uint32_t i = 0; i < n; i++) b->h_descs[i].flags |= kind[i] == 7u ? BROTLI_AMD_FLAG_ENGINE_ONLY : BROTLI_AMD_FLAG_DEFER;
  if (plan.no_spill)
    for (uint32_t i = 0; i < n; i++) if (!(b->h_descs[i].flags & BROTLI_AMD_BATCH_SPILL_IN_PLACE)) b->h_descs[i].flags |= BROTLI_AMD_FLAG_NO_SPILL;
  // (a gang's helper blocks have no scratch of their own -- a slot per stream --, but a launch whose kernel decides against gangs after all
  // (fewer waves than sixteen: experiments) indexes the scratch by block: there is a slot for every block as well)
  if (!ensure_scratch(b, std::max(n, b->grid))) return -1;
  if (b->ordered) {
    uint32_t* order = b->h_order + 16;
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order, order + n, [b](uint32_t x, uint32_t y) { return b->h_descs[x].in_size > b->h_descs[y].in_size; });
  }
  if (!hip_ok(hipMemcpyAsync(b->d_descs, b->h_descs, sizeof(BrotliAmdStreamDesc) * n, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(descs)")) return -1;
  return launch(b, stream);
}

bool brotli_amd_host::decode_descs(BrotliAmdBatch* b, uint32_t n, hipStream_t stream, bool exact_limit) {
  b->exact_limit = exact_limit;
  return submit(b, n, stream) == 0 && BrotliAmdBatchWait(b, nullptr) == 0;
}

void brotli_amd_host::drop_packed(BrotliAmdBatch* b) {
  b->packed_out = nullptr; b->packed_valid = false; b->packed_offsets.clear();
  b->last_packed_launches = b->last_packed_copies = 0; b->packed_ms = 0.0f;
  b->outputs = BrotliAmdBatch::Outputs::Failed;   // (until the call gets as far as a launch, or turns out to have no streams)
}

namespace {

// m descriptors in h_retry_descs -> h_retry_status, in a launch of the given shape on the job's stream (kernel time added to retry_ms);
// m == 0: the pass's buffers only
int run_retry_descs(BrotliAmdBatch* b, uint32_t m, uint32_t arena, uint32_t grid_max, int waves) {
  if (!b->h_retry_status) {   // (the last of the four)
    const size_t descs = sizeof(BrotliAmdStreamDesc) * b->max_streams, status = sizeof(BrotliAmdStreamStatus) * b->max_streams;
    if (!b->d_retry_descs.reserve(descs, "hipMalloc(retry descs)") || !b->d_retry_status.reserve(status, "hipMalloc(retry status)") ||
        !b->h_retry_descs.reserve(descs, "hipHostMalloc(retry descs)") || !b->h_retry_status.reserve(status, "hipHostMalloc(retry status)")) return -1;
  }
  if (m == 0) return 0;
  const uint32_t grid = std::min(m, grid_max);
  hipStream_t stream = b->last_stream;
  if (!ensure_scratch(b, std::max(grid, b->grid))) return -1;
  if (!hip_ok(hipMemcpyAsync(b->d_retry_descs, b->h_retry_descs, sizeof(BrotliAmdStreamDesc) * m, hipMemcpyHostToDevice, stream), "hipMemcpyAsync(retry descs)")) return -1;
  if (!hip_ok(hipMemsetAsync(b->d_queue, 0, sizeof(uint32_t) * 16, stream), "hipMemsetAsync(queue)")) return -1;
  if (!hip_ok(hipEventRecord(b->ev2, stream), "hipEventRecord")) return -1;
  if (!hip_ok(brotli_amd_launch_decode(b->d_retry_descs, b->d_retry_status, m, b->d_queue, b->d_scratch, kScratchPerBlock, grid, arena,
                                       b->d_dict, stream, waves), "brotli_amd_decode_kernel launch (later pass)")) return -1;
  if (!hip_ok(hipEventRecord(b->ev3, stream), "hipEventRecord")) return -1;
  if (!hip_ok(hipMemcpyAsync(b->h_retry_status, b->d_retry_status, sizeof(BrotliAmdStreamStatus) * m, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync(retry status)")) return -1;
  if (!hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize")) return -1;
  { float ms = 0.0f; if (hipEventElapsedTime(&ms, b->ev2, b->ev3) == hipSuccess) b->retry_ms += ms; }
  return 0;
}

// A stream's counters over the pass that stopped and the pass that went on from there (spilled_metablocks: the later pass's alone).
BrotliAmdStreamStatus sum_over_passes(const BrotliAmdStreamStatus& first, BrotliAmdStreamStatus next) {
  next.num_metablocks += first.num_metablocks;  // (the metablock a pass stopped in front of is counted by the pass that decodes it)
  next.num_commands += first.num_commands;
  next.engine_commands += first.engine_commands;
  next.peak_trees = std::max(next.peak_trees, first.peak_trees); next.peak_map_bytes = std::max(next.peak_map_bytes, first.peak_map_bytes);
  next.any_compressed |= first.any_compressed;
  return next;
}

// Streams that came back with BROTLI_AMD_RESULT_RETRY_ARENA continue, from the metablock boundary they stopped at, in
// a launch whose blocks have a larger LDS arena (fewer blocks per CU), level by level (brotli_launch_plan.h: plan_later_pass); each pass takes
// only what the one before could not hold.
int retry_with_larger_arenas(BrotliAmdBatch* b) {
  b->last_retry_count = 0;
  b->retry_ms = 0.0f;
  uint32_t level = b->cur_per_cu;  // 0: the first pass had the configured arena already
  bool many_came_back = false;
  for (int pass = 0; pass < 4; pass++) {
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < b->n; i++) if (b->h_status[i].result == BROTLI_AMD_RESULT_RETRY_ARENA) idx.push_back(i);
    const uint32_t m = (uint32_t)idx.size();
    // a good part of the batch did not fit the first pass: later batches of this object start with the shape that
    // did hold (nearly) all of it
    if (many_came_back && m <= b->n / 16) { b->per_cu_cap = std::max(4u, level); many_came_back = false; }
    if (idx.empty()) return 0;
    if (pass == 0) {
      b->last_retry_count = m;
      many_came_back = level > 4u && m > b->n / 16;
    }
    if (run_retry_descs(b, 0, 0, 0, 0) != 0) return -1;  // (allocates the pass's buffers)
    bool deferred = false;   // streams an engine launch sent back unread (BROTLI_AMD_FLAG_DEFER): the launch of small blocks they were promised
    if (pass == 0) for (uint32_t j = 0; j < m && !deferred; j++) deferred = (b->h_descs[idx[j]].flags & BROTLI_AMD_FLAG_DEFER) != 0u;
    const BrotliAmdLaterPass shape = plan_later_pass(b->dev, launch_knobs(), b->per_cu_cap, level, b->cur_arena, m, deferred);
    level = shape.level;
    for (uint32_t j = 0; j < m; j++) {
      BrotliAmdStreamDesc d = b->h_descs[idx[j]];
      d.flags = ((shape.last ? d.flags & ~BROTLI_AMD_FLAG_NO_SPILL : d.flags) & ~kRoutingFlags) | BROTLI_AMD_FLAG_RESUME;
      // (a stream sent back unread -- BROTLI_AMD_FLAG_DEFER -- reports no boundary at all: one that came RESUMED, a streaming state in a stream set's launch,
      // goes on from the boundary it came with, not from byte 0, which its buffers may no longer hold)
      if (b->h_status[idx[j]].resume.window_bits != 0u || !(b->h_descs[idx[j]].flags & BROTLI_AMD_FLAG_RESUME)) d.resume = b->h_status[idx[j]].resume;
      b->h_retry_descs[j] = d;
    }
    if (run_retry_descs(b, m, shape.arena, shape.grid_max, (int)shape.waves) != 0) return -1;
    for (uint32_t j = 0; j < m; j++) b->h_status[idx[j]] = sum_over_passes(b->h_status[idx[j]], b->h_retry_status[j]);
    if (shape.last) { if (many_came_back) b->per_cu_cap = 4; return 0; }
  }
  return 0;
}

// What the reference reports for a stream whose output buffer is too small depends on what the stream does up to its next
// ring-buffer flush point: it decodes into its ring and only notices the full buffer when it flushes (decode.rs:1693-1738;
// the driver ignores NEEDS_MORE_OUTPUT from the flush it forces when the input ends, decode.rs BrotliDecompressStream), so
// an error or the end of the input in front of that point wins over NEEDS_MORE_OUTPUT.  The kernel stops where the
// buffer ends; the streams it reports NEEDS_MORE_OUTPUT for are decoded once more, into scratch memory with room up to
// the flush point, and that outcome is mapped (the bytes in the caller's buffer stay: they are the same).
constexpr size_t kSettleChunkBytes = (size_t)2 << 30;
int settle_output_limits(BrotliAmdBatch* b) {
  b->last_settle_count = 0;
  std::vector<uint32_t> idx;
  for (uint32_t i = 0; i < b->n; i++)
    if (b->h_status[i].result == BROTLI_DECODER_RESULT_NEEDS_MORE_OUTPUT && b->h_status[i].ring_bytes != 0) idx.push_back(i);
  size_t at = 0;
  while (at < idx.size()) {
    // a chunk of streams whose scratch outputs fit the budget together (a single stream beyond it keeps the kernel's verdict)
    std::vector<uint32_t> part; std::vector<size_t> off, cap2s; size_t total = 0;
    for (; at < idx.size(); at++) {
      const BrotliAmdStreamDesc& d0 = b->h_descs[idx[at]];
      const uint64_t cap2 = flush_point_cap(d0.out_cap, b->h_status[idx[at]].ring_bytes);
      if (cap2 <= d0.out_cap) continue;  // (the buffer ends right in front of the flush point: nothing more to find out)
      const size_t need = (size_t)((cap2 + 255) & ~(uint64_t)255);
      if (need > kSettleChunkBytes) continue;
      if (total + need > kSettleChunkBytes && !part.empty()) break;
      part.push_back(idx[at]); off.push_back(total); cap2s.push_back((size_t)cap2); total += need;
    }
    if (part.empty()) continue;
    if (!b->d_settle.reserve(total, nullptr)) return 0;  // (no memory for it: the kernel's verdict stands)
    const uint32_t m = (uint32_t)part.size();
    if (run_retry_descs(b, 0, 0, 0, 0) != 0) return -1;
    for (uint32_t j = 0; j < m; j++) {
      BrotliAmdStreamDesc d = b->h_descs[part[j]];
      d.flags &= ~(BROTLI_AMD_FLAG_NO_SPILL | kRoutingFlags | BROTLI_AMD_FLAG_RESUME);
      d.out = b->d_settle + off[j]; d.out_cap = cap2s[j];
      b->h_retry_descs[j] = d;
    }
    if (run_retry_descs(b, m, b->dev.max_arena, b->dev.retry_grid_max, 4) != 0) return -1;
    for (uint32_t j = 0; j < m; j++) {
      BrotliAmdStreamStatus& st = b->h_status[part[j]];
      const BrotliAmdStreamStatus& st2 = b->h_retry_status[j];
      if (second_verdict_wins(st2, cap2s[j])) {
        const uint64_t produced = st.produced;
        st = st2;
        st.decoded_size = std::min<uint64_t>(st2.decoded_size, b->h_descs[part[j]].out_cap);
        st.produced = produced;  // (bytes in the caller's buffer)
      }
    }
    b->last_settle_count += m;
  }
  if (b->d_settle.capacity() > ((size_t)64 << 20)) b->d_settle.release();  // (a large scratch buffer is not kept for the next batch)
  return 0;
}

}  // namespace

extern "C" BrotliAmdBatch* BrotliAmdBatchCreate(uint32_t max_streams, uint32_t lds_arena_bytes, uint32_t grid_blocks) {
  DeviceGuard guard;
  int dev = 0;
  if (!current_device(&dev)) return nullptr;
  if (max_streams == 0) max_streams = 1;
  BrotliAmdBatch* b = new (std::nothrow) BrotliAmdBatch();
  if (!b) return nullptr;
  b->device = dev;
  b->max_streams = max_streams;
  hipDeviceProp_t prop;
  if (!hip_ok(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties")) { delete b; return nullptr; }
  const BrotliAmdPlanKnobs knobs = launch_knobs();
  BrotliAmdPlanDevice& d = b->dev;
  // LDS of a block = fixed carve + table arena (+ what the helper waves leave for each other, in blocks that have them)
  const uint32_t fixed = brotli_amd_lds_fixed_bytes(), helper = brotli_amd_lds_helper_bytes(4);
  uint32_t per_block = lds_arena_bytes ? lds_arena_bytes + fixed + helper : kDefaultLdsPerBlock;
  const size_t lds_cu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 65536;
  if (per_block > prop.sharedMemPerBlock && prop.sharedMemPerBlock) per_block = (uint32_t)prop.sharedMemPerBlock;
  d.lds_arena = (per_block - fixed - helper) & ~15u;
  b->cur_arena = d.lds_arena;
  d.auto_arena = lds_arena_bytes == 0;
  b->per_cu_cap = knobs.max_blocks_per_cu;
  d.cus = (uint32_t)prop.multiProcessorCount; d.lds_fixed = fixed; d.lds_per_cu = (uint32_t)lds_cu;
  d.lds_helper4 = helper; d.lds_helper8 = brotli_amd_lds_helper_bytes(8); d.lds_helper16 = brotli_amd_lds_helper_bytes(16);
  // the arena of the last pass: the largest block the device allows (at most 64 KiB: two such blocks per CU at least)
  d.block_max = (uint32_t)std::min<size_t>(prop.sharedMemPerBlock ? prop.sharedMemPerBlock : 65536, 65536);
  d.engine_ok = !knobs.no_scan && lds_cu >= (size_t)fixed + d.lds_helper16 + 16384u;
  d.max_arena = d.block_max > fixed + helper ? (d.block_max - fixed - helper) & ~15u : 0;
  d.retry_grid_max = d.cus * (uint32_t)std::max<size_t>(1, lds_cu / d.block_max);
  const uint32_t blocks_per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(knobs.max_blocks_per_cu, lds_cu / per_block));
  d.grid_max = grid_blocks ? grid_blocks : d.cus * blocks_per_cu;
  b->d_dict = device_dictionary(dev);
  const size_t descs = sizeof(BrotliAmdStreamDesc) * max_streams, status = sizeof(BrotliAmdStreamStatus) * max_streams, queue = sizeof(uint32_t) * (16 + (size_t)max_streams);
  bool ok = b->d_dict != nullptr;
  ok = ok && b->d_descs.reserve(descs, "hipMalloc(descs)") && b->d_status.reserve(status, "hipMalloc(status)") && b->d_queue.reserve(queue, "hipMalloc(queue)");
  ok = ok && b->h_descs.reserve(descs, "hipHostMalloc(descs)") && b->h_status.reserve(status, "hipHostMalloc(status)") && b->h_order.reserve(queue, "hipHostMalloc(order)");
  ok = ok && hip_ok(hipEventCreate(&b->ev0), "hipEventCreate") && hip_ok(hipEventCreate(&b->ev1), "hipEventCreate");
  ok = ok && hip_ok(hipEventCreate(&b->ev2), "hipEventCreate") && hip_ok(hipEventCreate(&b->ev3), "hipEventCreate");
  ok = ok && hip_ok(hipMemset(b->d_status, 0, status), "hipMemset(status)");
  if (ok) std::memset(b->h_status, 0, status);
  if (!ok) { BrotliAmdBatchDestroy(b); return nullptr; }
  return b;
}

// The order: the object's device, a wait for its last stream (or the device), then everything it owns -- the buffers by destruction.
extern "C" void BrotliAmdBatchDestroy(BrotliAmdBatch* b) {
  if (!b) return;
  DeviceGuard guard;
  (void)hipSetDevice(b->device);
  if (b->launched && b->last_stream != nullptr) (void)hipStreamSynchronize(b->last_stream);
  else (void)hipDeviceSynchronize();
  if (b->copy_stream) (void)hipStreamDestroy(b->copy_stream);
  for (hipEvent_t ev : {b->ev0, b->ev1, b->ev2, b->ev3}) if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : b->digest.ev) if (ev) (void)hipEventDestroy(ev);
  for (BrotliAmdBatch::FilterCall& f : b->filter)
    for (hipEvent_t ev : f.call.ev) if (ev) (void)hipEventDestroy(ev);
  delete b;
}

extern "C" int BrotliAmdBatchDecodeDeviceDict(BrotliAmdBatch* b, uint32_t n, const void* const* d_in, const size_t* in_sizes, void* const* d_out,
                                              const size_t* out_caps, const void* const* d_dicts, const size_t* dict_sizes, uint32_t flags,
                                              void* hip_stream) {
  if (!b || n > b->max_streams || (n && (!d_in || !in_sizes || !d_out || !out_caps))) { g_last_error = "invalid batch arguments"; return -1; }
  drop_packed(b);
  DeviceGuard guard;
  const bool dicts = d_dicts && dict_sizes;
  for (uint32_t i = 0; i < n; i++) b->h_descs[i] = make_desc(d_in[i], in_sizes[i], d_out[i], out_caps[i], flags, dicts ? d_dicts[i] : nullptr, dicts ? dict_sizes[i] : 0);
  b->exact_limit = !(flags & BROTLI_AMD_BATCH_EAGER_OUTPUT_LIMIT);
  return submit(b, n, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchDecodeDevice(BrotliAmdBatch* b, uint32_t n, const void* const* d_in, const size_t* in_sizes, void* const* d_out,
                                          const size_t* out_caps, uint32_t flags, void* hip_stream) {
  return BrotliAmdBatchDecodeDeviceDict(b, n, d_in, in_sizes, d_out, out_caps, nullptr, nullptr, flags, hip_stream);
}

extern "C" int BrotliAmdBatchRelaunch(BrotliAmdBatch* b, void* hip_stream) {
  if (!b || b->n == 0) { g_last_error = "nothing to relaunch"; return -1; }
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  return launch(b, static_cast<hipStream_t>(hip_stream));
}

extern "C" int BrotliAmdBatchWait(BrotliAmdBatch* b, BrotliAmdResult* results) {
  if (!b) return -1;
  if (b->n == 0 || !b->launched) return 0;
  DeviceGuard guard;
  if (!hip_ok(hipSetDevice(b->device), "hipSetDevice")) return -1;
  if (!hip_ok(hipMemcpyAsync(b->h_status, b->d_status, sizeof(BrotliAmdStreamStatus) * b->n, hipMemcpyDeviceToHost, b->last_stream), "hipMemcpyAsync(status)")) return -1;
  if (!hip_ok(hipStreamSynchronize(b->last_stream), "hipStreamSynchronize")) return -1;
  if (retry_with_larger_arenas(b) != 0) return -1;
  if (b->exact_limit && settle_output_limits(b) != 0) return -1;
  b->outputs = BrotliAmdBatch::Outputs::Waited;
  if (results) for (uint32_t i = 0; i < b->n; i++) results[i] = to_result(b->h_status[i]);
  return 0;
}

extern "C" uint32_t BrotliAmdBatchLastSecondPassCount(BrotliAmdBatch* b) { return b ? b->last_retry_count : 0; }
extern "C" uint32_t BrotliAmdBatchLastGang(BrotliAmdBatch* b) { return b ? (b->last_gang > 1u && b->last_gang <= 16u ? b->last_gang : 1u) : 0; }
extern "C" float BrotliAmdBatchLastProbeMs(BrotliAmdBatch* b) { return b ? b->last_probe_ms : 0.0f; }
extern "C" uint32_t BrotliAmdBatchLastPool(BrotliAmdBatch* b) { return b && (b->last_gang & BROTLI_AMD_GANG_POOL_FLAG) != 0u ? 1u : 0u; }

extern "C" float BrotliAmdBatchLastKernelMs(BrotliAmdBatch* b) {
  if (b && b->packed_valid) return b->packed_ms;   // (a packed call: all its decode launches)
  if (!b || !b->launched) return 0.0f;
  float ms = 0.0f;
  if (!hip_ok(hipEventSynchronize(b->ev1), "hipEventSynchronize")) return -1.0f;
  if (!hip_ok(hipEventElapsedTime(&ms, b->ev0, b->ev1), "hipEventElapsedTime")) return -1.0f;
  return ms + b->retry_ms;
}

extern "C" const char* BrotliAmdLastError(void) { return g_last_error.c_str(); }
extern "C" const char* BrotliAmdLastNote(void) { return g_last_note.c_str(); }

// ---- test hooks: the planner without a device ----
extern "C" uint32_t BrotliAmdDebugPlanGangs(uint32_t n, uint32_t cus, const size_t* in_sizes, int gang_env, int pool_env, uint32_t* grid) {
  uint32_t g = n;
  const uint32_t r = (n != 0u && in_sizes != nullptr) ? plan_gangs(n, cus, in_sizes, gang_env, pool_env, &g) : 0u;
  if (grid) *grid = g;
  return r;
}
extern "C" int BrotliAmdDebugPlanLaunch(const BrotliAmdPlanDevice* dev, const BrotliAmdPlanKnobs* knobs, uint32_t per_cu_cap, uint32_t n,
                                        const size_t* in_sizes, const uint8_t* kinds, BrotliAmdLaunchPlan* plan) {
  if (!dev || !knobs || !plan || n == 0u || !in_sizes || dev->cus == 0u) return -1;
  *plan = plan_launch(*dev, *knobs, per_cu_cap, n, [in_sizes](uint32_t i) { return (uint64_t)in_sizes[i]; }, kinds);
  return 0;
}
extern "C" int BrotliAmdDebugPlanLaterPass(const BrotliAmdPlanDevice* dev, const BrotliAmdPlanKnobs* knobs, uint32_t per_cu_cap, uint32_t level,
                                           uint32_t cur_arena, uint32_t m, int deferred, BrotliAmdLaterPass* pass) {
  if (!dev || !knobs || !pass || dev->cus == 0u) return -1;
  *pass = plan_later_pass(*dev, *knobs, per_cu_cap, level, cur_arena, m, deferred != 0);
  return 0;
}

// Test hook, not in the public headers: bytes the host side holds at the moment -- device memory, pinned host memory (the per-device
// dictionary, which stays for the life of the process, is not counted).  Back at its earlier value once every object is destroyed.
extern "C" __attribute__((visibility("default"))) void brotli_amd_debug_live_bytes(size_t* device_bytes, size_t* pinned_bytes) {
  if (device_bytes) *device_bytes = g_live_bytes[(int)Mem::Device].load();
  if (pinned_bytes) *pinned_bytes = g_live_bytes[(int)Mem::Pinned].load();
}

extern "C" int BrotliAmdDebugBuildTree(const uint8_t* code_lengths, uint32_t alphabet_size, uint16_t* decoded, uint32_t* table_entries) {
  if (code_lengths == nullptr || decoded == nullptr || table_entries == nullptr || alphabet_size == 0u || alphabet_size > 1128u) return -1;
  DevBuf<> d_len; DevBuf<uint16_t> d_dec; DevBuf<uint32_t> d_n;
  bool ok = d_len.reserve(alphabet_size, "hipMalloc") && d_dec.reserve(32768 * sizeof(uint16_t), "hipMalloc") && d_n.reserve(sizeof(uint32_t), "hipMalloc");
  ok = ok && hip_ok(hipMemcpy(d_len, code_lengths, alphabet_size, hipMemcpyHostToDevice), "hipMemcpy");
  ok = ok && hip_ok(brotli_amd_launch_debug_build_tree(d_len, alphabet_size, d_dec, d_n, nullptr), "brotli_amd_debug_build_tree_kernel launch");
  ok = ok && hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
  ok = ok && hip_ok(hipMemcpy(decoded, d_dec, 32768 * sizeof(uint16_t), hipMemcpyDeviceToHost), "hipMemcpy") && hip_ok(hipMemcpy(table_entries, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy");
  return ok && *table_entries != 0u ? 0 : -1;
}
