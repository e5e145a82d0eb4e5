// art_enqueue.cpp — the kernels of one frame on one device: the raytrace, permeation and reduce
// stages with their side streams and timing events, and one device's share of a host-API frame
// (copies in, kernels, copies out, completion event).
#include "art_ctx.hpp"

namespace art {

hipEvent_t pool_event(Device& dv, size_t i) {
  while (dv.ev_pool.size() <= i) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    dv.ev_pool.push_back(e);
  }
  return dv.ev_pool[i];
}

// A timing event pair of kind `kind` opened on stream `on` (its pool index) and closed.
static size_t time_start(Device& dv, int kind, hipStream_t on) {
  size_t i = dv.ev_used.size() * 2;
  hipEvent_t e = pool_event(dv, i);
  pool_event(dv, i + 1);
  if (e) (void)hipEventRecord(e, on);
  dv.ev_used.push_back({kind, i});
  return i;
}
static void time_stop(Device& dv, size_t i, hipStream_t on) {
  hipEvent_t e = pool_event(dv, i + 1);
  if (e) (void)hipEventRecord(e, on);
}

// The throughput raytrace stage of fp.S fans on st. The pair arrays index pairs with 32-bit slots
// (below 2^31) and the echo outputs with 32-bit half offsets into the block: larger frames run as
// consecutive fan chunks on st (the pair buffer and counters are reused, the muffle accumulators
// offset per chunk).
static void raytrace_fast(Device& dv, const Frame& f, const FrameParams& fp, const float* d_origins, uint8_t* d_block,
                          uint32_t* acc, uint32_t* pair_count, hipStream_t st, bool mark_each) {
  const int fan_count = fp.S, chunk = fast_fans_per_launch(f.R, f.H, f.T, f.TC, f.L.stride);
  const int* order = reinterpret_cast<const int*>(static_cast<const uint8_t*>(dv.raw.p) + f.off_order);
  // per-kernel marks (ART_CTX_TIME_EACH_KERNEL): pool pairs after the stage's own, kept for
  // those recorded; a frame has at most 3H + 2 stage kernels per fan chunk
  KernelMarks marks;
  std::vector<hipEvent_t> mev;
  std::vector<int> mkind;
  if (mark_each) {
    const size_t base = dv.ev_used.size() * 2;
    marks.cap = (3 * f.H + 2) * ((fan_count + chunk - 1) / chunk);
    for (int k = 0; k < 2 * marks.cap; ++k) {
      hipEvent_t e = pool_event(dv, base + k);
      if (!e) { marks.cap = k / 2; break; }
      mev.push_back(e);
    }
    mkind.assign((size_t)marks.cap, 0);
    marks.ev = mev.data();
    marks.kind = mkind.data();
  }
  dv.last_plan = fan_count > chunk ? ART_PLAN_CHUNKED : 0u;
  for (int b0 = 0; b0 < fan_count; b0 += chunk) {
    FrameParams fpc = fp;
    fpc.S = std::min(chunk, fan_count - b0);
    dv.last_plan |= launch_raytrace_fast(dv.sc, fpc, f.L, d_origins + 3 * (size_t)b0, d_block + (size_t)b0 * f.L.stride,
                                         acc + (size_t)b0 * (size_t)f.TC * f.T, order, dv.pairs.p, pair_count, st, dv.echo,
                                         marks.cap ? &marks : nullptr, b0 == 0);
  }
  dv.echo_decided = reinterpret_cast<const unsigned long long*>(pair_count + 4);
  for (int k = 0; k < marks.used; ++k)  // pool index base + 2 k
    dv.ev_used.push_back({kEvKernel0 + mkind[(size_t)k], dv.ev_used.size() * 2});
  dv.marks_dropped += marks.dropped;
}

// Enqueue the kernels of one frame for fan_count fans on stream st.
int enqueue_kernels(art_ctx* c, Device& dv, const Frame& f, const float* d_origins, int fan_count, uint8_t* d_block,
                    hipStream_t st, bool count, const float* perm_in, uint8_t* host_out) {
  if (fan_count == 0) return ART_OK;
  const bool timing = (c->flags & ART_CTX_TIME_KERNELS) && !count;
  FrameParams fp = f.fp;
  fp.S = fan_count;
  const uint8_t* raw = static_cast<const uint8_t*>(dv.raw.p);
  fp.vol_curve = reinterpret_cast<const float*>(raw + f.off_vol);
  fp.muf_curve = reinterpret_cast<const float*>(raw + f.off_muf);
  const int2* slot_batch = reinterpret_cast<const int2*>(raw + f.off_tab);
  const uint8_t* muffle_reset = raw + f.off_reset;
  const bool fast = (f.stages & ART_STAGE_RAYTRACE) && !count && !(c->flags & ART_CTX_FORCE_REFERENCE_ORDER);
  dv.last_plan = 0;  // (raytrace_fast sets it)
  dv.echo_decided = nullptr;
  const size_t acc_per_fan = (size_t)f.TC * f.T;
  // muffle accumulators, then (16-B aligned) the visibility pair counters: cleared by the first
  // nearest_first_kernel of each fast-path chunk, by one memset before the reference-order kernel
  const size_t acc_words = ((size_t)fan_count * acc_per_fan + 3) & ~(size_t)3;
  const size_t acc_bytes = acc_words * sizeof(uint32_t) + 16 + 8 * kEchoCountSlots;  // + 4 pair counters + the echo replay's counts
  // (room for the scene's target capacity, so that a count change within it allocates nothing)
  const size_t acc_room = ((((size_t)fan_count * f.TC * f.tcap() + 3) & ~(size_t)3)) * sizeof(uint32_t) + 16 + 8 * kEchoCountSlots;
  if (!dv.acc.reserve(std::max(acc_bytes, acc_room))) return fail(c, ART_E_NOMEM, "device allocation failed");
  uint32_t* acc = static_cast<uint32_t*>(dv.acc.p);
  uint32_t* pair_count = acc + acc_words;
  DevCounts* counts = nullptr;
  unsigned long long* nhit = nullptr;
  if (count) {
    if (!dv.counts.reserve(sizeof(DevCounts) + 16)) return fail(c, ART_E_NOMEM, "device allocation failed");
    counts = static_cast<DevCounts*>(dv.counts.p);
    nhit = reinterpret_cast<unsigned long long*>(static_cast<uint8_t*>(dv.counts.p) + sizeof(DevCounts));
    HIP_TRY(c, hipMemsetAsync(dv.counts.p, 0, sizeof(DevCounts) + 16, st));
  }
  // Everything the stages allocate or create comes first: once the permeation job is forked to the
  // side stream, an early error return would leave it writing the caller's block unjoined.
  // the permeation job over the BVH (art_permeate.hip); reference-order and counting frames sweep every
  // collider (art_kernels.hip), an independent implementation the parity tests compare too
  const bool perm_bvh = !count && !(c->flags & ART_CTX_FORCE_REFERENCE_ORDER);
  const int chunk = fast_fans_per_launch(f.R, f.H, f.T, f.TC, f.L.stride);
  if (fast) {
    if ((c->flags & ART_CTX_COUNT_EXECUTED) && !dv.exec.p) {
      if (!dv.exec.reserve(8 * kExecSlots)) return fail(c, ART_E_NOMEM, "device allocation failed");
      HIP_TRY(c, hipMemsetAsync(dv.exec.p, 0, 8 * kExecSlots, st));
    }
    if (int rc = ensure_side(c, dv.echo)) return rc;
    FrameParams fps = fp;
    fps.S = std::min(fan_count, chunk);
    // (the pair buffer depends on T only through the fan chunk, which is largest at T = 1)
    if (f.Tc > 0) fps.S = std::min(fan_count, fast_fans_per_launch(f.R, f.H, 1, f.TC, f.L.stride));
    if (!dv.pairs.reserve(fast_pair_bytes(fps))) return fail(c, ART_E_NOMEM, "device allocation failed");
  }
  // The permeation job (read-only scene and origins, writes only the fans' permeation sections)
  // runs on the side stream concurrently with the raytrace stage, whose kernels leave CUs idle in
  // their tails; the reduce job waits for both. Counting frames stay serial.
  const bool both = (f.stages & ART_STAGE_RAYTRACE) && (f.stages & ART_STAGE_PERMEATE);
  const bool overlap = both && !count;
  if (overlap)
    if (int rc = ensure_side(c, dv.side)) return rc;
  unsigned long long* exec_ctr = nullptr;
  if (fast && (c->flags & ART_CTX_COUNT_EXECUTED)) {
    exec_ctr = static_cast<unsigned long long*>(dv.exec.p);
    dv.exec_launches++;
  }

  // The frame's launch sequence on stream st: stage kernels, side-stream forks and joins.
  // an error return after the fork drains the side stream first (the caller may free d_block)
  struct SideDrain {
    hipStream_t side = nullptr;
    ~SideDrain() { if (side) (void)hipStreamSynchronize(side); }
  } drain;
  if (overlap) {
    drain.side = dv.side.st;
    HIP_TRY(c, hipEventRecord(dv.side.fork, st));
    HIP_TRY(c, hipStreamWaitEvent(dv.side.st, dv.side.fork, 0));
    size_t ti = timing ? time_start(dv, kEvPermeate, dv.side.st) : 0;
    (perm_bvh ? launch_permeate : launch_permeate_sweep)(dv.sc, fp, f.L, d_origins, d_block, slot_batch, dv.side.st);
    if (timing) time_stop(dv, ti, dv.side.st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(dv.side.join, dv.side.st));
  }

  if (f.stages & ART_STAGE_RAYTRACE) {
    size_t ti = timing ? time_start(dv, kEvRaytrace, st) : 0;
    // The counting variant sweeps colliders in exact reference order per lane (its per-lane
    // test counts are the metric's numerator); the throughput kernel splits the sweep over waves.
    if (!fast) {
      HIP_TRY(c, hipMemsetAsync(acc, 0, acc_bytes, st));
      launch_raytrace(dv.sc, fp, f.L, d_origins, d_block, acc, counts, st);
    } else {
      FrameParams fpx = fp;
      fpx.exec = exec_ctr;
      raytrace_fast(dv, f, fpx, d_origins, d_block, acc, pair_count, st, timing && (c->flags & ART_CTX_TIME_EACH_KERNEL));
    }
    if (timing) time_stop(dv, ti, st);
    HIP_TRY(c, hipGetLastError());
  }
  if (overlap) {
    HIP_TRY(c, hipStreamWaitEvent(st, dv.side.join, 0));
    drain.side = nullptr;  // joined: stream order covers it from here
  }
  if ((f.stages & ART_STAGE_PERMEATE) && !overlap) {
    size_t ti = timing ? time_start(dv, kEvPermeate, st) : 0;
    (perm_bvh ? launch_permeate : launch_permeate_sweep)(dv.sc, fp, f.L, d_origins, d_block, slot_batch, st);
    if (timing) time_stop(dv, ti, st);
    HIP_TRY(c, hipGetLastError());
    if (count) {
      launch_perm_count(dv.sc, fp, d_origins, counts, nhit, st);
      HIP_TRY(c, hipGetLastError());
    }
  }
  if (f.stages & (ART_STAGE_RAYTRACE | ART_STAGE_REDUCE)) {
    size_t ti = timing ? time_start(dv, kEvReduce, st) : 0;
    launch_reduce(dv.sc, fp, f.L, d_block, acc, muffle_reset, st, perm_in, (f.stages & ART_STAGE_REDUCE) ? host_out : nullptr);
    if (timing) time_stop(dv, ti, st);
    HIP_TRY(c, hipGetLastError());
  }
  return ART_OK;
}

int read_counts(art_ctx* c, Device& dv, hipStream_t st, art_test_counts* out, bool accumulate) {
  DevCounts h{};
  unsigned long long nhit = 0;
  HIP_TRY(c, hipMemcpyAsync(&h, dv.counts.p, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&nhit, static_cast<uint8_t*>(dv.counts.p) + sizeof(DevCounts), 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (!accumulate) memset(out, 0, sizeof *out);
  out->rt_sphere += h.v[0]; out->rt_aabb += h.v[1]; out->rt_obb += h.v[2];
  out->perm_hit_sphere += h.v[3]; out->perm_hit_aabb += h.v[4]; out->perm_hit_obb += h.v[5];
  if (c->nonowned.size() == 3) {
    out->perm_loss_sphere += nhit * c->nonowned[0];
    out->perm_loss_aabb += nhit * c->nonowned[1];
    out->perm_loss_obb += nhit * c->nonowned[2];
  }
  return ART_OK;
}

// Host-API frames whose slot arrays need no upload (art_schedule): one batch slot (every muffle
// slot is reset by the raytrace stage, the permeation stage rewrites its slot), the raytrace stage
// on, no echo upload, no hit outputs.
bool compact_slots(const Frame& f, bool need_echo) {
  return f.TC == 1 && (f.stages & ART_STAGE_RAYTRACE) && !need_echo && !f.L.has_hits;
}

// One device's share of an art_schedule frame: scene upload, origins and in/out slot arrays H2D,
// kernels, result blocks D2H, completion event (all async on dv.stream).
int enqueue_device_frame(art_ctx* c, Device& dv, const Frame& f, const uint8_t* hin, uint8_t* hb, bool need_echo, bool count,
                         bool inject_failure, PhaseClock* pc) {
  const FanLayout& L = f.L;
  int rc = upload_scene(c, dv, f, hin);
  if (pc) pc->mark(3);
  if (rc) return rc;
  if (inject_failure) {
    dv.last.valid = false;  // the scene upload may not have completed: never reuse it
    return fail(c, ART_E_DEVICE, "injected enqueue failure on shard %d (ART_TEST_FAIL_SHARD)", dv.id);
  }
  if (dv.fan_count == 0) { HIP_TRY(c, hipEventRecord(dv.done, dv.stream)); return ART_OK; }
  const size_t bbytes = (size_t)dv.fan_count * L.stride;
  const size_t tcT = (size_t)f.TC * f.T;
  const bool compact = compact_slots(f, need_echo);
  // compact frames: the origins and (without the permeation stage) the caller's permeation slots in
  // one copy; the block's slot sections are written by the kernels (muffle) or not used (permeation)
  const size_t perm_in_off = align_up((size_t)dv.fan_count * 12, 16);
  const bool perm_in = compact && !(f.stages & ART_STAGE_PERMEATE);
  const size_t in_bytes = perm_in ? perm_in_off + (size_t)dv.fan_count * tcT * 4 : (size_t)dv.fan_count * 12;
  if (!dv.origins.reserve(in_bytes) || !dv.block.reserve(bbytes)) return fail(c, ART_E_NOMEM, "device allocation failed");
  uint8_t* hbs = hb + (size_t)dv.fan_begin * L.stride;
  // the shard's origins (and permeation slots), contiguous in the staging (art_schedule)
  HIP_TRY(c, hipMemcpyAsync(dv.origins.p, hin + dv.in_off, in_bytes, hipMemcpyHostToDevice, dv.stream));
  if (need_echo || L.has_hits) {
    HIP_TRY(c, hipMemcpyAsync(dv.block.p, hbs, bbytes, hipMemcpyHostToDevice, dv.stream));
  } else if (!compact) {  // only the muffle + permeation slot arrays (adjacent in the record)
    HIP_TRY(c, hipMemcpy2DAsync(static_cast<uint8_t*>(dv.block.p) + L.muffle_off, L.stride, hbs + L.muffle_off, L.stride,
                                L.echo_off - L.muffle_off, dv.fan_count, hipMemcpyHostToDevice, dv.stream));
  }
  // the reduce kernel stores each fan's record into the pinned staging itself (no D2H copy) when it
  // runs the reduce stage
  const bool direct = (f.stages & ART_STAGE_REDUCE) && !count;
  rc = enqueue_kernels(c, dv, f, static_cast<const float*>(dv.origins.p), dv.fan_count, static_cast<uint8_t*>(dv.block.p),
                       dv.stream, count,
                       perm_in ? reinterpret_cast<const float*>(static_cast<uint8_t*>(dv.origins.p) + perm_in_off) : nullptr,
                       direct ? hbs : nullptr);
  if (rc) return rc;
  if (!direct) HIP_TRY(c, hipMemcpyAsync(hbs, dv.block.p, bbytes, hipMemcpyDeviceToHost, dv.stream));
  HIP_TRY(c, hipEventRecord(dv.done, dv.stream));
  if (pc) pc->mark(4);
  return ART_OK;
}

}  // namespace art
