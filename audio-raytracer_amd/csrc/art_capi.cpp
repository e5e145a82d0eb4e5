// art_capi.cpp — the C ABI (include/art.h, include/art_device.h) over the HIP kernels.
//
// Replaces the reference's per-frame job scheduling in Audio/AudioRayTracer.cs:161-237:
//   AudioRaytracerJobBatched.Schedule(rayCount, batchSize)           (:191)
//   + AudioPermeationJobBatched.Schedule(rayCount, batchSize)        (:213)
//   + ProcessAudioDataJob.Schedule(handleA), CombineDependencies     (:237)
//   -> art_schedule: H2D of the frame's inputs, prep + raytrace + permeate + reduce kernels on
//      one HIP stream per device, D2H of the packed per-fan result blocks; one event per device.
//   JobHandle.IsCompleted (:95) -> art_is_completed; JobHandle.Complete() (:97) -> art_complete.
// Fans are sharded contiguously over the context's devices (SURVEY.md §8 e); each device holds
// a full copy of the scene. art_create(0) gives the CPU backend instead (art_cpu.cpp): the host
// entry points only, no HIP device needed.
// This unit keeps create / destroy / flags, the frame life cycle (art_schedule, art_is_completed,
// art_complete), the device launch path and the test and debug entry points; art_ctx.hpp names the
// units behind it.
#include <atomic>
#include <cmath>
#include <csignal>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <execinfo.h>
#include <new>

#include "art_ctx.hpp"
#include "art_frame_math.hpp"

using namespace art;

// The ABI structs are byte-identical to the C# structs (App. C of SURVEY.md).
static_assert(sizeof(art_half3) == 6, "half3");
static_assert(sizeof(art_aabb) == 20, "ColliderAABBStruct");
static_assert(sizeof(art_obb) == 26, "ColliderOBBStruct");
static_assert(sizeof(art_sphere) == 16, "ColliderSphereStruct");
static_assert(sizeof(art_target_settings) == 24, "AudioTargetRTSettings");
static_assert(sizeof(art_dsp_params) == 24, "art_dsp_params");

namespace {

// ABI major.minor. A struct that grows is a major bump (a caller built against the older header
// would be written past its end). 2.0: art_fan.ray_hit_ids, art_fan_layout.hit_ids_off; 2.1:
// art_exec_counts.cell_entries / muffle_fallback; 2.2: art_exec_counts.bounce_rays; 2.3:
// art_exec_counts.by_kernel (grew from 208 to 328 B), art_kernel_times.nearest_* (32 to 48 B),
// art_debug_leaf_order, ART_CTX_GRAPH removed — a growth 2.3 should have made a major bump; 3.0:
// art_kernel_times per kernel family (kernel_ms / kernel_launches / kernel_marks_dropped, 80 B),
// ART_CTX_TIME_EACH_KERNEL.
// 3.1: ART_CTX_EVENT_EACH_LAUNCH, art_recip_exact_device; 3.2: art_debug_last_plan, ART_PLAN_*;
// 3.3: art_debug_echo_decided; 3.4: the resident target store (art_target_*, art_targets_*,
// ART_CTX_RESIDENT_TARGETS, art_debug_cells_arena); 3.5: the audio tick (art_listener,
// art_dsp_tick_params_host, art_dsp_settings_bind, art_dsp_tick_params_device, art_dsp_tick_device);
// 3.6: the listener mix (art_dsp_mix_device, art_dsp_tick_mix_device, art_dsp_mix_host); 3.7: targets
// added and removed on a bound scene (art_targets_reserve, art_target_capacity, art_targets_last_resize,
// art_debug_target_sync_map); 3.8: art_debug_sphere_slack; 3.9: art_debug_bvh_records;
// 3.10: colliders added and removed on a bound scene (art_colliders_reserve, art_collider_capacity,
// art_colliders_last_resize); 3.11: art_debug_node_margin_cap; 3.12: art_debug_cells_lists;
// 3.13: per-source data and collider owners follow the targets (art_target_follow_map, art_target_follow_mark,
// art_dsp_sources_follow_host, art_dsp_sources_follow_device, ART_CTX_TARGET_OWNERS_FOLLOW,
// art_target_last_remove_owners); 3.14: art_debug_last_dsp_kernel, ART_DSP_KERNEL_*; 3.15: spatializer
// settings per target (art_dsp_settings_bind_classes, art_dsp_target_classes_set / _get / _follow,
// art_dsp_tick_params_classes_host)
constexpr uint32_t kAbiVersion = (3u << 16) | 15u;

// Per-type sum over targets of colliders NOT owned by the target (permeation loss test counts).
void count_nonowned(art_ctx* c, const art_frame_desc* d) {
  c->nonowned.assign(3, 0);
  if (c->flags & ART_CTX_RESIDENT_COLLIDERS) {  // from the last sync's audio_target_id histograms
    for (int k = 0; k < 3; ++k) {
      uint64_t owned = 0;
      if (!c->store.tid_hist[k].empty())
        for (int t = 0; t < d->audio_target_count && t < 32768; ++t) owned += (uint64_t)c->store.tid_hist[k][(size_t)t + 32768];
      c->nonowned[k] = (uint64_t)d->audio_target_count * (uint64_t)c->store.synced[k] - owned;
    }
    return;
  }
  for (int t = 0; t < d->audio_target_count; ++t) {
    uint64_t os = 0, oa = 0, oo = 0;
    for (int i = 0; i < d->sphere_count; ++i) os += d->sphere_colliders[i].audio_target_id == t;
    for (int i = 0; i < d->aabb_count; ++i) oa += d->aabb_colliders[i].audio_target_id == t;
    for (int i = 0; i < d->obb_count; ++i) oo += d->obb_colliders[i].audio_target_id == t;
    c->nonowned[0] += d->sphere_count - os;
    c->nonowned[1] += d->aabb_count - oa;
    c->nonowned[2] += d->obb_count - oo;
  }
}

// ART_CTX_RESIDENT_COLLIDERS: the desc carries no colliders and the store has been synced.
int check_resident(art_ctx* c, const art_frame_desc* d) {
  if (!(c->flags & ART_CTX_RESIDENT_COLLIDERS)) return ART_OK;
  if (d->sphere_count || d->aabb_count || d->obb_count || d->sphere_colliders || d->aabb_colliders || d->obb_colliders)
    return fail(c, ART_E_INVALID, "ART_CTX_RESIDENT_COLLIDERS: the desc's collider arrays must be NULL / 0");
  if (!c->store.store_synced) return fail(c, ART_E_STATE, "ART_CTX_RESIDENT_COLLIDERS: no art_colliders_sync yet");
  return ART_OK;
}

// ART_CTX_RESIDENT_TARGETS: the desc carries no targets and the store has been synced; the frame
// is then made from `eff`, the desc with the positions and count of the last art_targets_sync (d
// points at it). Without the flag d stays.
int resident_targets_desc(art_ctx* c, const art_frame_desc*& d, art_frame_desc& eff) {
  if (!(c->flags & ART_CTX_RESIDENT_TARGETS)) return ART_OK;
  if (!d) return fail(c, ART_E_INVALID, "desc is NULL");
  if (d->audio_target_positions || d->audio_target_count)
    return fail(c, ART_E_INVALID, "ART_CTX_RESIDENT_TARGETS: the desc's audio_target_positions / count must be NULL / 0");
  if (!c->targets.store_synced) return fail(c, ART_E_STATE, "ART_CTX_RESIDENT_TARGETS: no art_targets_sync yet");
  eff = *d;
  eff.audio_target_positions = c->targets.snap.data();
  eff.audio_target_count = c->targets.synced;  // (0: validate_desc refuses a frame without targets)
  if (c->targets.synced == 0) eff.audio_target_positions = nullptr;
  d = &eff;
  return ART_OK;
}

bool fan_wants_hits(const art_fan* fans, int n) {
  for (int i = 0; i < n; ++i)
    if (fans[i].ray_hit_points || fans[i].ray_hit_counts || fans[i].ray_hit_ids) return true;
  return false;
}

// JobHandle.Complete (AudioRayTracer.cs:97): the frame's completion event, polled for up to 4 ms
// (a frame takes ~0.1-2 ms: polling wakes the caller within a microsecond or two of the event,
// where a blocking wait adds the runtime's wake-up latency), then waited for. ART_COMPLETE_SPIN=0
// in the environment: always the blocking wait.
hipError_t wait_done(hipEvent_t ev) {
  static const bool spin = [] { const char* e = getenv("ART_COMPLETE_SPIN"); return !(e && e[0] == '0'); }();
  if (spin) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipEventQuery(ev);
      if (e != hipErrorNotReady) return e;
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(4)) break;
    }
  }
  return hipEventSynchronize(ev);
}

// phase names of art_ctx::HostPhases (in the order the frame runs them)
const char* const kHostPhase[8] = {"validate_frame", "pack_inputs", "stage_fans", "upload_scene", "enqueue_copies_kernels",
                                   "complete_wait", "unpack_outputs", "complete_other"};

}  // namespace

int art::fail(art_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
  }
  return code;
}

// ============================================================================================
// C ABI
// ============================================================================================
extern "C" {

ART_API uint32_t art_version(void) { return kAbiVersion; }

ART_API int art_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Diagnostics: ART_SEGV_TRACE=1 prints the native stack of a fatal signal (glibc backtrace).
static void segv_trace(int sig) {
  void* frames[64];
  const int n = backtrace(frames, 64);
  fprintf(stderr, "libart: fatal signal %d, native stack:\n", sig);
  backtrace_symbols_fd(frames, n, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}

static int create_on(const int32_t* ids, int32_t count, art_ctx** out) {
  if (const char* e = getenv("ART_SEGV_TRACE"))
    if (e[0] == '1') { signal(SIGSEGV, segv_trace); signal(SIGABRT, segv_trace); }
  if (!out) return ART_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ART_E_DEVICE;
  if (count <= 0 || count > 64 || !ids) return ART_E_INVALID;
  art_ctx* c = new (std::nothrow) art_ctx();
  if (!c) return ART_E_NOMEM;
  if (const char* e = getenv("ART_HOST_TIMES")) c->hp.on = e[0] == '1';
  for (int32_t k = 0; k < count; ++k) {
    const int i = ids[k];
    Device dv;
    dv.id = i;
    if (i < 0 || i >= n || hipSetDevice(i) != hipSuccess || hipStreamCreateWithFlags(&dv.stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&dv.done, hipEventDisableTiming) != hipSuccess) {
      if (dv.stream) (void)hipStreamDestroy(dv.stream);
      art_destroy(c);  // the devices created so far; the failed entry holds nothing
      return ART_E_DEVICE;
    }
    c->devs.push_back(dv);
  }
  *out = c;
  return ART_OK;
}

ART_API int art_create(uint32_t device_mask, art_ctx** out) {
  if (!out) return ART_E_INVALID;
  *out = nullptr;
  if (device_mask == 0) {  // the CPU backend: worker threads, no HIP device needed
    art_ctx* c = new (std::nothrow) art_ctx();
    if (!c) return ART_E_NOMEM;
    c->cpu = art::cpu_create(0);
    if (!c->cpu) { delete c; return ART_E_NOMEM; }
    *out = c;
    return ART_OK;
  }
  int32_t ids[32];
  int32_t k = 0;
  for (int i = 0; i < 32; ++i)
    if (device_mask & (1u << i)) ids[k++] = i;
  return create_on(ids, k, out);
}

ART_API int art_create_on(const int32_t* device_ids, int32_t count, art_ctx** out) {
  return create_on(device_ids, count, out);
}

#ifdef ART_DIAG
void art_diag_dump_impl();
#endif
#ifdef ART_WAVE_TIMES
extern "C" void art_wave_times_dump_impl();
#endif
ART_API void art_destroy(art_ctx* c) {
#ifdef ART_DIAG
  if (c && !c->devs.empty()) art_diag_dump_impl();
#endif
#ifdef ART_WAVE_TIMES
  if (c && !c->devs.empty()) art_wave_times_dump_impl();
#endif
  if (!c) return;
  if (c->hp.on && c->hp.frames) {
    fprintf(stderr, "{\"art_host_phases_us\": {");
    for (int k = 0; k < 8; ++k) fprintf(stderr, "%s\"%s\": %.3f", k ? ", " : "", kHostPhase[k], c->hp.us[k] / (double)c->hp.frames);
    fprintf(stderr, "}, \"frames\": %llu}\n", (unsigned long long)c->hp.frames);
  }
  if (c->cpu) {
    if (c->inflight) art::cpu_complete(c->cpu, nullptr);
    art::cpu_destroy(c->cpu);
  }
  for (Device& dv : c->devs) {
    (void)hipSetDevice(dv.id);
    if (dv.stream) (void)hipStreamSynchronize(dv.stream);
    if (dv.fence.pending) {  // a device frame on the caller's stream: wait for it alone (the stream is valid
                              // until this call, art_device.h); the device-wide wait only if that fails
      if (dv.fence.mark_done(c) != ART_OK || hipEventSynchronize(dv.fence.done) != hipSuccess) (void)hipDeviceSynchronize();
      dv.fence.pending = false;
    }
    dv.raw.release(); dv.soa.release(); dv.origins.release(); dv.block.release(); dv.acc.release(); dv.counts.release();
    dv.exec.release(); dv.pairs.release(); dv.dsp.release(); dv.tick_curves.release(); dv.cones.release(); dv.tsel.release();
    dv.cell_status.release();
    dv.relabel_status.release();
    dv.store.raw.release(); dv.store.soa.release(); dv.store.upd.release();
    if (dv.store.done) (void)hipEventDestroy(dv.store.done);
    for (hipEvent_t e : dv.store.epoch)
      if (e) (void)hipEventDestroy(e);
    if (dv.fence.done) (void)hipEventDestroy(dv.fence.done);
    for (hipEvent_t e : dv.ev_pool) (void)hipEventDestroy(e);
    if (dv.done) (void)hipEventDestroy(dv.done);
    for (SideStream* s : {&dv.side, &dv.echo}) {
      if (s->st) (void)hipStreamSynchronize(s->st);
      if (s->fork) (void)hipEventDestroy(s->fork);
      if (s->join) (void)hipEventDestroy(s->join);
      if (s->st) (void)hipStreamDestroy(s->st);
    }
    if (dv.stream) (void)hipStreamDestroy(dv.stream);
  }
  c->h_in.release();
  c->h_block.release();
  c->h_dsp.release();
  for (HostBuf& b : c->store.h_upd) b.release();
  delete c;
}

ART_API const char* art_last_error(const art_ctx* c) { return c ? c->err.c_str() : "null context"; }

// Timing events a device keeps ready once ART_CTX_TIME_KERNELS is first set: the pool grows on the
// host here, before any timed frame, so a timed frame of up to 5 bounces never creates events
// (hipEventCreate inside a caller's timed loop): 6 stage events + 2 (3H + 2) per-kernel events
// (ART_CTX_TIME_EACH_KERNEL) per frame, 64 frames between art_kernel_timing calls.
constexpr size_t kTimingEventsReserve = 64 * (6 + 2 * (3 * 5 + 2));

ART_API int art_set_flags(art_ctx* c, uint32_t flags) {
  if (!c) return ART_E_INVALID;
  if ((flags & ART_CTX_TIME_KERNELS) && !(c->flags & ART_CTX_TIME_KERNELS) && !c->devs.empty()) {
    int prev = 0;
    (void)hipGetDevice(&prev);
    for (Device& dv : c->devs) {
      (void)hipSetDevice(dv.id);
      (void)pool_event(dv, kTimingEventsReserve - 1);
    }
    (void)hipSetDevice(prev);
  }
  c->flags = flags;
  return ART_OK;
}

ART_API int art_fan_layout_get(const art_frame_desc* d, uint32_t out_flags, art_fan_layout* out) {
  if (!out) return ART_E_INVALID;
  int rc = validate_desc(nullptr, d);
  if (rc) return rc;
  FanLayout L = make_layout(d, out_flags);
  out->stride = L.stride; out->settings_off = L.settings_off; out->dsp_off = L.dsp_off; out->muffle_off = L.muffle_off;
  out->perm_off = L.perm_off; out->echo_off = L.echo_off; out->hit_points_off = L.hit_points_off;
  out->hit_counts_off = L.hit_counts_off;
  out->hit_ids_off = L.hit_ids_off;
  return ART_OK;
}

ART_API int art_schedule(art_ctx* c, const art_frame_desc* d, const art_fan* fans, int32_t fan_count, art_handle* out) {
  if (!c) return ART_E_INVALID;
  if (!out) return fail(c, ART_E_INVALID, "handle pointer is NULL");
  if (c->inflight) return fail(c, ART_E_STATE, "a frame is in flight: call art_complete first (AudioRayTracer.cs:97)");
  art_frame_desc eff;
  int rc = resident_targets_desc(c, d, eff);
  if (rc) return rc;
  rc = validate_desc(c, d);
  if (rc) return rc;
  if (fan_count < 0 || (fan_count > 0 && !fans)) return fail(c, ART_E_INVALID, "bad fans array");
  rc = check_resident(c, d);
  if (rc) return rc;
  const bool hits = fan_wants_hits(fans, fan_count);
  for (int i = 0; i < fan_count; ++i) {
    const art_fan& f = fans[i];
    if (!f.echo_ray_distances || !f.muffle_ray_hits || !f.permeation_power_remains || !f.settings)
      return fail(c, ART_E_INVALID, "fan %d: echo/muffle/permeation/settings arrays are required", i);
  }
  if (c->cpu) {
    art::CpuColliders rc_{};
    const bool res = (c->flags & ART_CTX_RESIDENT_COLLIDERS) != 0;
    if (res) {
      rc_.sph = reinterpret_cast<const art_sphere*>(c->store.cpu_recs[0].data()); rc_.ns = c->store.synced[0];
      rc_.aabb = reinterpret_cast<const art_aabb*>(c->store.cpu_recs[1].data()); rc_.na = c->store.synced[1];
      rc_.obb = reinterpret_cast<const art_obb*>(c->store.cpu_recs[2].data()); rc_.no = c->store.synced[2];
    }
    const bool count = (c->flags & ART_CTX_COUNT_TESTS) != 0;
    rc = art::cpu_schedule(c->cpu, d, fans, fan_count, res ? &rc_ : nullptr, count);
    if (rc) return fail(c, rc, "CPU backend: schedule failed");
    c->counted = count;
    c->inflight = true;
    c->handle = c->next_handle++;
    *out = c->handle;
    return ART_OK;
  }
  PhaseClock pc(&c->hp);
  Frame& f = c->fr;
  make_frame(d, hits ? ART_OUT_HIT_RESULTS : 0u, f, (c->flags & ART_CTX_RESIDENT_COLLIDERS) ? c->store.synced : nullptr,
             (c->flags & ART_CTX_RESIDENT_TARGETS) != 0, c->targets.reserved, c->store.reserved);
  const FanLayout& L = f.L;
  const size_t origins_off = align_up(f.raw_bytes, 16);
  if (!c->h_block.reserve((size_t)fan_count * L.stride)) return fail(c, ART_E_NOMEM, "pinned allocation failed");
  // shard fans over devices
  const int nd = (int)c->devs.size();
  for (int k = 0; k < nd; ++k) {
    Device& dv = c->devs[k];
    dv.fan_begin = (int)((long long)fan_count * k / nd);
    dv.fan_count = (int)((long long)fan_count * (k + 1) / nd) - dv.fan_begin;
  }
  // In/out arrays (the reference's persistent NativeArrays): slots no batch resets keep their
  // contents, so their current values travel to the device with the frame. Compact frames (one
  // batch slot, raytrace stage, no echo upload or hit outputs: every muffle slot is reset) upload
  // no slots, except the permeation slots when the permeation stage does not rewrite them, and
  // those beside the origins (one H2D copy per shard: [origins | permeation slots]).
  const size_t RH = (size_t)f.R * f.H;
  const bool need_echo = f.TC > 1 || !(f.stages & ART_STAGE_RAYTRACE);
  const bool compact = compact_slots(f, need_echo);
  const bool perm_in = compact && !(f.stages & ART_STAGE_PERMEATE);
  const size_t tcT = (size_t)f.TC * f.T;
  size_t in_end = origins_off;
  for (Device& dv : c->devs) {
    dv.in_off = in_end;
    in_end += align_up(align_up((size_t)dv.fan_count * 12, 16) + (perm_in ? (size_t)dv.fan_count * tcT * 4 : 0), 16);
  }
  if (!c->h_in.reserve(in_end)) return fail(c, ART_E_NOMEM, "pinned allocation failed");
  uint8_t* hin = static_cast<uint8_t*>(c->h_in.p);
  uint8_t* hb = static_cast<uint8_t*>(c->h_block.p);
  pc.mark(0);
  pack_inputs(d, f, hin);
  pc.mark(1);
  for (int i = 0, k = 0; i < fan_count; ++i) {
    const art_fan& fn = fans[i];
    while (i >= c->devs[k].fan_begin + c->devs[k].fan_count) ++k;
    const Device& dv = c->devs[k];
    uint8_t* seg = hin + dv.in_off;
    const size_t j = (size_t)(i - dv.fan_begin);
    memcpy(seg + 12 * j, fn.origin, 12);
    if (perm_in) memcpy(seg + align_up((size_t)dv.fan_count * 12, 16) + j * tcT * 4, fn.permeation_power_remains, tcT * 4);
    uint8_t* rec = hb + (size_t)i * L.stride;
    if (!compact) {
      memcpy(rec + L.muffle_off, fn.muffle_ray_hits, tcT * 2);
      memcpy(rec + L.perm_off, fn.permeation_power_remains, tcT * 4);
    }
    if (need_echo) {
      memcpy(rec + L.echo_off, fn.echo_ray_distances, RH * 2);
      if (L.has_hits) {
        if (fn.ray_hit_points) memcpy(rec + L.hit_points_off, fn.ray_hit_points, RH * sizeof(art_half3));
        else memset(rec + L.hit_points_off, 0, RH * sizeof(art_half3));
        if (fn.ray_hit_ids) memcpy(rec + L.hit_ids_off, fn.ray_hit_ids, RH * sizeof(uint32_t));
        else memset(rec + L.hit_ids_off, 0xFF, RH * sizeof(uint32_t));
      }
    }
    if (L.has_hits) {
      if (fn.ray_hit_counts) memcpy(rec + L.hit_counts_off, fn.ray_hit_counts, (size_t)f.R);
      else memset(rec + L.hit_counts_off, 0, (size_t)f.R);
    }
  }
  const bool count = (c->flags & ART_CTX_COUNT_TESTS) != 0;
  if (count) count_nonowned(c, d);
  pc.mark(2);
  // Enqueue per device. An error on device k leaves devices [0, k) (and k itself, partly) with
  // async copies that still read or write the pinned staging: drain every stream before returning,
  // so the next art_schedule can repack h_in / h_block safely.
  // test hook (tests/test_multigpu_gpu.py): shard k's enqueue fails after its scene upload
  const char* fail_env = getenv("ART_TEST_FAIL_SHARD");
  const int fail_shard = fail_env ? atoi(fail_env) : -1;
  for (size_t k = 0; k < c->devs.size(); ++k) {
    Device& dv = c->devs[k];
    rc = enqueue_device_frame(c, dv, f, hin, hb, need_echo, count, (int)k == fail_shard, &pc);
    if (rc) {
      for (Device& e : c->devs) {
        (void)hipSetDevice(e.id);
        (void)hipStreamSynchronize(e.stream);
        if (e.side.st) (void)hipStreamSynchronize(e.side.st);  // a forked stage may not have joined
        if (e.echo.st) (void)hipStreamSynchronize(e.echo.st);
      }
      return rc;
    }
  }
  c->fans.assign(fans, fans + fan_count);
  c->counted = count;
  c->inflight = true;
  c->handle = c->next_handle++;
  *out = c->handle;
  return ART_OK;
}

ART_API int art_is_completed(art_ctx* c, art_handle h) {
  if (!c) return ART_E_INVALID;
  if (!c->inflight || h != c->handle) return (h != 0 && h < c->next_handle) ? 1 : fail(c, ART_E_STATE, "unknown handle");
  if (c->cpu) return art::cpu_is_completed(c->cpu) ? 1 : 0;
  for (Device& dv : c->devs) {
    (void)hipSetDevice(dv.id);
    hipError_t e = hipEventQuery(dv.done);
    if (e == hipErrorNotReady) return 0;
    if (e != hipSuccess) return fail(c, ART_E_DEVICE, "hipEventQuery: %s", hipGetErrorString(e));
  }
  return 1;
}

ART_API int art_complete(art_ctx* c, art_handle h) {
  if (!c) return ART_E_INVALID;
  if (!c->inflight || h != c->handle) {
    if (h != 0 && h < c->next_handle) return ART_OK;  // already completed (JobHandle.Complete is idempotent)
    return fail(c, ART_E_STATE, "unknown handle");
  }
  c->inflight = false;
  if (c->cpu) {
    art::cpu_complete(c->cpu, c->counted ? &c->last_counts : nullptr);
    if (c->counted) c->has_counts = true;
    return ART_OK;
  }
  PhaseClock pc(&c->hp);
  for (Device& dv : c->devs) {
    HIP_TRY(c, hipSetDevice(dv.id));
    HIP_TRY(c, wait_done(dv.done));
  }
  pc.mark(5);
  const Frame& f = c->fr;
  const FanLayout& L = f.L;
  const size_t RH = (size_t)f.R * f.H;
  const uint8_t* hb = static_cast<const uint8_t*>(c->h_block.p);
  // compact frames without the permeation stage leave the caller's permeation slots as they are
  const bool perm_back = !(compact_slots(f, f.TC > 1 || !(f.stages & ART_STAGE_RAYTRACE)) && !(f.stages & ART_STAGE_PERMEATE));
  for (size_t i = 0; i < c->fans.size(); ++i) {
    const art_fan& fn = c->fans[i];
    const uint8_t* rec = hb + i * L.stride;
    if (f.stages & ART_STAGE_REDUCE)  // otherwise AudioTargetSettings keep the caller's contents
      memcpy(fn.settings, rec + L.settings_off, (size_t)f.T * sizeof(art_target_settings));
    if (L.has_dsp && fn.dsp_params) memcpy(fn.dsp_params, rec + L.dsp_off, (size_t)f.T * sizeof(art_dsp_params));
    memcpy(fn.muffle_ray_hits, rec + L.muffle_off, (size_t)f.TC * f.T * 2);
    if (perm_back) memcpy(fn.permeation_power_remains, rec + L.perm_off, (size_t)f.TC * f.T * 4);
    memcpy(fn.echo_ray_distances, rec + L.echo_off, RH * 2);
    if (L.has_hits && fn.ray_hit_points) memcpy(fn.ray_hit_points, rec + L.hit_points_off, RH * sizeof(art_half3));
    if (L.has_hits && fn.ray_hit_counts) memcpy(fn.ray_hit_counts, rec + L.hit_counts_off, (size_t)f.R);
    if (L.has_hits && fn.ray_hit_ids) memcpy(fn.ray_hit_ids, rec + L.hit_ids_off, RH * sizeof(uint32_t));
  }
  pc.mark(6);
  if (c->counted) {
    memset(&c->last_counts, 0, sizeof c->last_counts);
    for (Device& dv : c->devs) {
      if (dv.fan_count == 0) continue;
      HIP_TRY(c, hipSetDevice(dv.id));
      int rc = read_counts(c, dv, dv.stream, &c->last_counts, true);
      if (rc) return rc;
    }
    c->has_counts = true;
  }
  pc.mark(7);
  if (c->hp.on) c->hp.frames++;
  return ART_OK;
}

ART_API int art_last_test_counts(art_ctx* c, art_test_counts* out) {
  if (!c || !out) return ART_E_INVALID;
  if (!c->has_counts) return fail(c, ART_E_STATE, "no counted frame yet (set ART_CTX_COUNT_TESTS)");
  *out = c->last_counts;
  return ART_OK;
}

// ---------------------------------------------------------------------------- device-resident
ART_API int art_scene_bind(art_ctx* c, const art_frame_desc* d) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  // the in-flight frame's art_complete reads c->fr and its H2D copy may still read c->h_in
  if (c->inflight) return fail(c, ART_E_STATE, "art_scene_bind: a frame is in flight (bind after art_complete)");
  art_frame_desc eff;
  int rc = resident_targets_desc(c, d, eff);
  if (rc) return rc;
  rc = validate_desc(c, d);
  if (rc) return rc;
  rc = check_resident(c, d);
  if (rc) return rc;
  Frame& f = c->fr;
  make_frame(d, 0u, f, (c->flags & ART_CTX_RESIDENT_COLLIDERS) ? c->store.synced : nullptr,
             (c->flags & ART_CTX_RESIDENT_TARGETS) != 0, c->targets.reserved, c->store.reserved);
  if (!c->h_in.reserve(f.raw_bytes)) return fail(c, ART_E_NOMEM, "pinned allocation failed");
  pack_inputs(d, f, static_cast<uint8_t*>(c->h_in.p));
  count_nonowned(c, d);
  // which target indices own colliders (a count-changing target sync asks; the resident store keeps its own)
  for (auto& h : c->bind_tid_hist) h.clear();
  if (f.Tc > 0 && !f.resident) {
    for (auto& h : c->bind_tid_hist) h.assign(65536, 0);
    for (int i = 0; i < d->sphere_count; ++i) c->bind_tid_hist[0][(size_t)(d->sphere_colliders[i].audio_target_id + 32768)]++;
    for (int i = 0; i < d->aabb_count; ++i) c->bind_tid_hist[1][(size_t)(d->aabb_colliders[i].audio_target_id + 32768)]++;
    for (int i = 0; i < d->obb_count; ++i) c->bind_tid_hist[2][(size_t)(d->obb_colliders[i].audio_target_id + 32768)]++;
  }
  for (Device& dv : c->devs) {
    rc = upload_scene(c, dv, f, static_cast<const uint8_t*>(c->h_in.p));
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(dv.stream));
  }
  if (f.Tc > 0) {
    // A later target sync allocates nothing: its build selection, and every slot of the pinned
    // image ring at the largest image Tc targets make ([indices][positions][selection][moves] <=
    // 24 Tc + 64 bytes). Every earlier sync has completed (the streams were just waited for).
    const size_t image = 4 * align_up((size_t)f.Tc * 12, 16) + 64;
    for (HostBuf& b : c->store.h_upd)
      if (!b.reserve(image)) return fail(c, ART_E_NOMEM, "pinned allocation failed");
    for (Device& dv : c->devs) {
      HIP_TRY(c, hipSetDevice(dv.id));
      if (!dv.tsel.reserve((size_t)kMaxTargets * sizeof(int))) return fail(c, ART_E_NOMEM, "device allocation failed");
    }
  }
  if (f.Cc[0] + f.Cc[1] + f.Cc[2] > 0) {
    // A later count-changing collider sync allocates nothing while it uploads at most
    // min(capacity, kSyncRefitMax) records: every slot of the pinned image ring and the devices'
    // copy of it at that image's size ([indices][records] per kind, 16-B aligned sections), and the
    // word the relabel kernel reports through.
    const size_t recs = (size_t)std::min<long long>(f.ccap(), kSyncRefitMax);
    const size_t image = recs * (4 + sizeof(art_obb)) + 6 * 16;
    for (HostBuf& b : c->store.h_upd)
      if (!b.reserve(image)) return fail(c, ART_E_NOMEM, "pinned allocation failed");
    for (Device& dv : c->devs) {
      HIP_TRY(c, hipSetDevice(dv.id));
      if (!dv.store.upd.reserve(image)) return fail(c, ART_E_NOMEM, "device allocation failed");
      if (!dv.relabel_status.p) {
        if (!dv.relabel_status.reserve(sizeof(uint32_t))) return fail(c, ART_E_NOMEM, "pinned allocation failed");
        memset(dv.relabel_status.p, 0, sizeof(uint32_t));
      }
    }
  }
  return ART_OK;
}

static int launch_common(art_ctx* c, const float* d_origins, int32_t fan_count, void* d_block, uint32_t out_flags,
                         void* stream, bool count, art_test_counts* out) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  if (c->inflight) return fail(c, ART_E_STATE, "a frame is in flight (launch after art_complete)");
  if (c->devs.empty() || !c->devs[0].bound) return fail(c, ART_E_STATE, "no scene bound (art_scene_bind)");
  if (fan_count < 0 || (fan_count > 0 && (!d_origins || !d_block))) return fail(c, ART_E_INVALID, "bad device buffers");
  Device& dv = c->devs[0];
  HIP_TRY(c, hipSetDevice(dv.id));
  Frame& f = c->fr;
  // the bound frame's layout is for out_flags = 0; refresh for the requested outputs
  f.L.has_hits = (out_flags & ART_OUT_HIT_RESULTS) ? 1 : 0;
  {
    art_frame_desc tmp{};
    tmp.ray_count = f.R; tmp.max_hits_per_ray = f.H; tmp.audio_target_count = f.T; tmp.batch_slots = f.TC;
    tmp.stages = f.stages;
    f.L = make_layout(&tmp, out_flags);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);  // NULL is the HIP default stream (torch's default)
  int rc = scene_reader_begin(c, dv, f, st);
  if (rc) return rc;
  rc = enqueue_kernels(c, dv, f, d_origins, fan_count, static_cast<uint8_t*>(d_block), st, count);
  if (rc) return rc;
  rc = scene_reader_end(c, dv, st);
  if (rc) return rc;
  if (count) return read_counts(c, dv, st, out, false);
  return ART_OK;
}

ART_API int art_launch_device(art_ctx* c, const float* d_origins, int32_t fan_count, void* d_block, uint32_t out_flags,
                              void* stream) {
  return launch_common(c, d_origins, fan_count, d_block, out_flags, stream, false, nullptr);
}

ART_API int art_count_device(art_ctx* c, const float* d_origins, int32_t fan_count, void* d_block, uint32_t out_flags,
                             void* stream, art_test_counts* out) {
  if (!out) return ART_E_INVALID;
  return launch_common(c, d_origins, fan_count, d_block, out_flags, stream, true, out);
}

ART_API int art_fibonacci_directions_device(art_ctx* c, int32_t count, art_half3* d_out, void* stream) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  if (count < 0 || (count > 0 && !d_out)) return fail(c, ART_E_INVALID, "art_fibonacci_directions_device: bad arguments");
  if (count == 0) return ART_OK;
  HIP_TRY(c, hipSetDevice(c->devs[0].id));
  launch_fibonacci(count, d_out, static_cast<hipStream_t>(stream));
  HIP_TRY(c, hipGetLastError());
  return ART_OK;
}

ART_API int art_f32tof16_device(art_ctx* c, uint32_t first_bits, uint32_t count, uint16_t* d_out, void* stream) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  if (count > 0 && !d_out) return fail(c, ART_E_INVALID, "art_f32tof16_device: d_out is NULL");
  HIP_TRY(c, hipSetDevice(c->devs[0].id));
  launch_half_range(first_bits, count, d_out, static_cast<hipStream_t>(stream));
  HIP_TRY(c, hipGetLastError());
  return ART_OK;
}

ART_API int art_recip_exact_device(art_ctx* c, uint32_t first_bits, uint32_t count, uint32_t* d_out, void* stream) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  if (count > 0 && !d_out) return fail(c, ART_E_INVALID, "art_recip_exact_device: d_out is NULL");
  HIP_TRY(c, hipSetDevice(c->devs[0].id));
  launch_recip_range(first_bits, count, d_out, static_cast<hipStream_t>(stream));
  HIP_TRY(c, hipGetLastError());
  return ART_OK;
}

ART_API int art_executed_counts(art_ctx* c, art_exec_counts* out) {
  if (!c || !out) return ART_E_INVALID;
  memset(out, 0, sizeof *out);
  for (Device& dv : c->devs) {
    if (!dv.exec.p) continue;
    HIP_TRY(c, hipSetDevice(dv.id));
    HIP_TRY(c, hipDeviceSynchronize());
    unsigned long long v[kExecSlots] = {};
    HIP_TRY(c, hipMemcpy(v, dv.exec.p, sizeof v, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemset(dv.exec.p, 0, sizeof v));
    for (int k = 0; k < 3; ++k) {  // per kernel family (kExecNearest, kExecEcho, kExecMuffle), then the totals
      const unsigned long long* g = v + kExecNearest + k * kExecGroup;
      out->by_kernel[k].sphere += g[kExecSphere]; out->by_kernel[k].aabb += g[kExecAabb]; out->by_kernel[k].obb += g[kExecObb];
      out->by_kernel[k].cull_box += g[kExecCullBox]; out->by_kernel[k].cell_entries += g[kExecCellEntries];
      out->sphere += g[kExecSphere]; out->aabb += g[kExecAabb]; out->obb += g[kExecObb]; out->cull_box += g[kExecCullBox];
      out->cell_entries += g[kExecCellEntries]; out->muffle_fallback += g[kExecMuffleFallback];
    }
    out->echo_pairs += v[kExecEchoPairs];
    for (int k = 0; k < kExecBounces; ++k) out->bounce_rays[k] += v[kExecBounce0 + k];
    out->launches += dv.exec_launches;
    dv.exec_launches = 0;
  }
  return ART_OK;
}

ART_API int art_debug_leaf_order(art_ctx* c, uint32_t* out, int32_t cap) {
  if (!c || (!out && cap > 0) || cap < 0) return ART_E_INVALID;
  if (c->devs.empty() || !c->devs[0].bound) return ART_E_STATE;
  Device& dv = c->devs[0];
  const int n = dv.sc.ns + dv.sc.na + dv.sc.no;
  if (!dv.sc.bvh_ref || n <= 0) return 0;
  const int m = n < cap ? n : cap;
  HIP_TRY(c, hipSetDevice(dv.id));
  HIP_TRY(c, hipDeviceSynchronize());
  if (m > 0) HIP_TRY(c, hipMemcpy(out, dv.sc.bvh_ref, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return m;
}

ART_API int art_debug_bvh_records(art_ctx* c, int32_t which, float* out, int32_t cap) {
  static_assert(sizeof(CullRec) == 8 * sizeof(float), "CullRec: 8 floats");
  if (!c || (!out && cap > 0) || cap < 0 || (which != ART_DEBUG_BVH_BOUNDS && which != ART_DEBUG_BVH_NODES)) return ART_E_INVALID;
  if (c->devs.empty() || !c->devs[0].bound) return ART_E_STATE;
  Device& dv = c->devs[0];
  const int n = dv.sc.ns + dv.sc.na + dv.sc.no;
  if (!dv.sc.bvh || !dv.sc.cull || n <= 0) return 0;
  const CullRec* src = which == ART_DEBUG_BVH_BOUNDS ? dv.sc.cull : dv.sc.bvh;
  const int count = which == ART_DEBUG_BVH_BOUNDS ? n : (int)bvh_node_count(n);
  const int m = count < cap ? count : cap;
  HIP_TRY(c, hipSetDevice(dv.id));
  HIP_TRY(c, hipDeviceSynchronize());
  if (m > 0) HIP_TRY(c, hipMemcpy(out, src, (size_t)m * sizeof(CullRec), hipMemcpyDeviceToHost));
  return count;
}

ART_API int art_debug_last_plan(art_ctx* c, uint32_t* bits) {
  if (!c || !bits) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  *bits = c->devs.empty() ? 0u : c->devs[0].last_plan;
  return ART_OK;
}

ART_API int art_debug_echo_decided(art_ctx* c, uint64_t* replayed, uint64_t* traversed) {
  if (!c || !replayed || !traversed) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  *replayed = *traversed = 0;
  for (Device& dv : c->devs) {
    if (!dv.echo_decided) continue;
    unsigned long long v[kEchoCountSlots];
    HIP_TRY(c, hipSetDevice(dv.id));
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(v, dv.echo_decided, sizeof v, hipMemcpyDeviceToHost));
    for (unsigned long long x : v) {
      *replayed += x & 0xffffffffull;
      *traversed += x >> 32;
    }
  }
  return ART_OK;
}

ART_API int art_debug_sphere_slack(art_ctx* c, float r, float D, float* slack, float* scene_r_min) {
  if (!slack || (scene_r_min && !c)) return ART_E_INVALID;
  *slack = art::sphere_report_slack(r, D);
  if (!scene_r_min) return ART_OK;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) keeps no device scene", __func__);
  if (c->devs.empty() || !c->devs[0].bound) return fail(c, ART_E_STATE, "no scene bound (art_scene_bind)");
  *scene_r_min = c->devs[0].sc.r_min;
  return ART_OK;
}

ART_API int art_debug_node_margin_cap(art_ctx* c, float r_min, float s_root, float om, int32_t has_obb, float reach, float* cap,
                                      float* scene_s_root) {
  if (!cap || (scene_s_root && !c)) return ART_E_INVALID;
  *cap = art::node_margin_cap(r_min, s_root, om, has_obb != 0, reach);
  if (!scene_s_root) return ART_OK;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) keeps no device scene", __func__);
  if (c->devs.empty() || !c->devs[0].bound) return fail(c, ART_E_STATE, "no scene bound (art_scene_bind)");
  Device& dv = c->devs[0];
  *scene_s_root = 0.0f;
  if (!dv.sc.bvh || dv.sc.ns + dv.sc.na + dv.sc.no <= 0) return ART_OK;
  CullRec root;
  HIP_TRY(c, hipSetDevice(dv.id));
  HIP_TRY(c, hipDeviceSynchronize());
  HIP_TRY(c, hipMemcpy(&root, dv.sc.bvh, sizeof root, hipMemcpyDeviceToHost));
  *scene_s_root = art::node_abs_sum(root.lox, root.loy, root.loz, root.hix, root.hiy, root.hiz);
  return ART_OK;
}

ART_API int art_debug_cells_arena(art_ctx* c, uint64_t* used, uint64_t* cap, uint32_t* dropped_targets) {
  if (!c || !used || !cap || !dropped_targets) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  if (c->devs.empty() || !c->devs[0].bound) return fail(c, ART_E_STATE, "no scene bound (art_scene_bind)");
  Device& dv = c->devs[0];
  HIP_TRY(c, hipSetDevice(dv.id));
  HIP_TRY(c, hipDeviceSynchronize());
  uint32_t v[2] = {0u, 0u};
  if (dv.cb.tail) HIP_TRY(c, hipMemcpy(v, dv.cb.tail, sizeof v, hipMemcpyDeviceToHost));
  *used = v[0];
  *cap = dv.cb.cap;
  *dropped_targets = v[1];
  return ART_OK;
}

ART_API int art_debug_cells_lists(art_ctx* c, int32_t which, uint32_t* out, int32_t cap) {
  if (!c || (!out && cap > 0) || cap < 0 || which < ART_DEBUG_CELLS_STARTS || which > ART_DEBUG_CELLS_INFO) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  if (c->devs.empty() || !c->devs[0].bound) return fail(c, ART_E_STATE, "no scene bound (art_scene_bind)");
  Device& dv = c->devs[0];
  const CellBufs& cb = dv.cb;
  const size_t T = (size_t)std::max(dv.sc.T, 0);
  HIP_TRY(c, hipSetDevice(dv.id));
  HIP_TRY(c, hipDeviceSynchronize());
  uint32_t tail[2] = {0u, 0u};
  if (cb.tail) HIP_TRY(c, hipMemcpy(tail, cb.tail, sizeof tail, hipMemcpyDeviceToHost));
  const uint32_t info[6] = {cb.compact, cb.cap, tail[0], tail[1], (uint32_t)kCellG, (uint32_t)kCellStride};
  const void* src = nullptr;
  size_t count = 0;  // 4-byte words
  switch (which) {
    case ART_DEBUG_CELLS_STARTS: src = cb.start; count = cb.cap ? T * kCellStride + 1 : 0; break;
    case ART_DEBUG_CELLS_ENTRIES: src = cb.ent_s; count = (size_t)std::min(tail[0], cb.cap) * (cb.compact ? 1 : 2); break;
    case ART_DEBUG_CELLS_OK: src = cb.ok; count = T; break;
    case ART_DEBUG_CELLS_FAR: src = cb.far; count = cb.cap ? T : 0; break;  // (not written without lists)
    default: break;
  }
  if (which == ART_DEBUG_CELLS_INFO) {
    count = 6;
    if (cap > 0) memcpy(out, info, std::min<size_t>(count, (size_t)cap) * sizeof(uint32_t));
    return (int)count;
  }
  if (count > (size_t)INT32_MAX) return fail(c, ART_E_UNSUPPORTED, "%s: more than 2^31 - 1 words", __func__);
  const size_t m = std::min(count, (size_t)cap);
  if (m > 0 && src) HIP_TRY(c, hipMemcpy(out, src, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return (int)count;
}

ART_API int art_kernel_timing(art_ctx* c, art_kernel_times* out) {
  if (!c || !out) return ART_E_INVALID;
  memset(out, 0, sizeof *out);
  for (Device& dv : c->devs) {
    HIP_TRY(c, hipSetDevice(dv.id));
    int frames = 0;
    for (auto& u : dv.ev_used) {
      hipEvent_t a = dv.ev_pool[u.second], b = dv.ev_pool[u.second + 1];
      HIP_TRY(c, hipEventSynchronize(b));
      float ms = 0.0f;
      HIP_TRY(c, hipEventElapsedTime(&ms, a, b));
      if (u.first == kEvRaytrace) { out->raytrace_ms += ms; frames++; }
      else if (u.first == kEvPermeate) out->permeate_ms += ms;
      else if (u.first == kEvReduce) out->reduce_ms += ms;
      else if (u.first - kEvKernel0 < kMarkKinds) {
        out->kernel_ms[u.first - kEvKernel0] += ms;
        out->kernel_launches[u.first - kEvKernel0]++;
      }
    }
    dv.ev_used.clear();
    out->launches += frames;
    out->kernel_marks_dropped += dv.marks_dropped;
    dv.marks_dropped = 0;
  }
  return ART_OK;
}

}  // extern "C"
