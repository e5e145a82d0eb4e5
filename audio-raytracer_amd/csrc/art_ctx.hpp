// art_ctx.hpp — the context behind the C ABI (internal to libart.so): per-device and per-context
// state grouped by owner, and the functions that cross the host units art_capi.cpp, art_frame.cpp,
// art_scene.cpp, art_enqueue.cpp, art_store.cpp and art_dsp_api.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/art_colliders.h"
#include "../../include/art_device.h"
#include "art_cpu.hpp"
#include "art_internal.hpp"

struct art_ctx;

namespace art {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// per collider kind (sphere, AABB, OBB): record size and offset of its audio_target_id
constexpr size_t kRecSize[3] = {sizeof(art_sphere), sizeof(art_aabb), sizeof(art_obb)};
constexpr size_t kTidOff[3] = {offsetof(art_sphere, audio_target_id), offsetof(art_aabb, audio_target_id),
                               offsetof(art_obb, audio_target_id)};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool reserve(size_t n) {
    if (n <= cap) return true;
    release();
    if (hipMalloc(&p, std::max<size_t>(n, 256)) != hipSuccess) { p = nullptr; return false; }
    cap = std::max<size_t>(n, 256);
    return true;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  bool reserve(size_t n) {
    if (n <= cap) return true;
    release();
    if (hipHostMalloc(&p, std::max<size_t>(n, 256), hipHostMallocDefault) != hipSuccess) { p = nullptr; return false; }
    cap = std::max<size_t>(n, 256);
    return true;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// Hands out the 256-B aligned sections of one device allocation in order (base 0: only their sizes).
struct Carver {
  uintptr_t base;
  size_t off = 0;
  template <class T>
  T* take(size_t bytes) {
    T* p = reinterpret_cast<T*>(base + off);
    off = align_up(off + bytes, 256);
    return p;
  }
};

// Scalars of one frame that the kernels need, plus the derived batch tables.
struct Frame {
  int R = 0, H = 0, T = 0, TC = 0, bs = 0, nb = 0;
  // Target capacity of a resident-target scene bound after art_targets_reserve (>= T): every
  // T-sized device section is sized by it, and a target sync whose count stays in [1, Tc] keeps the
  // scene bound. 0: nothing reserved (sections sized by T, a count change unbinds).
  int Tc = 0;
  int tcap() const { return Tc > 0 ? Tc : T; }
  int ns = 0, na = 0, no = 0;
  // Collider capacity per kind of a resident scene bound after art_colliders_reserve (each >= the
  // kind's count): everything carve_sort and carve_cells size by collider count is sized by their
  // sum, and a collider sync whose counts stay within them keeps the scene bound. All 0: nothing
  // reserved (sized by the counts, a count change unbinds).
  int Cc[3] = {0, 0, 0};
  int ccap() const { return Cc[0] + Cc[1] + Cc[2] > 0 ? Cc[0] + Cc[1] + Cc[2] : ns + na + no; }
  uint32_t stages = 0;
  bool resident = false;               // colliders come from the resident store (art_colliders.h)
  bool res_targets = false;            // target positions and T come from the last art_targets_sync
  FrameParams fp{};
  FanLayout L{};
  std::vector<int2> slot_batch;        // permeation: [TC] ray range of the last batch writing slot s
  std::vector<uint8_t> muffle_reset;   // raytrace: [TC] 1 if some batch resets slot s
  std::vector<int> ray_order;          // lane slot -> ray index (direction-coherent at TC == 1)
  std::vector<uint8_t> order_dirs;     // the half3 directions ray_order was computed from
  // input staging layout (bytes)
  size_t off_sph = 0, off_aabb = 0, off_obb = 0, off_tgt = 0, off_dirs = 0, off_vol = 0, off_muf = 0, off_tab = 0,
         off_reset = 0, off_order = 0, raw_bytes = 0;
  // bytes of the record allocation (carve_decoded, carve_sort, carve_cells), entry capacity of the cell lists
  size_t soa_bytes = 0;
  uint32_t cells_cap = 0;
};

// One device's part of the resident collider store (art_colliders.h): AoS lists, decoded records +
// bounds, sync upload.
struct StoreDev {
  DevBuf raw, soa, upd;
  int cap[3] = {0, 0, 0};
  DecodedColliders dec{};       // the store's decoded records, with the counts of the last sync
  int n[3] = {0, 0, 0};
  bool fresh = true;            // capacity (re)allocated: every record must be uploaded
  hipEvent_t done = nullptr;    // recorded after the last sync's upload + decode (on stream)
  hipStream_t stream = nullptr; // the stream the last sync ran on (dv.stream or a device-path launch stream)
  hipEvent_t epoch[2] = {nullptr, nullptr};  // after the last sync of an epoch of the update ring
  bool epoch_pending[2] = {false, false};
};

// An art_launch_device frame still running on the caller's stream reads the scene (records, sorted
// copies, BVH) and uses the context's shared buffers (accumulators, pairs, side streams): work on
// dv.stream that rewrites or reuses them waits for it first.
// The completion event of those frames is recorded only when something has to wait for them: an
// event record between frames costs the launch stream ~5 us of GPU idle per frame (kernel trace,
// DESIGN.md §4), so back-to-back frames on one stream record none. The caller's stream of the last
// frame must still exist at the next call that touches the scene (art.h, streams).
// With ART_CTX_EVENT_EACH_LAUNCH the event is recorded by art_launch_device itself (recorded), so
// the caller may destroy or recycle its stream right after the call.
struct LaunchFence {
  hipEvent_t done = nullptr;     // after the last art_launch_device frame (caller's stream)
  bool pending = false;          // work on dv.stream waits for it before reusing the scene / buffers
  hipStream_t stream = nullptr;  // the caller's stream of that frame
  bool recorded = false;         // done already recorded after that frame
  int mark_done(art_ctx* c);                // record done on the frame's stream (once per frame)
  int wait(art_ctx* c, hipStream_t waiter); // a pending frame: waiter waits for it, nothing is pending then
};

// Host-API frames: the inputs of the last full upload (bytes, layout key, buffers) and the scene
// built from them; a frame whose packed inputs are byte-identical skips the H2D copy, the record
// decode and the BVH build (the Unity caller passes unchanged collider arrays every frame).
struct UploadCache {
  std::vector<uint8_t> raw;
  int key[10] = {};
  const void* raw_p = nullptr;
  const void* soa_p = nullptr;
  bool valid = false;
  DevScene sc{};
};

// Resident scenes: the sorted copies / BVH in dv.soa were built for store generation gen (~0: none)
// with these counts; later frames reuse them (refit when the store changed).
struct SortedCache {
  uint64_t gen = ~0ull;
  const void* soa = nullptr;
  int n[3] = {-1, -1, -1};
  int ccap = -1;  // the collider capacity the sorted copies' buffers were carved for (Frame::ccap)
  DevScene sc{};
  bool matches(const Frame& f, const void* soa_p) const {
    return f.resident && gen != ~0ull && soa == soa_p && n[0] == f.ns && n[1] == f.na && n[2] == f.no && ccap == f.ccap();
  }
};

struct Device {
  int id = 0;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  DevBuf raw, soa, origins, block, acc, counts;
  DevBuf exec;  // executed-work counters (ART_CTX_COUNT_EXECUTED)
  DevBuf cones; // the cell cone table (art_cells.hip), uploaded once
  CellBufs cb{};  // muffle candidate list buffers of the current scene (upload_scene)
  DevBuf tsel;    // the moved targets of the last art_targets_sync (the partial list build's selection)
  HostBuf relabel_status;  // pinned: leaf positions the last bvh_relabel_kernel rewrote (art_collider_resize_stats::relabelled)
  HostBuf cell_status;  // pinned (tail, dropped) of the cell lists' entry arena, written by the device (CellBufs::status)
  bool cells_partial = false;  // a target's lists were rebuilt on their own since the last full build: the arena holds garbage
  DevBuf pairs; // global visibility pairs of the split raytrace path
  DevBuf dsp;   // per-sample DSP batch (art_dsp_process): samples, offsets, frames, params, states
  DevBuf tick_curves;  // the bound spatializer settings (art_dsp_settings_bind*): the class table | each class's baked curves (muffle, reverb volume)
  StoreDev store;
  LaunchFence fence;
  uint64_t exec_launches = 0;
  uint32_t last_plan = 0;  // ART_PLAN_* bits of the last frame's throughput raytrace stage (art_debug_last_plan)
  const unsigned long long* echo_decided = nullptr;  // device: the last frame's echo replay counts (art_debug_echo_decided)
  int fan_begin = 0, fan_count = 0;
  size_t in_off = 0;  // art_schedule: this shard's [origins | permeation slots] in the input staging
  DevScene sc{};
  SortBufs sb{};  // buffers of the spatially sorted scene copy (art_bvh.hip), set by upload_scene
  SortedCache sorted;
  UploadCache last;
  bool bound = false;
  // side stream of the permeation job: it runs beside the raytrace stage (the reference schedules
  // the two jobs independently, AudioRayTracer.cs:191,213), joined before the reduce job (:237);
  // a rebuilt scene's cell lists build there beside the BVH
  SideStream side;
  SideStream echo;  // the echo visibility beside the muffle kernel
  std::vector<hipEvent_t> ev_pool;  // timing events (start/stop pairs)
  std::vector<std::pair<int, size_t>> ev_used;  // (EvKind, pool index of start)
  int marks_dropped = 0;                          // per-kernel marks past the pairs (art_kernel_timing)
};

// The resident collider store of a context: the NextBatch mirror per kind, dirty marks, the last
// sync's counts.
struct ColliderStore {
  struct Kind {
    std::vector<uint8_t> recs;      // count * size bytes
    int count = 0;
    std::vector<uint8_t> dirty;     // per record
    std::vector<int> dirty_list;
  } kinds[3];
  int synced[3] = {0, 0, 0};
  bool store_synced = false;
  // the synced records the resident scene's muffle cell lists were built from (cell_still_valid)
  std::vector<uint8_t> cell_base[3];
  bool cell_base_ok = false;
  uint64_t sync_gen = 0;         // bumped by every art_colliders_sync that changed a record
  // lower bound of |radius| over the synced spheres (DevScene::r_min): exact after a sync that walks
  // every record (a count change, a reallocation), lowered by the dirty spheres of any other
  float sphere_rmin = INFINITY;
  // audio_target_id of every synced record and their histogram (index = id + 32768), kept
  // incrementally from the dirty records (permeation loss test counts of counting frames)
  std::vector<int16_t> synced_tid[3];
  std::vector<int> tid_hist[3];
  art_collider_sync_stats last_sync{};
  int reserved[3] = {0, 0, 0};   // art_colliders_reserve
  art_collider_resize_stats last_resize{};
  bool relabel_pending = false;  // last_resize.relabelled is still to be read from device 0's relabel_status
  // adds and effective removes since the bound scene's last kd build (the synced ones), and those
  // since the last sync: a relabelled tree loses tightness with them (art_store.cpp, kResortDen)
  long long churn = 0, churn_unsynced = 0;
  std::vector<uint8_t> cpu_recs[3];  // CPU backend: the records at the last sync
  // pinned update images of art_colliders_sync, a ring (sync s uses slot s % kUpdRing): a slot is
  // reused only after the previous epoch's syncs are done (one event per epoch, not per sync)
  static constexpr int kUpdRing = 8;
  HostBuf h_upd[kUpdRing];
  uint64_t upd_seq = 0;
};

// The resident target store of a context (art_colliders.h, second half): the NextBatch mirror of
// AudioTargetPositions with dirty marks, and the positions of the last sync (the JobBatch snapshot
// that resident-target frames read).
struct TargetStore {
  std::vector<float> pos;         // count * 3
  int count = 0;
  std::vector<uint8_t> dirty;     // per target
  std::vector<int> dirty_list;
  int synced = 0;
  bool store_synced = false;
  std::vector<float> snap;        // synced * 3: the positions at the last sync
  art_target_sync_stats last_sync{};
  // identity of the mirror's targets since the last sync: src[i] is the synced index target i held
  // then, -1 for a target added since (add appends -1, a swap-back carries the last one's along)
  std::vector<int> src;           // count
  std::vector<int> last_map;      // synced: src at the last sync (art_debug_target_sync_map)
  // the syncs' maps composed since the last art_target_follow_mark: follow[i] is the index the target
  // now at synced index i held in the base list (the synced list at the mark; empty before the first
  // sync), -1 if it was not in it (art_target_follow_map)
  std::vector<int> follow;        // synced
  int base_count = 0;
  int last_remove_owners[3] = {0, 0, 0};  // art_target_last_remove_owners
  int reserved = 0;               // art_targets_reserve
  art_target_resize_stats last_resize{};
};

}  // namespace art

struct art_ctx {
  std::vector<art::Device> devs;   // empty for the CPU backend
  art::CpuEngine* cpu = nullptr;   // art_create(0): the CPU backend (art_cpu.cpp)
  std::string err;
  uint32_t flags = 0;
  art::HostBuf h_in, h_block;
  art::HostBuf h_dsp;            // staging of art_dsp_process
  int last_dsp_kernel = 0;       // ART_DSP_KERNEL_* of the last per-sample DSP call (art_debug_last_dsp_kernel)
  // the audio tick's spatializer settings (art_dsp_settings_bind, art_dsp_settings_bind_classes):
  // class 0's scalars with its curves pointing into devs[0].tick_curves, where the table of all
  // class_count records lies too (d_table); target_class is the class map (art_dsp_target_classes_*:
  // host state, empty = every target is class 0, untouched by a bind)
  struct TickSettings {
    bool bound = false;
    art_spatializer_settings st{};
    int sample_rate = 0;
    int class_count = 0;
    const art_spatializer_settings* d_table = nullptr;
    std::vector<uint8_t> target_class;
  } tick;
  art::Frame fr;                 // frame of the bound scene / last schedule
  // in-flight frame
  bool inflight = false;
  art_handle handle = 0;
  uint64_t next_handle = 1;
  std::vector<art_fan> fans;
  bool counted = false;
  art_test_counts last_counts{};
  bool has_counts = false;
  std::vector<uint64_t> nonowned;  // per type (s, a, o): sum over targets of non-owned colliders
  // audio_target_id histogram (index = id + 32768) per kind of the colliders a scene bound from desc
  // arrays holds (the resident store keeps its own, ColliderStore::tid_hist): which target indices
  // own colliders, for a count-changing target sync
  std::vector<int> bind_tid_hist[3];
  art::ColliderStore store;
  art::TargetStore targets;
  // Host phases of the Unity-facing frame (ART_HOST_TIMES=1 in the environment at art_create:
  // steady_clock marks in art_schedule / art_complete, means printed by art_destroy to stderr).
  struct HostPhases {
    bool on = false;
    uint64_t frames = 0;
    double us[8] = {};
  } hp;
};

namespace art {

struct PhaseClock {
  art_ctx::HostPhases* hp;
  std::chrono::steady_clock::time_point t;
  explicit PhaseClock(art_ctx::HostPhases* h) : hp(h && h->on ? h : nullptr) { if (hp) t = std::chrono::steady_clock::now(); }
  void mark(int phase) {
    if (!hp) return;
    const auto n = std::chrono::steady_clock::now();
    hp->us[phase] += std::chrono::duration<double, std::micro>(n - t).count();
    t = n;
  }
};

int fail(art_ctx* c, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

#define HIP_TRY(ctx, expr)                                                                          \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return art::fail(ctx, ART_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// art_frame.cpp
int validate_desc(art_ctx* c, const art_frame_desc* d);
FanLayout make_layout(const art_frame_desc* d, uint32_t out_flags);
void make_frame(const art_frame_desc* d, uint32_t out_flags, Frame& f, const int* resident_counts = nullptr,
                bool resident_targets = false, int target_capacity = 0, const int* collider_capacity = nullptr);
// True when the permeation slot table of f (Frame::slot_batch) is the same for T targets.
bool slot_tables_hold(const Frame& f, int T);
void pack_inputs(const art_frame_desc* d, const Frame& f, uint8_t* h);
struct ConeTable {
  CellCone cone[kCells];
  float alpha_max = 0.0f;
  ConeTable();
};
const ConeTable& cone_table();
// The sections of a frame's record allocation, carved in this order: the decoded records (empty
// when the store holds them), the sorted scene copy and BVH (art_bvh.hip), the muffle cell lists
// (art_cells.hip; cones and compact are set by upload_scene).
DecodedColliders carve_decoded(Carver& c, const Frame& f);
SortBufs carve_sort(Carver& c, const Frame& f);
CellBufs carve_cells(Carver& c, const Frame& f);

// art_scene.cpp
int ensure_side(art_ctx* c, SideStream& s);  // the stream and its fork / join events, created once
int scene_reader_begin(art_ctx* c, Device& dv, const Frame& f, hipStream_t st);
int scene_reader_end(art_ctx* c, Device& dv, hipStream_t st);
int upload_scene(art_ctx* c, Device& dv, const Frame& f, const uint8_t* h_in);
void snapshot_cell_base(art_ctx* c);
bool cell_still_valid(int kind, const uint8_t* now, const uint8_t* base);
// min(bound, the smallest |radius| of the n sphere records at recs) (DevScene::r_min; a non-finite radius counts as 0)
float spheres_rmin(const void* recs, int n, float bound);

// art_enqueue.cpp
// What an event pair of Device::ev_used times: a stage of the frame, or one kernel of the raytrace
// stage (kEvKernel0 + MarkKind, ART_CTX_TIME_EACH_KERNEL).
enum EvKind { kEvRaytrace = 0, kEvPermeate = 1, kEvReduce = 2, kEvKernel0 = 3 };
hipEvent_t pool_event(Device& dv, size_t i);
int enqueue_kernels(art_ctx* c, Device& dv, const Frame& f, const float* d_origins, int fan_count, uint8_t* d_block,
                    hipStream_t st, bool count, const float* perm_in = nullptr, uint8_t* host_out = nullptr);
int read_counts(art_ctx* c, Device& dv, hipStream_t st, art_test_counts* out, bool accumulate);
bool compact_slots(const Frame& f, bool need_echo);
int enqueue_device_frame(art_ctx* c, Device& dv, const Frame& f, const uint8_t* hin, uint8_t* hb, bool need_echo, bool count,
                         bool inject_failure = false, PhaseClock* pc = nullptr);

}  // namespace art
