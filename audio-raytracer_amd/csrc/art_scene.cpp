// art_scene.cpp — one device's scene: the upload of a frame's packed inputs, the record decode and
// the BVH / muffle cell-list builds behind it, the caches that let a frame skip them, and the fence
// between device-path frames on a caller's stream and the context stream.
#include <cmath>

#include "art_ctx.hpp"
#include "art_frame_math.hpp"
#include "unity_math.hpp"

namespace art {

#ifndef ART_CELLS_BESIDE_BVH
#define ART_CELLS_BESIDE_BVH 1
#endif
constexpr bool kCellsBesideBvh = ART_CELLS_BESIDE_BVH != 0;
#ifndef ART_CELLS_COMPACT
#define ART_CELLS_COMPACT 1
#endif

int LaunchFence::mark_done(art_ctx* c) {
  if (recorded) return ART_OK;
  if (!done) HIP_TRY(c, hipEventCreateWithFlags(&done, hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(done, stream));
  recorded = true;
  return ART_OK;
}
int LaunchFence::wait(art_ctx* c, hipStream_t waiter) {
  if (pending) {
    int rc = mark_done(c);
    if (rc) return rc;
    HIP_TRY(c, hipStreamWaitEvent(waiter, done, 0));
    pending = false;
  }
  return ART_OK;
}

// A reader of the bound scene enqueued on the caller's stream st (a device frame, the audio tick).
// Before it: st waits for the resident store's last sync and for the previous reader when they ran
// on other streams (frames also share the context's accumulators and pair buffers; on the same
// stream, stream order already does).
int scene_reader_begin(art_ctx* c, Device& dv, const Frame& f, hipStream_t st) {
  if ((f.resident || f.res_targets) && dv.store.done && st != dv.store.stream) HIP_TRY(c, hipStreamWaitEvent(st, dv.store.done, 0));
  if (dv.fence.pending && st != dv.fence.stream) {
    int rc = dv.fence.mark_done(c);
    if (rc) return rc;
    HIP_TRY(c, hipStreamWaitEvent(st, dv.fence.done, 0));
  }
  return ART_OK;
}
// After it: the next sync, bind or schedule rewrites the scene or reuses the shared buffers on
// dv.stream after this reader (LaunchFence::wait records the event on st then).
int scene_reader_end(art_ctx* c, Device& dv, hipStream_t st) {
  dv.fence.pending = true;
  dv.fence.stream = st;
  dv.fence.recorded = false;
  if (c->flags & ART_CTX_EVENT_EACH_LAUNCH) return dv.fence.mark_done(c);  // opt-in: the caller may drop its stream after this call
  return ART_OK;
}

int ensure_side(art_ctx* c, SideStream& s) {
  if (s.st) return ART_OK;
  HIP_TRY(c, hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
  HIP_TRY(c, hipEventCreateWithFlags(&s.fork, hipEventDisableTiming));
  HIP_TRY(c, hipEventCreateWithFlags(&s.join, hipEventDisableTiming));
  return ART_OK;
}

// The resident store's records as the muffle cell lists were just built from them (none dirty).
void snapshot_cell_base(art_ctx* c) {
  ColliderStore& s = c->store;
  bool clean = true;
  for (int k = 0; k < 3; ++k) clean &= s.kinds[k].dirty_list.empty();
  for (int k = 0; k < 3; ++k) s.cell_base[k] = s.kinds[k].recs;
  s.cell_base_ok = clean;
}

// The lists built from record `base` still hold record `now` (cell_slack): same extents and owner,
// centre moved by at most half the slack of the base's bounding radius.
bool cell_still_valid(int kind, const uint8_t* now, const uint8_t* base) {
  const size_t ext = kind == 0 ? 2 : 6;  // radius (half) or size (half3), after the centre
  const size_t tid_off = kTidOff[kind];
  if (memcmp(now + 6, base + 6, ext) != 0 || memcmp(now + tid_off, base + tid_off, 2) != 0) return false;
  uint16_t cn[3], cb[3], e[3] = {0, 0, 0};
  memcpy(cn, now, 6);
  memcpy(cb, base, 6);
  memcpy(e, base + 6, ext);
  float d2 = 0.0f, r2 = 0.0f;
  for (int a = 0; a < 3; ++a) {
    const float dd = art::f16tof32(cn[a]) - art::f16tof32(cb[a]);
    d2 += dd * dd;
    const float ea = art::f16tof32(e[a]);
    r2 += ea * ea;
  }
  const float half = 0.5f * art::cell_slack(std::sqrt(r2)) * 0.999f;
  return std::isfinite(d2) && std::isfinite(r2) && d2 <= half * half;
}

float spheres_rmin(const void* recs, int n, float bound) {
  const uint8_t* p = static_cast<const uint8_t*>(recs);
  for (int i = 0; i < n; ++i) {
    art_sphere s;
    memcpy(&s, p + (size_t)i * sizeof(art_sphere), sizeof s);
    const float r = std::fabs(art::f16tof32(s.radius));
    bound = std::isfinite(r) ? std::min(bound, r) : 0.0f;
  }
  return bound;
}

// The BVH of dv.sc on dv.stream: the resident scene's kept orders (refit when the store changed
// since) or a new sort and build.
static int build_bvh(art_ctx* c, Device& dv, const Frame& f, bool reuse) {
  DevScene& sc = dv.sc;
  if (reuse) {  // same resident colliders (or only moved ones): keep the orders, refit if needed
    const DevScene& o = dv.sorted.sc;
    sc.bvh = o.bvh; sc.bvh_ref = o.bvh_ref; sc.bvh_leaf = o.bvh_leaf;
    sc.bvh_levels = o.bvh_levels; sc.bvh_leaf0 = o.bvh_leaf0;
    if (dv.sorted.gen != c->store.sync_gen && launch_refit_scene(sc, dv.sb, dv.stream) != 0)
      return fail(c, ART_E_DEVICE, "collider refit failed");
  } else if (launch_sort_scene(sc, dv.sb, dv.stream) != 0) {
    return fail(c, ART_E_DEVICE, "collider sort failed");
  } else if (f.resident) {
    c->store.churn = 0;  // a fresh kd order of the synced colliders
  }
  dv.sorted.gen = f.resident ? c->store.sync_gen : ~0ull;
  dv.sorted.soa = dv.soa.p;
  dv.sorted.n[0] = f.ns; dv.sorted.n[1] = f.na; dv.sorted.n[2] = f.no;
  dv.sorted.ccap = f.ccap();
  return ART_OK;
}

// Upload the packed inputs to one device and build its SoA records (async on dv.stream).
int upload_scene(art_ctx* c, Device& dv, const Frame& f, const uint8_t* h_in) {
  HIP_TRY(c, hipSetDevice(dv.id));
  if (int rc = dv.fence.wait(c, dv.stream)) return rc;
  if (!dv.raw.reserve(f.raw_bytes) || !dv.soa.reserve(f.soa_bytes)) return fail(c, ART_E_NOMEM, "device allocation failed");
  const int key[10] = {f.ns, f.na, f.no, f.T, f.R, f.TC, f.H, f.fp.vol_n, f.fp.muf_n, (int)f.raw_bytes};
  UploadCache& last = dv.last;
  // (resident frames skip the compare: a sync rewrites the bound scene's records or targets in place)
  if (!f.resident && !f.res_targets && last.valid && last.raw_p == dv.raw.p && last.soa_p == dv.soa.p &&
      memcmp(last.key, key, sizeof key) == 0 && memcmp(last.raw.data(), h_in, f.raw_bytes) == 0) {
    dv.sc = last.sc;  // device records, sorted copies and BVH are those of these same inputs
    dv.bound = true;
    return ART_OK;
  }
  last.valid = false;
  HIP_TRY(c, hipMemcpyAsync(dv.raw.p, h_in, f.raw_bytes, hipMemcpyHostToDevice, dv.stream));
  uint8_t* raw = static_cast<uint8_t*>(dv.raw.p);
  Carver soa{reinterpret_cast<uintptr_t>(dv.soa.p)};
  const DecodedColliders out = carve_decoded(soa, f);
  dv.sb = carve_sort(soa, f);
  CellBufs cb = carve_cells(soa, f);
  DevScene& sc = dv.sc;
  if (f.resident) {  // records and bounds of the last art_colliders_sync
    set_colliders(sc, dv.store.dec, dv.store.n);
    set_r_min(sc, c->store.sphere_rmin);
  } else {
    set_r_min(sc, spheres_rmin(h_in + f.off_sph, f.ns, INFINITY));
    const RawColliders in = {reinterpret_cast<const art_sphere*>(raw + f.off_sph), reinterpret_cast<const art_aabb*>(raw + f.off_aabb),
                             reinterpret_cast<const art_obb*>(raw + f.off_obb), f.ns, f.na, f.no};
    launch_prep(in, out, dv.stream);
    HIP_TRY(c, hipGetLastError());
    const int n[3] = {f.ns, f.na, f.no};
    set_colliders(sc, out, n);
  }
  sc.targets = reinterpret_cast<const float*>(raw + f.off_tgt); sc.T = f.T;
  sc.dirs = reinterpret_cast<const uint16_t*>(raw + f.off_dirs); sc.R = f.R;
  sc.bvh = nullptr; sc.bvh_ref = nullptr; sc.bvh_leaf = nullptr; sc.bvh_levels = 0;
  if (!dv.cones.p) {
    if (!dv.cones.reserve(sizeof(CellCone) * kCells)) return fail(c, ART_E_NOMEM, "device allocation failed");
    HIP_TRY(c, hipMemcpyAsync(dv.cones.p, cone_table().cone, sizeof(CellCone) * kCells, hipMemcpyHostToDevice, dv.stream));
  }
  // the arena's (tail, dropped) as the next art_targets_sync reads it, without waiting (a stale
  // value only delays or hastens a compaction: the device checks the capacity itself)
  if (!dv.cell_status.p) {
    if (!dv.cell_status.reserve(2 * sizeof(uint32_t))) return fail(c, ART_E_NOMEM, "pinned allocation failed");
    memset(dv.cell_status.p, 0, 2 * sizeof(uint32_t));
  }
  void* status = nullptr;
  HIP_TRY(c, hipHostGetDevicePointer(&status, dv.cell_status.p, 0));
  // The cell lists need only the decoded colliders and the targets (cells_box_kernel gives their
  // distance bound), the BVH only the colliders: with a rebuilt BVH the lists build on the side
  // stream beside it (its surface-area passes occupy a few CUs for ~70 us), joined before the frame.
  const bool reuse = dv.sorted.matches(f, dv.soa.p);
  hipStream_t cells_st = dv.stream;
  if (!reuse && kCellsBesideBvh && f.cells_cap > 0) {
    if (int rc = ensure_side(c, dv.side)) return rc;
    HIP_TRY(c, hipEventRecord(dv.side.fork, dv.stream));
    HIP_TRY(c, hipStreamWaitEvent(dv.side.st, dv.side.fork, 0));
    cells_st = dv.side.st;
  }
  // the BVH's launches first: its first kernels reach the CUs before the lists' wide passes fill them
  int rc = build_bvh(c, dv, f, reuse);
  if (rc == 0) {
    cb.cones = static_cast<const CellCone*>(dv.cones.p);
    cb.alpha_max = cone_table().alpha_max;
    // 4-B entries (by the kinds' capacities: the entry format holds for every count the scene can take)
    cb.compact = (ART_CELLS_COMPACT && std::max(f.ns, f.Cc[0]) < (1 << 16) && std::max(f.na, f.Cc[1]) < (1 << 16) &&
                  std::max(f.no, f.Cc[2]) < (1 << 16)) ? 1u : 0u;
    cb.status = static_cast<uint32_t*>(status);
    dv.cb = cb;
    if (launch_build_cells(sc, dv.cb, cells_st) != 0) rc = fail(c, ART_E_DEVICE, "muffle cell lists failed");
    dv.cells_partial = false;
  }
  if (rc) {  // kernels may already be queued on the side stream: later work on dv.stream waits for them
    if (cells_st != dv.stream && hipEventRecord(dv.side.join, cells_st) == hipSuccess)
      (void)hipStreamWaitEvent(dv.stream, dv.side.join, 0);
    return rc;
  }
  if (cells_st != dv.stream) {  // the frame's kernels wait for the lists
    HIP_TRY(c, hipEventRecord(dv.side.join, cells_st));
    HIP_TRY(c, hipStreamWaitEvent(dv.stream, dv.side.join, 0));
  }
  dv.sorted.sc = sc;
  if (f.resident) snapshot_cell_base(c);  // the store's synced records (clean unless edited since)
  else c->store.cell_base_ok = false;
  HIP_TRY(c, hipGetLastError());
  if (!f.resident && !f.res_targets) {
    last.raw.assign(h_in, h_in + f.raw_bytes);
    memcpy(last.key, key, sizeof key);
    last.raw_p = dv.raw.p;
    last.soa_p = dv.soa.p;
    last.sc = sc;
    last.valid = true;
  }
  dv.bound = true;
  return ART_OK;
}

}  // namespace art
