// art_store.cpp — the resident scene store (include/art_colliders.h): the host mirrors of the
// caller's collider lists and target positions with dirty marks, and art_colliders_sync /
// art_targets_sync, each of which uploads what changed to every device as a plan (plan_sync /
// plan_target_sync) and four steps (stage_image, sync_device per device, commit_sync; the target
// half's are stage_target_image, sync_device_targets, commit_target_sync). Both kinds of sync
// share the ring of pinned update images and its epoch events.
#include <cstdlib>

#include "art_ctx.hpp"
#include "art_frame_math.hpp"

using namespace art;

namespace {

// The store's device layout for the capacities cap[3]: the AoS lists in one buffer, the decoded
// records and bounds in another (base 0: only the sizes, in the carvers' offsets).
struct StoreViews {
  art_sphere* sph; art_aabb* aabb; art_obb* obb;
  DecodedColliders dec;
};
StoreViews store_views(const int cap[3], Carver& raw, Carver& soa) {
  StoreViews v;
  v.sph = raw.take<art_sphere>((size_t)cap[0] * sizeof(art_sphere));
  v.aabb = raw.take<art_aabb>((size_t)cap[1] * sizeof(art_aabb));
  v.obb = raw.take<art_obb>((size_t)cap[2] * sizeof(art_obb));
  v.dec.sph = soa.take<SphereRec>((size_t)cap[0] * sizeof(SphereRec));
  v.dec.sphc = soa.take<SphereCold>((size_t)cap[0] * sizeof(SphereCold));
  v.dec.aabb = soa.take<AabbRec>((size_t)cap[1] * sizeof(AabbRec));
  v.dec.aabbc = soa.take<AabbCold>((size_t)cap[1] * sizeof(AabbCold));
  v.dec.obb = soa.take<ObbRec>((size_t)cap[2] * sizeof(ObbRec));
  v.dec.obbc = soa.take<ObbCold>((size_t)cap[2] * sizeof(ObbCold));
  v.dec.cull = soa.take<CullRec>((size_t)(cap[0] + cap[1] + cap[2]) * sizeof(CullRec));
  return v;
}

// A sync's slot in the ring of pinned update images and the ring's epoch (0 / 1).
// The update image goes to ring slot seq % kUpdRing. A new epoch reuses the ring: every sync of the
// previous epoch has finished reading its slot once that epoch's event (recorded after its last
// sync, on that sync's stream) has completed. Each sync's stream is ordered after the earlier
// syncs' (a launch on a new stream waits on the old one, a context-stream sync on the launch
// stream), so that one event covers the whole epoch.
struct RingSlot { int slot, ep; };
RingSlot take_ring_slot(ColliderStore& s) {
  const uint64_t seq = s.upd_seq++;
  return RingSlot{(int)(seq % ColliderStore::kUpdRing), (int)((seq / ColliderStore::kUpdRing) & 1u)};
}
// A sync that starts a new epoch first waits for the last one (before it writes its image).
int wait_ring_epoch(art_ctx* c, const RingSlot& r) {
  if (r.slot != 0) return ART_OK;
  for (Device& dv : c->devs)
    if (dv.store.epoch_pending[r.ep ^ 1]) {
      HIP_TRY(c, hipSetDevice(dv.id));
      HIP_TRY(c, hipEventSynchronize(dv.store.epoch[r.ep ^ 1]));
      dv.store.epoch_pending[r.ep ^ 1] = false;
    }
  return ART_OK;
}

// What one art_colliders_sync does, decided on the host before any device is given work.
struct SyncPlan {
  int n[3];                   // the lists' counts
  bool counts_changed;        // against the last sync (true for the first)
  bool fresh;                 // some device's capacity was (re)allocated: every record is uploaded
  std::vector<int> lists[3];  // dirty records of each kind (all of them when fresh), ascending
  // update image: [idx_s][rec_s][idx_a][rec_a][idx_o][rec_o], 16-B aligned sections
  size_t off_idx[3], off_rec[3], bytes;
  int nd;                     // dirty records over the kinds
  bool cells_ok;              // every changed collider stayed within the muffle cell lists' slack
  RingSlot ring;              // the image's slot in the pinned ring
  // A count change that every device's bound resident scene follows in place (the scene was bound
  // with a collider capacity, every kind stays within it and no device list has to grow): the
  // labels that appear and vanish at the kinds' tails, and whether the leaf order is relabelled
  // (bvh_relabel_kernel) or sorted again in the same buffers.
  int old_n[3];               // the counts of the last sync
  int added, removed;
  bool resize;
  bool rebuild;               // (of a resize) the full kd build instead of the relabel
};

// A relabelled tree loses tightness: survivors that a swap-back moved and new colliders sit where a
// stranger was. Once the adds and effective removes since the last kd build exceed 1 / kResortDen of
// the colliders, the count-changing sync sorts again in place; 1 = at every count change, 0 = never.
// Measured at config 2 (profiles/collider_churn.txt): 64 churned colliders of 4096
// already take the static frame from 0.092 to 0.319 ms, no fraction down to 1/64 stays within the
// measurement spread of a fresh bind, and the step that sorts every time is the fastest against the
// rebind it replaces. So the default sorts at every count change, and the relabel is what
// ART_BVH_RESORT_DEN in the environment (read per sync) asks for.
constexpr int kResortDen = 1;
int resort_den() {
  const char* e = getenv("ART_BVH_RESORT_DEN");
  if (!e || !*e) return kResortDen;
  const long v = strtol(e, nullptr, 10);
  return v < 0 ? kResortDen : (int)std::min<long>(v, 1 << 30);
}

// No HIP call, but it does change host state: it grows the devices' capacities (x2) and marks them
// fresh (sync_device then frees and reallocates their buffers), and it takes the sync's generation
// and ring sequence numbers.
SyncPlan plan_sync(art_ctx& c) {
  ColliderStore& s = c.store;
  SyncPlan p;
  for (int k = 0; k < 3; ++k) p.n[k] = s.kinds[k].count;
  p.counts_changed = !s.store_synced;
  for (int k = 0; k < 3; ++k) p.counts_changed |= p.n[k] != s.synced[k];
  p.fresh = false;
  for (Device& dv : c.devs) {  // a list outgrew the device capacity: everything is uploaded again
    StoreDev& d = dv.store;
    // (a reserved capacity the lists do not have yet is taken now unless a bound scene reads them)
    const bool reserve_grows = !dv.bound && (s.reserved[0] > d.cap[0] || s.reserved[1] > d.cap[1] || s.reserved[2] > d.cap[2]);
    if (p.n[0] > d.cap[0] || p.n[1] > d.cap[1] || p.n[2] > d.cap[2] || !d.raw.p || reserve_grows) {
      for (int k = 0; k < 3; ++k) d.cap[k] = std::max({p.n[k], 2 * d.cap[k], 64, s.reserved[k]});
      d.fresh = true;
    }
    p.fresh |= d.fresh;
  }
  // the labels (kind, index) that appear and vanish: only at the kinds' tails (swap-back removes)
  p.added = p.removed = 0;
  for (int k = 0; k < 3; ++k) {
    p.old_n[k] = s.store_synced ? s.synced[k] : 0;
    p.added += std::max(0, p.n[k] - p.old_n[k]);
    p.removed += std::max(0, p.old_n[k] - p.n[k]);
  }
  s.churn += s.churn_unsynced;
  s.churn_unsynced = 0;
  const Frame& f = c.fr;
  p.resize = !c.cpu && p.counts_changed && s.store_synced && !p.fresh && f.resident && f.Cc[0] + f.Cc[1] + f.Cc[2] > 0 &&
             !c.devs.empty();
  for (int k = 0; p.resize && k < 3; ++k) p.resize = p.n[k] <= f.Cc[k];
  for (const Device& dv : c.devs)
    p.resize = p.resize && dv.bound && dv.sc.ns == p.old_n[0] && dv.sc.na == p.old_n[1] && dv.sc.no == p.old_n[2];
  p.rebuild = false;
  if (p.resize) {
    const long long n_old = (long long)p.old_n[0] + p.old_n[1] + p.old_n[2], n_new = (long long)p.n[0] + p.n[1] + p.n[2];
    const int den = resort_den();
    p.rebuild = n_old == 0 || n_new == 0 || f.ccap() > kSyncRefitMax || den == 1 || (den > 1 && s.churn > n_new / den);
    if (p.rebuild) s.churn = 0;
  }
  p.bytes = 0;
  for (int k = 0; k < 3; ++k) {
    auto& K = s.kinds[k];
    std::vector<int>& l = p.lists[k];
    if (p.fresh) {
      l.resize((size_t)p.n[k]);
      for (int i = 0; i < p.n[k]; ++i) l[(size_t)i] = i;
    } else {
      for (int i : K.dirty_list)
        if (i < p.n[k] && K.dirty[(size_t)i]) l.push_back(i);
      std::sort(l.begin(), l.end());
      l.erase(std::unique(l.begin(), l.end()), l.end());
    }
    p.off_idx[k] = p.bytes; p.bytes = align_up(p.bytes + l.size() * 4, 16);
    p.off_rec[k] = p.bytes; p.bytes = align_up(p.bytes + l.size() * kRecSize[k], 16);
  }
  if (c.cpu) p.bytes = 0;  // the CPU backend keeps no device copy (commit_sync snapshots the lists)
  p.nd = (int)(p.lists[0].size() + p.lists[1].size() + p.lists[2].size());
  if (p.nd || p.counts_changed) ++s.sync_gen;  // resident frames refit / rebuild their sorted copies
  // the muffle cell lists need a rebuild unless every changed collider stayed within their slack
  p.cells_ok = s.cell_base_ok && !p.counts_changed && !p.fresh;
  for (int k = 0; p.cells_ok && k < 3; ++k) {
    const size_t rs = kRecSize[k];
    if (s.cell_base[k].size() < (size_t)p.n[k] * rs) { p.cells_ok = false; break; }
    for (int i : p.lists[k])
      if (!cell_still_valid(k, s.kinds[k].recs.data() + (size_t)i * rs, s.cell_base[k].data() + (size_t)i * rs)) {
        p.cells_ok = false;
        break;
      }
  }
  // the spheres' radius bound (DevScene::r_min): a sync that walks every record recomputes it, any
  // other only lowers it by the dirty spheres (the mirror holds the records as the devices will)
  if (p.counts_changed || p.fresh) s.sphere_rmin = spheres_rmin(s.kinds[0].recs.data(), p.n[0], INFINITY);
  else
    for (int i : p.lists[0]) s.sphere_rmin = spheres_rmin(s.kinds[0].recs.data() + (size_t)i * kRecSize[0], 1, s.sphere_rmin);
  p.ring = take_ring_slot(s);
  return p;
}

// The pinned update image of the plan, in its ring slot (a new epoch first waits for the last one).
int stage_image(art_ctx* c, const SyncPlan& p) {
  ColliderStore& s = c->store;
  if (int rc = wait_ring_epoch(c, p.ring)) return rc;
  if (!p.bytes) return ART_OK;
  if (!s.h_upd[p.ring.slot].reserve(p.bytes)) return fail(c, ART_E_NOMEM, "pinned allocation failed");
  uint8_t* h = static_cast<uint8_t*>(s.h_upd[p.ring.slot].p);
  for (int k = 0; k < 3; ++k) {
    const size_t rs = kRecSize[k];
    for (size_t j = 0; j < p.lists[k].size(); ++j) {
      const int i = p.lists[k][j];
      memcpy(h + p.off_idx[k] + j * 4, &i, 4);
      memcpy(h + p.off_rec[k] + j * rs, s.kinds[k].recs.data() + (size_t)i * rs, rs);
    }
  }
  return ART_OK;
}

// The plan's dirty records in the update image at `image` (a device copy, or the pinned image as
// the device sees it), scattered into the store's lists and decoded records.
ScatterArgs scatter_args(const SyncPlan& p, const void* image, const StoreViews& v) {
  const uint8_t* u = static_cast<const uint8_t*>(image);
  ScatterArgs a;
  a.idx_s = reinterpret_cast<const int*>(u + p.off_idx[0]); a.rec_s = reinterpret_cast<const art_sphere*>(u + p.off_rec[0]);
  a.idx_a = reinterpret_cast<const int*>(u + p.off_idx[1]); a.rec_a = reinterpret_cast<const art_aabb*>(u + p.off_rec[1]);
  a.idx_o = reinterpret_cast<const int*>(u + p.off_idx[2]); a.rec_o = reinterpret_cast<const art_obb*>(u + p.off_rec[2]);
  a.ds = (int)p.lists[0].size(); a.da = (int)p.lists[1].size(); a.dob = (int)p.lists[2].size();
  a.sph = v.sph; a.aabb = v.aabb; a.obb = v.obb;
  a.ns = p.n[0]; a.na = p.n[1];
  const DecodedColliders& d = v.dec;
  a.osph = d.sph; a.osphc = d.sphc; a.oaabb = d.aabb; a.oaabbc = d.aabbc; a.oobb = d.obb; a.oobbc = d.obbc; a.cull = d.cull;
  return a;
}

// The event that frees the ring for the epoch after the next, recorded after the epoch's last sync
// once the device may have been given work that reads the slot: by record() on the normal exits of
// sync_device (a failure fails the sync, as before), by the destructor on its error exits.
struct EpochMark {
  StoreDev& s;
  const RingSlot& p;
  hipStream_t ss;
  bool done = false;
  int record(art_ctx* c) {
    done = true;
    if (p.slot != ColliderStore::kUpdRing - 1) return ART_OK;
    if (!s.epoch[p.ep]) HIP_TRY(c, hipEventCreateWithFlags(&s.epoch[p.ep], hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(s.epoch[p.ep], ss));
    s.epoch_pending[p.ep] = true;
    return ART_OK;
  }
  ~EpochMark() { if (!done) (void)record(nullptr); }  // (no context: the first error's text is kept)
};

// One device's share of a sync, async on the stream it picks: scatter + decode of the dirty records
// (or the full decode after a count change), the bound resident scene's refit and, outside the
// slack, its cell lists.
int sync_device(art_ctx* c, Device& dv, const SyncPlan& p, bool& cells_rebuilt, art_collider_resize_stats& rs) {
  StoreDev& s = dv.store;
  HIP_TRY(c, hipSetDevice(dv.id));
  if (s.fresh) { s.raw.release(); s.soa.release(); }  // grown capacity: new buffers, every record uploaded
  Carver raw{0}, soa{0};
  store_views(s.cap, raw, soa);
  if (!s.raw.reserve(raw.off) || !s.soa.reserve(soa.off) || (p.bytes && !s.upd.reserve(p.bytes)))
    return fail(c, ART_E_NOMEM, "device allocation failed");
  raw = Carver{reinterpret_cast<uintptr_t>(s.raw.p)};
  soa = Carver{reinterpret_cast<uintptr_t>(s.soa.p)};
  const StoreViews v = store_views(s.cap, raw, soa);
  void* h = c->store.h_upd[p.ring.slot].p;
  // Device-path frames still read the records / BVH being rewritten. The sync runs on the stream of
  // the last such frame when its completion is not recorded yet (the stream is valid until this
  // call, art_device.h): stream order puts it after that frame and before the next launch on the
  // same stream, with no cross-stream events (each costs the queue ~5-10 us of idle). Otherwise
  // it runs on the context stream, after the frame's completion event.
  const hipStream_t ss = (dv.fence.pending && !dv.fence.recorded) ? dv.fence.stream : dv.stream;
  if (ss == dv.stream)
    if (int rc = dv.fence.wait(c, dv.stream)) return rc;
  s.stream = ss;
  EpochMark epoch{s, p.ring, ss};
  // moved colliders of a bound resident scene: one launch scatters the records from the pinned image
  // and refits the BVH (launch_sync_refit), below
  const bool refit_follows = p.nd && dv.bound && c->fr.resident && !p.counts_changed;
  const bool resize = p.resize && dv.bound && c->fr.resident;  // (the same for every device: plan_sync)
  const bool fused = refit_follows && (long long)p.n[0] + p.n[1] + p.n[2] <= kSyncRefitMax && dv.sc.bvh_levels > 0 && dv.sb.bvh;
  if (p.nd && !fused) {
    HIP_TRY(c, hipMemcpyAsync(s.upd.p, h, p.bytes, hipMemcpyHostToDevice, ss));
    launch_scatter_prep(scatter_args(p, s.upd.p, v), ss);
    HIP_TRY(c, hipGetLastError());
  }
  // a count change moves the bounds of the later kinds (global order spheres, AABBs, OBBs)
  if (p.counts_changed && !p.fresh && p.n[0] + p.n[1] + p.n[2] > 0) {
    launch_prep(RawColliders{v.sph, v.aabb, v.obb, p.n[0], p.n[1], p.n[2]}, v.dec, ss);
    HIP_TRY(c, hipGetLastError());
  }
  // stream-ordered: frames on ss follow. A sync on the context stream records done, which
  // device-path launches on other streams wait on (a refit below records it after its kernels). A
  // sync on the launch stream records nothing (each record costs the queue ~5 us): a launch on
  // another stream waits on that stream's fence, work on dv.stream on it through LaunchFence::wait.
  if (!s.done) HIP_TRY(c, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  const bool lazy = ss != dv.stream;
  if (!refit_follows && !resize && !lazy) HIP_TRY(c, hipEventRecord(s.done, ss));
  s.dec = v.dec;
  for (int k = 0; k < 3; ++k) s.n[k] = p.n[k];
  s.fresh = false;
  if (!(dv.bound && c->fr.resident)) return epoch.record(c);
  if (resize) {
    // A count change within the scene's capacity, in its buffers and in stream order: the leaf order
    // follows the labels that vanished and appeared (or is sorted again), the full refit rewrites
    // every leaf slot (the empty ones up to the new leaf count, the slot stride when the first OBB
    // appears or the last one leaves) and every node (a level change needs nothing more), and the
    // cell lists are built for the new records. Nothing is allocated.
    if (!dv.relabel_status.p) {  // (a scene bound by art_schedule: art_scene_bind has it already)
      if (!dv.relabel_status.reserve(sizeof(uint32_t))) return fail(c, ART_E_NOMEM, "pinned allocation failed");
      memset(dv.relabel_status.p, 0, sizeof(uint32_t));
    }
    const int levels_before = dv.sc.bvh_levels;
    const bool rebuild = p.rebuild || dv.sc.bvh_levels == 0 || !dv.sb.bvh;
    set_colliders(dv.sc, v.dec, p.n);
    set_r_min(dv.sc, c->store.sphere_rmin);
    // Beside a kd build the lists build on the side stream, as at a bind (they need the decoded
    // records and the targets, not the tree; the sort's surface-area passes occupy a few CUs).
    hipStream_t cells_st = ss;
    if (rebuild && dv.cb.cap > 0 && p.n[0] + p.n[1] + p.n[2] > 0) {
      if (int rc = ensure_side(c, dv.side)) return rc;
      HIP_TRY(c, hipEventRecord(dv.side.fork, ss));
      HIP_TRY(c, hipStreamWaitEvent(dv.side.st, dv.side.fork, 0));
      cells_st = dv.side.st;
    }
    if (rebuild) {
      if (launch_build_bvh(dv.sc, dv.sb, ss) != 0) return fail(c, ART_E_DEVICE, "collider sort failed");
    } else {
      void* status = nullptr;
      HIP_TRY(c, hipHostGetDevicePointer(&status, dv.relabel_status.p, 0));
      if (!launch_bvh_relabel(p.old_n, p.n, dv.sb, static_cast<uint32_t*>(status), ss))
        return fail(c, ART_E_DEVICE, "collider relabel not applicable");
      HIP_TRY(c, hipGetLastError());
      dv.sc.bvh_levels = bvh_tree_layout(p.n[0] + p.n[1] + p.n[2], dv.sc.bvh_leaf0);
      if (launch_refit_scene(dv.sc, dv.sb, ss) != 0) return fail(c, ART_E_DEVICE, "collider refit failed");
    }
    HIP_TRY(c, hipGetLastError());
    rs.bvh_rebuilt = rebuild ? 1 : 0;
    rs.levels_changed |= dv.sc.bvh_levels != levels_before ? 1 : 0;
    const int cells_rc = launch_build_cells(dv.sc, dv.cb, cells_st);
    if (cells_st != ss) {  // the frames that follow on ss wait for the lists (also after a failed launch)
      HIP_TRY(c, hipEventRecord(dv.side.join, cells_st));
      HIP_TRY(c, hipStreamWaitEvent(ss, dv.side.join, 0));
    }
    if (cells_rc != 0) return fail(c, ART_E_DEVICE, "muffle cell lists failed");
    dv.cells_partial = false;
    cells_rebuilt = true;
    dv.last.valid = false;
    for (int k = 0; k < 3; ++k) dv.sorted.n[k] = p.n[k];
    if (dv.sorted.gen != ~0ull) dv.sorted.gen = c->store.sync_gen;
    dv.sorted.sc = dv.sc;
    if (!lazy) HIP_TRY(c, hipEventRecord(s.done, ss));
    return epoch.record(c);
  }
  if (p.counts_changed) {
    dv.bound = false;  // the sorted copies are sized by count: bind again
    return epoch.record(c);
  }
  set_colliders(dv.sc, v.dec, p.n);  // the bound device-resident scene sees the new snapshot
  set_r_min(dv.sc, c->store.sphere_rmin);
  if (!p.nd) return epoch.record(c);
  // moved colliders: refit the sorted copies and the BVH in place (device only, no H2D)
  if (fused) {
    void* hd = nullptr;  // the pinned image as the device sees it
    HIP_TRY(c, hipHostGetDevicePointer(&hd, h, 0));
    if (!launch_sync_refit(scatter_args(p, hd, v), dv.sc, dv.sb, ss))
      return fail(c, ART_E_DEVICE, "collider sync refit not applicable");
    HIP_TRY(c, hipGetLastError());
  } else if (launch_refit_scene(dv.sc, dv.sb, ss) != 0) {
    (void)hipEventRecord(s.done, ss);
    return fail(c, ART_E_DEVICE, "collider refit failed");
  }
  if (!p.cells_ok) {
    if (launch_build_cells(dv.sc, dv.cb, ss) != 0) return fail(c, ART_E_DEVICE, "muffle cell lists failed");
    dv.cells_partial = false;  // (the full build compacts the entry arena)
    cells_rebuilt = true;
  }
  if (dv.sorted.gen != ~0ull) dv.sorted.gen = c->store.sync_gen;
  if (!lazy) HIP_TRY(c, hipEventRecord(s.done, ss));  // device-path launches wait for the sort too
  return epoch.record(c);
}

// The host bookkeeping of a sync that every device took: dirty marks, counts, the audio_target_id
// histograms, the cell lists' base records, the CPU backend's snapshot and the statistics.
void commit_sync(art_ctx* c, const SyncPlan& p, bool cells_rebuilt, art_collider_resize_stats rs) {
  ColliderStore& s = c->store;
  const int* n = p.n;
  if (c->fr.resident) { c->fr.ns = n[0]; c->fr.na = n[1]; c->fr.no = n[2]; }
  for (int k = 0; k < 3; ++k) {
    auto& K = s.kinds[k];
    for (int i : K.dirty_list)  // O(changes), not O(colliders)
      if ((size_t)i < K.dirty.size()) K.dirty[(size_t)i] = 0;
    K.dirty_list.clear();
    s.synced[k] = n[k];
    // audio_target_id histogram of the synced records: removed tail, then the dirty records
    auto& tids = s.synced_tid[k];
    auto& hist = s.tid_hist[k];
    if (hist.empty()) hist.assign(65536, 0);
    for (size_t i = (size_t)n[k]; i < tids.size(); ++i) hist[(size_t)(tids[i] + 32768)]--;
    const size_t old_n = tids.size();
    tids.resize((size_t)n[k], 0);
    const size_t rs = kRecSize[k], tid_off = kTidOff[k];
    for (int i : p.lists[k]) {
      int16_t v;
      memcpy(&v, K.recs.data() + (size_t)i * rs + tid_off, 2);
      if ((size_t)i < old_n) hist[(size_t)(tids[(size_t)i] + 32768)]--;
      tids[(size_t)i] = v;
      hist[(size_t)(v + 32768)]++;
    }
  }
  if (cells_rebuilt) snapshot_cell_base(c);
  else if (!p.cells_ok) s.cell_base_ok = false;  // the lists (rebuilt at the next bind) no longer hold these records
  if (c->cpu)  // the CPU backend reads the synced snapshot (JobBatch) of each list
    for (int k = 0; k < 3; ++k) s.cpu_recs[k].assign(s.kinds[k].recs.begin(), s.kinds[k].recs.begin() + (size_t)n[k] * kRecSize[k]);
  s.store_synced = true;
  s.last_sync.dirty_records = p.nd;
  s.last_sync.full_prep = (p.counts_changed || p.fresh) ? 1 : 0;
  s.last_sync.reallocated = p.fresh ? 1 : 0;
  s.last_sync.cells_rebuilt = cells_rebuilt ? 1 : 0;
  s.last_sync.bytes_uploaded = p.nd ? p.bytes : 0;
  bool is_bound = !c->devs.empty();
  for (const Device& dv : c->devs) is_bound &= dv.bound;
  rs.kept_bound = (p.resize && is_bound) ? 1 : 0;
  rs.added = p.added;
  rs.removed = p.removed;
  rs.relabelled = 0;  // (of a relabel: read back by art_colliders_last_resize)
  rs.cells_rebuilt = cells_rebuilt ? 1 : 0;
  rs.bytes_uploaded = s.last_sync.bytes_uploaded;
  s.relabel_pending = rs.kept_bound && !rs.bvh_rebuilt;
  s.last_resize = rs;
  // counting frames: the colliders not owned, summed over the targets (count_nonowned). Also after a
  // sync that changed no count: it may have changed owners (art_collider_set, or a target remove with
  // ART_CTX_TARGET_OWNERS_FOLLOW), after a target sync that counted with the records of before.
  if (c->fr.resident && is_bound) {
    c->nonowned.assign(3, 0);
    for (int k = 0; k < 3; ++k) {
      uint64_t owned = 0;
      for (int t = 0; t < c->fr.T && t < 32768; ++t) owned += (uint64_t)s.tid_hist[k][(size_t)t + 32768];
      c->nonowned[(size_t)k] = (uint64_t)c->fr.T * (uint64_t)n[k] - owned;
    }
  }
}

// ------------------------------------------------------------------------------- target half

// The entry arena of a bound scene's cell lists is compacted (every target's lists rebuilt from
// entry 0) by the next target sync once a target has been dropped for capacity, or once the tail
// has passed this fraction of the capacity while the arena holds garbage (a target was rebuilt on
// its own since the last full build; without garbage a compaction gains nothing): 7/8, so that a
// scene whose compact lists fill a fifth of the arena (configs 2-5: 14-33 of 128 entries per pair)
// takes moves of about three times its target count between compactions.
constexpr uint32_t kArenaCompactNum = 7, kArenaCompactDen = 8;
// A sync that moves at least 3/4 of the targets runs the full build: measured at config 2 (T = 4,
// DESIGN.md §3b-targets), a step that relocates 3 of 4 targets costs 0.30 ms against 0.246 ms for
// the full build (the arena fills within a few steps), one that relocates 2 of 4 0.195 ms.
constexpr int kFullBuildNum = 3;  // (of 4)

// What one art_targets_sync does, decided on the host before any device is given work.
struct TargetSyncPlan {
  int n;                   // the list's count
  bool count_changed;      // against the last sync (true for the first)
  std::vector<int> moved;  // dirty positions still in the list, ascending
  // update image: [idx][positions], 16-B aligned sections; only when some device's bound
  // resident-target scene has to follow the moves (image), else no device is given work
  bool image;
  size_t off_idx, off_pos, bytes;
  RingSlot ring;
  // the list's edits since the last sync: every final index's synced index then (-1: new)
  std::vector<int> map;
  int added, removed;
  // A count change that every bound device follows in place (the scene was bound with a target
  // capacity and the count stays within it): the positions that travel, the targets whose lists are
  // built at their final index, and the survivors whose lists move from their old index.
  bool resize;
  std::vector<int> up;       // new, re-indexed or moved in space, ascending
  std::vector<int> sel;      // new, moved in space, or re-indexed onto / from an index that colliders name
  std::vector<int2> moves;   // (old index, new index)
  size_t off_sel, off_mov;   // further sections of the update image: [sel][moves]
};

// Colliders of the bound scene whose audio_target_id is `index` (the store's histogram of the synced
// records, or the one art_scene_bind made of the desc's arrays; without one: as if owned).
bool index_owns_colliders(const art_ctx& c, int index) {
  long long owned = 0;
  for (int k = 0; k < 3; ++k) {
    const std::vector<int>& h = c.fr.resident ? c.store.tid_hist[k] : c.bind_tid_hist[k];
    if (h.empty()) {
      if (!c.fr.resident) return true;
      continue;
    }
    owned += h[(size_t)(index + 32768)];
  }
  return owned > 0;
}

TargetSyncPlan plan_target_sync(art_ctx& c) {
  TargetStore& t = c.targets;
  TargetSyncPlan p;
  p.n = t.count;
  p.count_changed = !t.store_synced || p.n != t.synced;
  for (int i : t.dirty_list)
    if (i < p.n && t.dirty[(size_t)i]) p.moved.push_back(i);
  std::sort(p.moved.begin(), p.moved.end());
  p.moved.erase(std::unique(p.moved.begin(), p.moved.end()), p.moved.end());
  p.map.assign(t.src.begin(), t.src.begin() + p.n);
  p.added = (int)std::count(p.map.begin(), p.map.end(), -1);
  p.removed = (t.store_synced ? t.synced : 0) - (p.n - p.added);
  bool bound = false, follow = true;
  for (const Device& dv : c.devs) {
    bound |= dv.bound;
    follow &= !dv.bound || (dv.sc.T == t.synced && p.n <= dv.cb.tcap);
  }
  const Frame& f = c.fr;
  p.resize = !c.cpu && bound && follow && f.res_targets && p.count_changed && t.store_synced && f.Tc > 0 && p.n >= 1 &&
             p.n <= f.Tc && slot_tables_hold(f, p.n);
  if (p.resize)
    for (int i = 0; i < p.n; ++i) {
      const int s = p.map[(size_t)i];
      const bool fresh = s < 0 || memcmp(t.pos.data() + (size_t)i * 3, t.snap.data() + (size_t)s * 3, 12) != 0;
      if (!fresh && s == i) continue;  // unchanged
      p.up.push_back(i);
      // a block built at index s holds the colliders not owned by s: it is index i's only if no
      // collider names either (cells_geo_kernel drops those of the target's own index)
      if (fresh || index_owns_colliders(c, s) || index_owns_colliders(c, i)) p.sel.push_back(i);
      else p.moves.push_back(make_int2(s, i));
    }
  p.image = !c.cpu && bound && f.res_targets && ((!p.count_changed && !p.moved.empty()) || p.resize);
  const size_t K = p.resize ? p.up.size() : p.moved.size();
  p.off_idx = 0;
  p.off_pos = align_up(K * 4, 16);
  p.off_sel = align_up(p.off_pos + K * 12, 16);
  p.off_mov = align_up(p.off_sel + p.sel.size() * 4, 16);
  // (at least one section's worth: removing the last target changes the count and uploads nothing)
  p.bytes = p.image ? std::max<size_t>(16, align_up(p.off_mov + p.moves.size() * sizeof(int2), 16)) : 0;
  p.ring = p.image ? take_ring_slot(c.store) : RingSlot{-1, 0};
  return p;
}

int stage_target_image(art_ctx* c, const TargetSyncPlan& p) {
  if (int rc = wait_ring_epoch(c, p.ring)) return rc;
  HostBuf& hb = c->store.h_upd[p.ring.slot];
  if (!hb.reserve(p.bytes)) return fail(c, ART_E_NOMEM, "pinned allocation failed");
  uint8_t* h = static_cast<uint8_t*>(hb.p);
  const std::vector<int>& ids = p.resize ? p.up : p.moved;
  for (size_t j = 0; j < ids.size(); ++j) {
    const int i = ids[j];
    memcpy(h + p.off_idx + j * 4, &i, 4);
    memcpy(h + p.off_pos + j * 12, c->targets.pos.data() + (size_t)i * 3, 12);
  }
  if (!p.sel.empty()) memcpy(h + p.off_sel, p.sel.data(), p.sel.size() * 4);
  if (!p.moves.empty()) memcpy(h + p.off_mov, p.moves.data(), p.moves.size() * sizeof(int2));
  return ART_OK;
}

// One device's share of a moved-targets sync, async on the stream it picks (as sync_device): one
// launch scatters the positions from the pinned image into the bound scene's target array, then
// the moved targets' cell lists are rebuilt on their own (or every target's: full). A count change
// that the scene follows (p.resize) takes the first branch.
int sync_device_targets(art_ctx* c, Device& dv, const TargetSyncPlan& p, int& rebuilt, bool& full_rebuild, int& lists_moved) {
  StoreDev& s = dv.store;
  HIP_TRY(c, hipSetDevice(dv.id));
  const hipStream_t ss = (dv.fence.pending && !dv.fence.recorded) ? dv.fence.stream : dv.stream;
  if (ss == dv.stream)
    if (int rc = dv.fence.wait(c, dv.stream)) return rc;
  s.stream = ss;
  EpochMark epoch{s, p.ring, ss};
  if (!dv.bound) return epoch.record(c);
  if (p.resize) {
    // A count change within the scene's capacity: one launch scatters the positions and moves the
    // list blocks of the survivors that may keep theirs (before the builds below, which may write a
    // move's source), then the selected targets' lists are built at their final index, or every
    // target's (the existing rule, with the new count). Nothing is allocated.
    const int K = (int)p.sel.size();
    if (!dv.tsel.reserve((size_t)kMaxTargets * sizeof(int))) return fail(c, ART_E_NOMEM, "device allocation failed");
    const bool lists = dv.cb.cap > 0;
    bool full = false;
    if (lists) {
      if (p.removed > 0) dv.cells_partial = true;  // a removed target's entries are garbage in the arena
      const volatile uint32_t* status = static_cast<const volatile uint32_t*>(dv.cell_status.p);
      const uint32_t tail = status ? status[0] : 0u, dropped = status ? status[1] : 0u;
      full = dropped > 0u || (dv.cells_partial && tail > dv.cb.cap / kArenaCompactDen * kArenaCompactNum) ||
             4 * K >= kFullBuildNum * p.n;
    }
    void* hd = nullptr;  // the pinned image as the device sees it
    HIP_TRY(c, hipHostGetDevicePointer(&hd, c->store.h_upd[p.ring.slot].p, 0));
    const uint8_t* u = static_cast<const uint8_t*>(hd);
    TargetResizeArgs a{};
    a.idx = reinterpret_cast<const int*>(u + p.off_idx); a.pos = reinterpret_cast<const float*>(u + p.off_pos); a.K = (int)p.up.size();
    a.sel = reinterpret_cast<const int*>(u + p.off_sel); a.R = lists && !full ? K : 0;
    a.moves = reinterpret_cast<const int2*>(u + p.off_mov); a.M = lists && !full ? (int)p.moves.size() : 0;
    a.targets = const_cast<float*>(dv.sc.targets); a.tcap = dv.cb.tcap; a.tsel = static_cast<int*>(dv.tsel.p);
    a.start = dv.cb.start; a.far = dv.cb.far; a.ok = dv.cb.ok;
    launch_resize_targets(a, ss);
    HIP_TRY(c, hipGetLastError());
    dv.sc.T = dv.sorted.sc.T = p.n;
    dv.last.valid = false;
    if (lists) {
      const int rc = full ? launch_build_cells(dv.sc, dv.cb, ss)
                          : launch_build_cells_targets(dv.sc, dv.cb, static_cast<const int*>(dv.tsel.p), K, ss);
      if (rc != 0) return fail(c, ART_E_DEVICE, "muffle cell lists failed");
      dv.cells_partial = !full;
      if (full) full_rebuild = true;
      else { rebuilt = K; lists_moved = a.M; }
    }
    if (!s.done) HIP_TRY(c, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    if (ss == dv.stream) HIP_TRY(c, hipEventRecord(s.done, ss));
    return epoch.record(c);
  }
  const int K = (int)p.moved.size();
  if (dv.sc.T != p.n || K > kMaxTargets) return fail(c, ART_E_STATE, "art_targets_sync: the bound scene's targets are not the store's");
  if (!dv.tsel.reserve((size_t)kMaxTargets * sizeof(int))) return fail(c, ART_E_NOMEM, "device allocation failed");
  void* hd = nullptr;  // the pinned image as the device sees it
  HIP_TRY(c, hipHostGetDevicePointer(&hd, c->store.h_upd[p.ring.slot].p, 0));
  const uint8_t* u = static_cast<const uint8_t*>(hd);
  launch_scatter_targets(reinterpret_cast<const int*>(u + p.off_idx), reinterpret_cast<const float*>(u + p.off_pos), K,
                         const_cast<float*>(dv.sc.targets), dv.sc.T, static_cast<int*>(dv.tsel.p), ss);
  HIP_TRY(c, hipGetLastError());
  dv.last.valid = false;  // the device's targets no longer are those of the last host-API upload
  if (dv.cb.cap > 0) {
    // the arena as the device last reported it (not waited for: the device checks the capacity itself)
    const volatile uint32_t* status = static_cast<const volatile uint32_t*>(dv.cell_status.p);
    const uint32_t tail = status ? status[0] : 0u, dropped = status ? status[1] : 0u;
    const bool full = dropped > 0u || (dv.cells_partial && tail > dv.cb.cap / kArenaCompactDen * kArenaCompactNum) ||
                      4 * K >= kFullBuildNum * dv.sc.T;
    const int rc = full ? launch_build_cells(dv.sc, dv.cb, ss)
                        : launch_build_cells_targets(dv.sc, dv.cb, static_cast<const int*>(dv.tsel.p), K, ss);
    if (rc != 0) return fail(c, ART_E_DEVICE, "muffle cell lists failed");
    dv.cells_partial = !full;
    if (full) full_rebuild = true;
    else rebuilt = K;
  }
  if (!s.done) HIP_TRY(c, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  if (ss == dv.stream) HIP_TRY(c, hipEventRecord(s.done, ss));  // launches on other streams wait for it
  return epoch.record(c);
}

void commit_target_sync(art_ctx* c, const TargetSyncPlan& p, int rebuilt, bool full_rebuild, int lists_moved) {
  TargetStore& t = c->targets;
  bool was_bound = false;
  for (const Device& dv : c->devs) was_bound |= dv.bound;
  for (int i : t.dirty_list)
    if ((size_t)i < t.dirty.size()) t.dirty[(size_t)i] = 0;
  t.dirty_list.clear();
  t.synced = p.n;
  t.snap.assign(t.pos.begin(), t.pos.begin() + (size_t)p.n * 3);  // the JobBatch snapshot frames read
  t.store_synced = true;
  if (p.resize) {
    // The host frame follows: only T and the fan layout depend on the count (the batch slot tables do
    // not, slot_tables_hold). make_frame is not called: it reads the caller's direction array.
    Frame& f = c->fr;
    f.T = f.fp.T = p.n;
    art_frame_desc tmp{};
    tmp.ray_count = f.R; tmp.max_hits_per_ray = f.H; tmp.audio_target_count = f.T; tmp.batch_slots = f.TC;
    tmp.stages = f.stages;
    f.L = make_layout(&tmp, f.L.has_hits ? ART_OUT_HIT_RESULTS : 0u);
    c->nonowned.assign(3, 0);  // (counting frames: colliders not owned, summed over the new targets)
    const int n[3] = {f.ns, f.na, f.no};
    for (int k = 0; k < 3; ++k) {
      const std::vector<int>& h = f.resident ? c->store.tid_hist[k] : c->bind_tid_hist[k];
      uint64_t owned = 0;
      for (int i = 0; i < p.n && !h.empty(); ++i) owned += (uint64_t)h[(size_t)i + 32768];
      c->nonowned[(size_t)k] = (uint64_t)p.n * (uint64_t)n[k] - owned;
    }
  } else if (p.count_changed && c->fr.res_targets) {
    for (Device& dv : c->devs) dv.bound = false;  // T is in the frame layout: bind again
  }
  t.last_map = p.map;
  {  // the follow map: this sync's map composed onto the ones since the last mark
    std::vector<int> nf((size_t)p.n);
    for (int i = 0; i < p.n; ++i) {
      const int s = p.map[(size_t)i];
      nf[(size_t)i] = (s >= 0 && (size_t)s < t.follow.size()) ? t.follow[(size_t)s] : -1;
    }
    t.follow.swap(nf);
  }
  for (int i = 0; i < p.n; ++i) t.src[(size_t)i] = i;
  // a full rebuild used the colliders' synced records: they are the lists' base now
  if (full_rebuild && c->fr.resident) snapshot_cell_base(c);
  t.last_sync.dirty_targets = (int32_t)p.moved.size();
  t.last_sync.count_changed = p.count_changed ? 1 : 0;
  t.last_sync.lists_rebuilt = rebuilt;
  t.last_sync.lists_full_rebuild = full_rebuild ? 1 : 0;
  const bool resize_image = p.resize && (!p.up.empty() || !p.sel.empty() || !p.moves.empty());
  t.last_sync.bytes_uploaded = p.resize ? (resize_image ? p.bytes : 0) : p.image ? p.moved.size() * 16 : 0;
  bool is_bound = false;
  for (const Device& dv : c->devs) is_bound |= dv.bound;
  t.last_resize.kept_bound = (was_bound && is_bound && c->fr.res_targets) ? 1 : 0;
  t.last_resize.added = p.added;
  t.last_resize.removed = p.removed;
  t.last_resize.lists_moved = lists_moved;
  t.last_resize.lists_rebuilt = rebuilt;
  t.last_resize.lists_full_rebuild = full_rebuild ? 1 : 0;
  t.last_resize.bytes_uploaded = t.last_sync.bytes_uploaded;
}

}  // namespace

extern "C" {

ART_API int art_target_add(art_ctx* c, const float pos[3], int32_t* out_id) {
  if (!c) return ART_E_INVALID;
  if (!pos) return fail(c, ART_E_INVALID, "art_target_add: position is NULL");
  TargetStore& t = c->targets;
  if (t.count >= 32767) return fail(c, ART_E_UNSUPPORTED, "more than 32767 audio targets (the reference's ids are shorts)");
  t.pos.insert(t.pos.end(), pos, pos + 3);
  t.dirty.push_back(1);
  t.dirty_list.push_back(t.count);
  t.src.push_back(-1);
  if (out_id) *out_id = t.count;  // the index in the list (AudioTargetRT.cs:40-44)
  t.count++;
  return ART_OK;
}

ART_API int art_target_set(art_ctx* c, int32_t id, const float pos[3]) { return art_target_set_many(c, &id, pos, 1); }

ART_API int art_target_set_many(art_ctx* c, const int32_t* ids, const float* positions, int32_t n) {
  if (!c) return ART_E_INVALID;
  if (n < 0 || (n > 0 && (!ids || !positions))) return fail(c, ART_E_INVALID, "art_target_set_many: bad arguments");
  TargetStore& t = c->targets;
  for (int32_t j = 0; j < n; ++j)  // validate first: all or nothing
    if (ids[j] < 0 || ids[j] >= t.count)
      return fail(c, ART_E_INVALID, "art_target_set_many: id %d out of range [0, %d)", ids[j], t.count);
  for (int32_t j = 0; j < n; ++j) {
    const int id = ids[j];
    float* p = t.pos.data() + (size_t)id * 3;
    if (memcmp(p, positions + (size_t)j * 3, 12) == 0) continue;  // the same 12 bytes: nothing moved
    memcpy(p, positions + (size_t)j * 3, 12);
    if (!t.dirty[(size_t)id]) { t.dirty[(size_t)id] = 1; t.dirty_list.push_back(id); }
  }
  return ART_OK;
}

ART_API int art_target_remove_swapback(art_ctx* c, int32_t id) {
  if (!c) return ART_E_INVALID;
  TargetStore& t = c->targets;
  for (int& n : t.last_remove_owners) n = 0;
  if (id < 0 || id >= t.count) return ART_OK;  // skipped, as art_collider_remove_swapback
  const int last = t.count - 1;
  if (id != last) {  // AudioTargetManager.cs:67-73
    memcpy(t.pos.data() + (size_t)id * 3, t.pos.data() + (size_t)last * 3, 12);
    if (!t.dirty[(size_t)id]) { t.dirty[(size_t)id] = 1; t.dirty_list.push_back(id); }
    t.src[(size_t)id] = t.src[(size_t)last];  // the same target, at a new index
    if (c->flags & ART_CTX_TARGET_OWNERS_FOLLOW)
      // swapped.Id.Value = removeIndex (:86) -> AudioCollider.UpdateAudioTargetId (AudioCollider.cs:46-50):
      // the swapped target's colliders take its new index, as art_collider_set would write them
      for (int k = 0; k < 3; ++k) {
        auto& K = c->store.kinds[k];
        const size_t rs = kRecSize[k], tid_off = kTidOff[k];
        const int16_t from = (int16_t)last, to = (int16_t)id;
        for (int i = 0; i < K.count; ++i) {
          uint8_t* tid = K.recs.data() + (size_t)i * rs + tid_off;
          if (memcmp(tid, &from, 2) != 0) continue;
          memcpy(tid, &to, 2);
          if (!K.dirty[(size_t)i]) { K.dirty[(size_t)i] = 1; K.dirty_list.push_back(i); }
          t.last_remove_owners[k]++;
        }
      }
  }
  t.count = last;
  t.pos.resize((size_t)last * 3);
  t.dirty.resize((size_t)last);
  t.src.resize((size_t)last);
  return ART_OK;
}

ART_API int art_target_get(art_ctx* c, int32_t id, float pos[3]) {
  if (!c) return ART_E_INVALID;
  if (!pos) return fail(c, ART_E_INVALID, "art_target_get: position is NULL");
  const TargetStore& t = c->targets;
  if (id < 0 || id >= t.count) return fail(c, ART_E_INVALID, "art_target_get: id %d out of range [0, %d)", id, t.count);
  memcpy(pos, t.pos.data() + (size_t)id * 3, 12);
  return ART_OK;
}

ART_API int art_target_count(art_ctx* c) { return c ? c->targets.count : ART_E_INVALID; }

ART_API int art_target_synced_count(art_ctx* c) { return c ? c->targets.synced : ART_E_INVALID; }

ART_API int art_targets_clear(art_ctx* c) {
  if (!c) return ART_E_INVALID;
  TargetStore& t = c->targets;
  t.pos.clear(); t.dirty.clear(); t.dirty_list.clear(); t.src.clear(); t.count = 0;
  return ART_OK;
}

ART_API int art_targets_last_sync(art_ctx* c, art_target_sync_stats* out) {
  if (!c || !out) return ART_E_INVALID;
  *out = c->targets.last_sync;
  return ART_OK;
}

ART_API int art_targets_sync(art_ctx* c) {
  if (!c) return ART_E_INVALID;
  if (c->inflight) return fail(c, ART_E_STATE, "art_targets_sync: a frame is in flight (sync after art_complete)");
  const TargetSyncPlan p = plan_target_sync(*c);
  int rebuilt = 0, lists_moved = 0;
  bool full_rebuild = false;
  if (p.image) {
    if (int rc = stage_target_image(c, p)) return rc;
    for (Device& dv : c->devs)
      if (int rc = sync_device_targets(c, dv, p, rebuilt, full_rebuild, lists_moved)) return rc;
  }
  commit_target_sync(c, p, rebuilt, full_rebuild, lists_moved);
  return ART_OK;
}

ART_API int art_targets_reserve(art_ctx* c, int32_t capacity) {
  if (!c) return ART_E_INVALID;
  if (capacity < 0) return fail(c, ART_E_INVALID, "art_targets_reserve: negative capacity");
  if (capacity > kMaxTargets) return fail(c, ART_E_UNSUPPORTED, "art_targets_reserve: capacity > %d", kMaxTargets);
  if (c->inflight) return fail(c, ART_E_STATE, "art_targets_reserve: a frame is in flight (reserve after art_complete)");
  c->targets.reserved = capacity;
  return ART_OK;
}

ART_API int art_target_capacity(art_ctx* c) { return c ? c->targets.reserved : ART_E_INVALID; }

ART_API int art_targets_last_resize(art_ctx* c, art_target_resize_stats* out) {
  if (!c || !out) return ART_E_INVALID;
  *out = c->targets.last_resize;
  return ART_OK;
}

ART_API int art_debug_target_sync_map(art_ctx* c, int32_t* src, int32_t cap) {
  if (!c || cap < 0 || (cap > 0 && !src)) return ART_E_INVALID;
  const std::vector<int>& m = c->targets.last_map;
  for (int32_t i = 0; i < cap && (size_t)i < m.size(); ++i) src[i] = m[(size_t)i];
  return c->targets.synced;
}

ART_API int art_target_follow_map(art_ctx* c, int32_t* src, int32_t cap, int32_t* base_count) {
  if (!c || cap < 0 || (cap > 0 && !src)) return ART_E_INVALID;
  const TargetStore& t = c->targets;
  for (int32_t i = 0; i < cap && (size_t)i < t.follow.size(); ++i) src[i] = t.follow[(size_t)i];
  if (base_count) *base_count = t.base_count;
  return t.synced;
}

ART_API int art_target_follow_mark(art_ctx* c) {
  if (!c) return ART_E_INVALID;
  TargetStore& t = c->targets;
  t.follow.resize((size_t)t.synced);
  for (int i = 0; i < t.synced; ++i) t.follow[(size_t)i] = i;
  t.base_count = t.synced;
  return ART_OK;
}

ART_API int art_target_last_remove_owners(art_ctx* c, int32_t out[3]) {
  if (!c || !out) return ART_E_INVALID;
  for (int k = 0; k < 3; ++k) out[k] = c->targets.last_remove_owners[k];
  return ART_OK;
}

ART_API int art_collider_add(art_ctx* c, int32_t kind, const void* rec, int32_t* out_id) {
  if (!c) return ART_E_INVALID;
  if (kind < 0 || kind > 2 || !rec) return fail(c, ART_E_INVALID, "art_collider_add: bad kind or record");
  auto& K = c->store.kinds[kind];
  if (K.count >= (1 << 24)) return fail(c, ART_E_UNSUPPORTED, "more than 2^24 colliders of one kind");
  const size_t rs = kRecSize[kind];
  K.recs.resize((size_t)(K.count + 1) * rs);
  memcpy(K.recs.data() + (size_t)K.count * rs, rec, rs);
  K.dirty.push_back(1);
  K.dirty_list.push_back(K.count);
  if (out_id) *out_id = K.count;  // AudioColliderId = NextBatch.Length before the add
  K.count++;
  c->store.churn_unsynced++;
  return ART_OK;
}

ART_API int art_collider_set(art_ctx* c, int32_t kind, int32_t id, const void* rec) {
  if (!c) return ART_E_INVALID;
  if (kind < 0 || kind > 2 || !rec) return fail(c, ART_E_INVALID, "art_collider_set: bad kind or record");
  auto& K = c->store.kinds[kind];
  if (id < 0 || id >= K.count) return fail(c, ART_E_INVALID, "art_collider_set: id %d out of range [0, %d)", id, K.count);
  const size_t rs = kRecSize[kind];
  memcpy(K.recs.data() + (size_t)id * rs, rec, rs);
  if (!K.dirty[(size_t)id]) { K.dirty[(size_t)id] = 1; K.dirty_list.push_back(id); }
  return ART_OK;
}

ART_API int art_collider_set_many(art_ctx* c, int32_t kind, const int32_t* ids, const void* recs, int32_t n) {
  if (!c) return ART_E_INVALID;
  if (kind < 0 || kind > 2 || n < 0 || (n > 0 && (!ids || !recs)))
    return fail(c, ART_E_INVALID, "art_collider_set_many: bad arguments");
  auto& K = c->store.kinds[kind];
  for (int32_t j = 0; j < n; ++j)  // validate first: all or nothing
    if (ids[j] < 0 || ids[j] >= K.count)
      return fail(c, ART_E_INVALID, "art_collider_set_many: id %d out of range [0, %d)", ids[j], K.count);
  const size_t rs = kRecSize[kind];
  const uint8_t* r = static_cast<const uint8_t*>(recs);
  for (int32_t j = 0; j < n; ++j) {
    const int id = ids[j];
    memcpy(K.recs.data() + (size_t)id * rs, r + (size_t)j * rs, rs);
    if (!K.dirty[(size_t)id]) { K.dirty[(size_t)id] = 1; K.dirty_list.push_back(id); }
  }
  return ART_OK;
}

ART_API int art_collider_remove_swapback(art_ctx* c, int32_t kind, int32_t id) {
  if (!c) return ART_E_INVALID;
  if (kind < 0 || kind > 2) return fail(c, ART_E_INVALID, "art_collider_remove_swapback: bad kind");
  auto& K = c->store.kinds[kind];
  if (id < 0 || id >= K.count) return ART_OK;  // skipped, as AudioColliderManager.SwapRemove (:92-93)
  const size_t rs = kRecSize[kind];
  const int last = K.count - 1;
  if (id != last) {
    memcpy(K.recs.data() + (size_t)id * rs, K.recs.data() + (size_t)last * rs, rs);
    if (!K.dirty[(size_t)id]) { K.dirty[(size_t)id] = 1; K.dirty_list.push_back(id); }
  }
  K.count = last;
  K.recs.resize((size_t)last * rs);
  K.dirty.resize((size_t)last);
  c->store.churn_unsynced++;
  return ART_OK;
}

ART_API int art_collider_get(art_ctx* c, int32_t kind, int32_t id, void* rec) {
  if (!c) return ART_E_INVALID;
  if (kind < 0 || kind > 2 || !rec) return fail(c, ART_E_INVALID, "art_collider_get: bad kind or record");
  const auto& K = c->store.kinds[kind];
  if (id < 0 || id >= K.count) return fail(c, ART_E_INVALID, "art_collider_get: id %d out of range [0, %d)", id, K.count);
  memcpy(rec, K.recs.data() + (size_t)id * kRecSize[kind], kRecSize[kind]);
  return ART_OK;
}

ART_API int art_collider_count(art_ctx* c, int32_t kind) {
  if (!c) return ART_E_INVALID;
  if (kind < 0 || kind > 2) return fail(c, ART_E_INVALID, "art_collider_count: bad kind");
  return c->store.kinds[kind].count;
}

ART_API int art_colliders_clear(art_ctx* c) {
  if (!c) return ART_E_INVALID;
  for (auto& K : c->store.kinds) {
    K.recs.clear(); K.dirty.clear(); K.dirty_list.clear(); K.count = 0;
  }
  return ART_OK;
}

ART_API int art_colliders_last_sync(art_ctx* c, art_collider_sync_stats* out) {
  if (!c || !out) return ART_E_INVALID;
  *out = c->store.last_sync;
  return ART_OK;
}

ART_API int art_colliders_sync(art_ctx* c) {
  if (!c) return ART_E_INVALID;
  if (c->inflight) return fail(c, ART_E_STATE, "art_colliders_sync: a frame is in flight (sync after art_complete)");
  const auto& K = c->store.kinds;
  if ((long long)K[0].count + K[1].count + K[2].count > kMaxColliders)
    return fail(c, ART_E_UNSUPPORTED, "art_colliders_sync: more than %lld colliders", kMaxColliders);
  const SyncPlan p = plan_sync(*c);
  if (int rc = stage_image(c, p)) return rc;
  bool cells_rebuilt = false;
  art_collider_resize_stats rs{};
  for (Device& dv : c->devs)
    if (int rc = sync_device(c, dv, p, cells_rebuilt, rs)) return rc;
  commit_sync(c, p, cells_rebuilt, rs);
  return ART_OK;
}

ART_API int art_colliders_reserve(art_ctx* c, int32_t spheres, int32_t aabbs, int32_t obbs) {
  if (!c) return ART_E_INVALID;
  if (spheres < 0 || aabbs < 0 || obbs < 0) return fail(c, ART_E_INVALID, "art_colliders_reserve: negative capacity");
  if ((long long)spheres + aabbs + obbs > kMaxColliders)
    return fail(c, ART_E_UNSUPPORTED, "art_colliders_reserve: capacity > %lld in total", kMaxColliders);
  if (c->inflight) return fail(c, ART_E_STATE, "art_colliders_reserve: a frame is in flight (reserve after art_complete)");
  c->store.reserved[0] = spheres; c->store.reserved[1] = aabbs; c->store.reserved[2] = obbs;
  return ART_OK;
}

ART_API int art_collider_capacity(art_ctx* c, int32_t kind) {
  if (!c) return ART_E_INVALID;
  if (kind < 0 || kind > 2) return fail(c, ART_E_INVALID, "art_collider_capacity: bad kind");
  return c->store.reserved[kind];
}

ART_API int art_colliders_last_resize(art_ctx* c, art_collider_resize_stats* out) {
  if (!c || !out) return ART_E_INVALID;
  ColliderStore& s = c->store;
  if (s.relabel_pending && !c->devs.empty() && c->devs[0].relabel_status.p) {
    // the relabel kernel's own count, once (waits for that sync's work on the stream it ran on)
    Device& dv = c->devs[0];
    HIP_TRY(c, hipSetDevice(dv.id));
    HIP_TRY(c, hipStreamSynchronize(dv.store.stream));
    s.last_resize.relabelled = (int32_t)*static_cast<const volatile uint32_t*>(dv.relabel_status.p);
    s.relabel_pending = false;
  }
  *out = s.last_resize;
  return ART_OK;
}

}  // extern "C"
