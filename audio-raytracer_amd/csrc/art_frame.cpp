// art_frame.cpp — what a frame is before any device sees it: descriptor validation, the per-fan
// output layout, the direction-coherent ray order, the cell cone table, the staging and device
// buffer layout and the packing of the inputs. Pure host code.
#include <cmath>

#include "art_ctx.hpp"
#include "unity_math.hpp"

namespace art {

int validate_desc(art_ctx* c, const art_frame_desc* d) {
  if (!d) return fail(c, ART_E_INVALID, "desc is NULL");
  if (d->ray_count <= 0 || !d->ray_directions) return fail(c, ART_E_INVALID, "ray_count must be > 0 with directions");
  if (d->ray_count > (1 << 20)) return fail(c, ART_E_UNSUPPORTED, "ray_count > 2^20");
  if (d->audio_target_count <= 0 || !d->audio_target_positions)
    return fail(c, ART_E_INVALID, "audio_target_count must be > 0 (the reference skips frames without targets, AudioRayTracer.cs:95)");
  if (d->audio_target_count > kMaxTargets) return fail(c, ART_E_UNSUPPORTED, "audio_target_count > %d", kMaxTargets);
  if (d->max_hits_per_ray <= 0 || d->max_hits_per_ray > 32)
    return fail(c, ART_E_UNSUPPORTED, "max_hits_per_ray must be in [1, 32] (reference maxBounces <= 25, AudioRayTracer.cs:14)");
  if ((long long)d->ray_count * d->max_hits_per_ray > (1 << 24)) return fail(c, ART_E_UNSUPPORTED, "R*H > 2^24");
  if (d->batch_size <= 0 || d->batch_slots <= 0) return fail(c, ART_E_INVALID, "batch_size and batch_slots must be > 0");
  if (d->aabb_count < 0 || d->obb_count < 0 || d->sphere_count < 0) return fail(c, ART_E_INVALID, "negative collider count");
  if ((long long)d->aabb_count + d->obb_count + d->sphere_count > kMaxColliders)
    return fail(c, ART_E_UNSUPPORTED, "more than %lld colliders", kMaxColliders);
  if ((d->aabb_count && !d->aabb_colliders) || (d->obb_count && !d->obb_colliders) || (d->sphere_count && !d->sphere_colliders))
    return fail(c, ART_E_INVALID, "collider pointer is NULL with a non-zero count");
  if (d->stages & ~ART_STAGE_ALL) return fail(c, ART_E_INVALID, "unknown stage bits");
  if (d->stages & ART_STAGE_DSP_PARAMS) {
    if (!d->dsp) return fail(c, ART_E_INVALID, "ART_STAGE_DSP_PARAMS needs desc->dsp");
    if (!(d->stages & ART_STAGE_REDUCE)) return fail(c, ART_E_INVALID, "ART_STAGE_DSP_PARAMS needs ART_STAGE_REDUCE");
    const art_dsp_desc* p = d->dsp;
    if (!p->reverb_volume_curve.baked || p->reverb_volume_curve.sample_count < 2 || !p->muffle_curve.baked ||
        p->muffle_curve.sample_count < 2)
      return fail(c, ART_E_INVALID, "DSP curves need >= 2 baked samples");
    if (p->reverb_volume_curve.sample_count > 4096 || p->muffle_curve.sample_count > 4096)
      return fail(c, ART_E_UNSUPPORTED, "DSP curves > 4096 samples");
  }
  return ART_OK;
}

FanLayout make_layout(const art_frame_desc* d, uint32_t out_flags) {
  FanLayout L{};
  const size_t T = d->audio_target_count, TC = d->batch_slots, RH = (size_t)d->ray_count * d->max_hits_per_ray;
  L.has_dsp = (d->stages & ART_STAGE_DSP_PARAMS) ? 1 : 0;
  L.has_hits = (out_flags & ART_OUT_HIT_RESULTS) ? 1 : 0;
  size_t off = 0;
  L.settings_off = (uint32_t)off; off = align_up(off + T * sizeof(art_target_settings), 16);
  L.dsp_off = (uint32_t)off; off = align_up(off + (L.has_dsp ? T * sizeof(art_dsp_params) : 0), 16);
  L.muffle_off = (uint32_t)off; off = align_up(off + TC * T * 2, 16);
  L.perm_off = (uint32_t)off; off = align_up(off + TC * T * 4, 16);
  L.echo_off = (uint32_t)off; off = align_up(off + RH * 2, 16);
  L.hit_points_off = (uint32_t)off; off = align_up(off + (L.has_hits ? RH * sizeof(art_half3) : 0), 16);
  L.hit_counts_off = (uint32_t)off; off = align_up(off + (L.has_hits ? (size_t)d->ray_count : 0), 16);
  L.hit_ids_off = (uint32_t)off; off = align_up(off + (L.has_hits ? RH * sizeof(uint32_t) : 0), 16);
  L.stride = (uint32_t)off;
  return L;
}

// Direction-coherent visiting order of the rays: octahedral map of each direction, quantised
// to 16 bits per axis, Morton-interleaved, sorted. 64 consecutive slots then cover a compact
// patch of the sphere, so a wave's echo / muffle rays see the same blockers. Only the lane
// assignment changes; every output is written at the ray's own index.
static void coherent_order(const art_half3* dirs, int R, std::vector<int>& order) {
  std::vector<std::pair<uint32_t, int>> keys((size_t)R);
  for (int i = 0; i < R; ++i) {
    float x = f16tof32(dirs[i].x), y = f16tof32(dirs[i].y), z = f16tof32(dirs[i].z);
    float n = std::fabs(x) + std::fabs(y) + std::fabs(z);
    float u = 0.0f, v = 0.0f;
    if (n > 0.0f && n == n) {
      x /= n; y /= n; z /= n;
      if (z < 0.0f) {
        float ux = (1.0f - std::fabs(y)) * (x >= 0.0f ? 1.0f : -1.0f);
        float vy = (1.0f - std::fabs(x)) * (y >= 0.0f ? 1.0f : -1.0f);
        u = ux; v = vy;
      } else {
        u = x; v = y;
      }
    }
    auto q = [](float a) {
      float t = (a + 1.0f) * 0.5f * 65535.0f;
      t = t < 0.0f ? 0.0f : (t > 65535.0f ? 65535.0f : t);
      return (uint32_t)t;
    };
    auto spread = [](uint32_t a) {
      a &= 0xFFFFu;
      a = (a | (a << 8)) & 0x00FF00FFu;
      a = (a | (a << 4)) & 0x0F0F0F0Fu;
      a = (a | (a << 2)) & 0x33333333u;
      a = (a | (a << 1)) & 0x55555555u;
      return a;
    };
    keys[(size_t)i] = {spread(q(u)) | (spread(q(v)) << 1), i};
  }
  std::stable_sort(keys.begin(), keys.end(), [](const std::pair<uint32_t, int>& a, const std::pair<uint32_t, int>& b) {
    return a.first < b.first;
  });
  order.resize((size_t)R);
  for (int i = 0; i < R; ++i) order[(size_t)i] = keys[(size_t)i].second;
}

// Cube-map direction cells around a target (art_cells.hip): face f = 2 m + (negative), cell (i, j)
// covers u = v[(m+1)%3] / |v[m]| in [-1 + 2i/G, -1 + 2(i+1)/G] and w = v[(m+2)%3] / |v[m]| likewise
// (art_trace_muffle.hpp cube_cell). Each cell's cone: the normalised sum of its corner directions and the
// largest angle to a corner (the farthest point of a convex spherical quadrilateral from an inner
// point), plus 1e-4 rad for the rounding of the cell lookup and of this float table.
ConeTable::ConeTable() {
  for (int f = 0; f < 6; ++f) {
    const int m = f >> 1;
    const double sg = (f & 1) ? -1.0 : 1.0;
    for (int j = 0; j < kCellG; ++j)
      for (int i = 0; i < kCellG; ++i) {
        double corner[4][3], sum[3] = {0, 0, 0};
        for (int k = 0; k < 4; ++k) {
          const double u = -1.0 + 2.0 * (i + (k & 1)) / kCellG, w = -1.0 + 2.0 * (j + (k >> 1)) / kCellG;
          double d[3];
          d[m] = sg; d[(m + 1) % 3] = u; d[(m + 2) % 3] = w;
          const double nrm = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
          for (int a = 0; a < 3; ++a) { corner[k][a] = d[a] / nrm; sum[a] += corner[k][a]; }
        }
        const double sn = std::sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
        for (int a = 0; a < 3; ++a) sum[a] /= sn;
        double alpha = 0.0;
        for (int k = 0; k < 4; ++k) {
          const double c = sum[0] * corner[k][0] + sum[1] * corner[k][1] + sum[2] * corner[k][2];
          alpha = std::max(alpha, std::acos(std::min(1.0, c)));
        }
        alpha += 1e-4;
        CellCone& cc = cone[(f * kCellG + j) * kCellG + i];
        cc.ax = (float)sum[0]; cc.ay = (float)sum[1]; cc.az = (float)sum[2];
        cc.cos_a = (float)std::cos(alpha); cc.sin_a = (float)std::sin(alpha);
        cc.pad0 = cc.pad1 = cc.pad2 = 0.0f;
        alpha_max = std::max(alpha_max, (float)alpha);
      }
  }
}
const ConeTable& cone_table() {
  static const ConeTable t;
  return t;
}

// Frame scalars + batch tables (Audio/AudioRayTracer.cs:161, Jobs/*:63-64, :36-37).
// The permeation batch count (TC * T) / cnt / T equals floor(TC / cnt) for every T >= 1 (nested
// floor division: floor(floor(a T / c) / T) = floor(a / c)), so the slot table does not depend on
// the target count; checked, not assumed, by a count-changing target sync.
bool slot_tables_hold(const Frame& f, int T) {
  if (T < 1) return false;
  for (int start = 0; start < f.R; start += f.bs) {
    const int cnt = std::min(f.bs, f.R - start);
    if ((long long)f.TC * T / cnt / T != (long long)f.TC * f.T / cnt / f.T) return false;
  }
  return true;
}

void make_frame(const art_frame_desc* d, uint32_t out_flags, Frame& f, const int* resident_counts, bool resident_targets,
                int target_capacity, const int* collider_capacity) {
  // the direction-coherent order of the last frame is kept while its directions stay the same
  // (they are set once at init, AudioRayTracer.cs:72-86): a 3-KB compare instead of the sort
  std::vector<int> last_order;
  std::vector<uint8_t> last_dirs;
  last_order.swap(f.ray_order);
  last_dirs.swap(f.order_dirs);
  f = Frame();
  f.R = d->ray_count; f.H = d->max_hits_per_ray; f.T = d->audio_target_count;
  f.TC = d->batch_slots; f.bs = d->batch_size; f.nb = (f.R + f.bs - 1) / f.bs;
  f.ns = d->sphere_count; f.na = d->aabb_count; f.no = d->obb_count;
  f.res_targets = resident_targets;
  if (resident_targets && target_capacity > 0) f.Tc = std::max(target_capacity, f.T);
  if (resident_counts) {
    f.resident = true;
    f.ns = resident_counts[0]; f.na = resident_counts[1]; f.no = resident_counts[2];
    if (collider_capacity && collider_capacity[0] + collider_capacity[1] + collider_capacity[2] > 0)
      for (int k = 0; k < 3; ++k) f.Cc[k] = std::max(collider_capacity[k], resident_counts[k]);
  }
  // collider sections of the staging buffer (empty when the store holds them)
  const size_t sn = f.resident ? 0 : (size_t)f.ns, an = f.resident ? 0 : (size_t)f.na, on = f.resident ? 0 : (size_t)f.no;
  f.stages = d->stages;
  f.L = make_layout(d, out_flags);
  f.slot_batch.assign(f.TC, make_int2(0, 0));
  f.muffle_reset.assign(f.TC, 0);
  for (int start = 0; start < f.R; start += f.bs) {
    const int cnt = std::min(f.bs, f.R - start);
    // raytracer: batchCount = MuffleRayHits.Length / T = TC; batchId = start * TC / R
    const long long rid = (long long)start * f.TC / f.R;
    f.muffle_reset[rid] = 1;
    // permeation: batchCount = PPR.Length / totalRays / T (integer division, Q7)
    const int pbc = (f.TC * f.T) / cnt / f.T;
    const long long pid = (long long)start * pbc / f.R;
    f.slot_batch[pid] = make_int2(start, start + cnt);  // later batches overwrite earlier ones
  }
  if (f.TC == 1) {
    const size_t nb = (size_t)f.R * sizeof(art_half3);
    if (last_order.size() == (size_t)f.R && last_dirs.size() == nb && memcmp(last_dirs.data(), d->ray_directions, nb) == 0) {
      f.ray_order.swap(last_order);
      f.order_dirs.swap(last_dirs);
    } else {
      coherent_order(d->ray_directions, f.R, f.ray_order);
      const uint8_t* b = reinterpret_cast<const uint8_t*>(d->ray_directions);
      f.order_dirs.assign(b, b + nb);
    }
  } else {  // per-batch muffle slots: keep rays in index order
    f.ray_order.resize((size_t)f.R);
    for (int i = 0; i < f.R; ++i) f.ray_order[(size_t)i] = i;
  }
  FrameParams& p = f.fp;
  p.R = f.R; p.H = f.H; p.T = f.T; p.TC = f.TC; p.bs = f.bs; p.nb = f.nb;
  p.max_life = d->max_ray_life; p.max_muffle = d->max_muffle_hit_distance;
  p.muffle_eff = d->muffle_effectiveness; p.perm_strength = d->permeation_strength_per_ray;
  p.perm_eff = d->permeation_effectiveness; p.max_reverb = d->max_reverb_distance;
  p.stages = d->stages;
  if ((d->stages & ART_STAGE_DSP_PARAMS) && d->dsp) {
    const art_dsp_desc* q = d->dsp;
    p.dl_min = q->reverb_dry_level_min; p.dl_max = q->reverb_dry_level_max;
    p.db_min = q->reverb_dry_boost_min; p.db_max = q->reverb_dry_boost_max;
    p.mc_min = q->muffle_cutoff_min; p.mc_max = q->muffle_cutoff_max;
    p.vol_n = q->reverb_volume_curve.sample_count; p.vol_len = q->reverb_volume_curve.length;
    p.muf_n = q->muffle_curve.sample_count; p.muf_len = q->muffle_curve.length;
    p.sample_rate = q->sample_rate;
  }
  // input staging layout (16-B aligned sections)
  size_t o = 0;
  f.off_sph = o; o = align_up(o + sn * sizeof(art_sphere), 16);
  f.off_aabb = o; o = align_up(o + an * sizeof(art_aabb), 16);
  f.off_obb = o; o = align_up(o + on * sizeof(art_obb), 16);
  f.off_tgt = o; o = align_up(o + (size_t)f.tcap() * 12, 16);
  f.off_dirs = o; o = align_up(o + (size_t)f.R * sizeof(art_half3), 16);
  f.off_vol = o; o = align_up(o + (size_t)p.vol_n * 4, 16);
  f.off_muf = o; o = align_up(o + (size_t)p.muf_n * 4, 16);
  f.off_tab = o; o = align_up(o + (size_t)f.TC * sizeof(int2), 16);
  f.off_reset = o; o = align_up(o + (size_t)f.TC, 16);
  f.off_order = o; o = align_up(o + (size_t)f.R * 4, 16);
  f.raw_bytes = o;
  // (by the target and collider capacities: whether the scene has lists, and their room, hold for every count it takes)
  f.cells_cap = (uint32_t)cells_entry_cap(f.tcap(), f.ccap(), f.res_targets);
  Carver sizes{0};
  carve_decoded(sizes, f);
  carve_sort(sizes, f);
  carve_cells(sizes, f);
  f.soa_bytes = sizes.off;
}

DecodedColliders carve_decoded(Carver& c, const Frame& f) {
  const size_t sn = f.resident ? 0 : (size_t)f.ns, an = f.resident ? 0 : (size_t)f.na, on = f.resident ? 0 : (size_t)f.no;
  DecodedColliders d;
  d.sph = c.take<SphereRec>(sn * sizeof(SphereRec));
  d.aabb = c.take<AabbRec>(an * sizeof(AabbRec));
  d.obb = c.take<ObbRec>(on * sizeof(ObbRec));
  d.sphc = c.take<SphereCold>(sn * sizeof(SphereCold));
  d.aabbc = c.take<AabbCold>(an * sizeof(AabbCold));
  d.obbc = c.take<ObbCold>(on * sizeof(ObbCold));
  d.cull = c.take<CullRec>((sn + an + on) * sizeof(CullRec));
  return d;
}

SortBufs carve_sort(Carver& c, const Frame& f) {
  const int ni = f.ccap();  // (the counts' sum, or the reserved capacity they may grow to)
  const size_t n = (size_t)ni;
  SortBufs sb;
  sb.temp_bytes = sort_scene_temp_bytes(ni);
  sb.box = c.take<float>(6 * sizeof(float));
  sb.keys = c.take<uint32_t>(n * 4);
  sb.keys_s = c.take<uint32_t>(n * 4);
  sb.vals = c.take<int>(n * 4);
  sb.perm = c.take<int>(n * 4);
  sb.temp = c.take<void>(sb.temp_bytes);
  sb.bvh = c.take<CullRec>(bvh_node_count(ni) * sizeof(CullRec));
  if (!bvh_node_count(ni)) sb.bvh = nullptr;
  sb.bvh_ref = c.take<uint32_t>(n * 4);
  sb.bvh_pos = c.take<uint32_t>(n * 4);
  sb.bvh_leaf = c.take<float4>(bvh_slot_count(ni) * 64);
  sb.kd = c.take<void>(kd_scratch_bytes(ni));
  if (!kd_scratch_bytes(ni)) sb.kd = nullptr;  // Morton order
  return sb;
}

CellBufs carve_cells(Carver& c, const Frame& f) {
  const size_t T = (size_t)f.tcap();
  const size_t cells = T * kCellStride;  // counters per (target, cell, collider type), with the pads
  CellBufs cb{};
  cb.cap = f.cells_cap;
  cb.tcap = (int)T;
  cb.count = c.take<uint32_t>((cells + 1) * 4);
  cb.start = c.take<uint32_t>((cells + 1) * 4);
  cb.cursor = c.take<uint32_t>((cells + 1) * 4);
  cb.keys = c.take<uint32_t>((size_t)cb.cap * 8);
  cb.ent_s = c.take<uint2>((size_t)cb.cap * 8);
  cb.far = c.take<float>(T * 4);
  cb.ok = c.take<uint32_t>(T * 4);
  cb.tcount = c.take<unsigned long long>(T * 8);
  cb.box = c.take<CullRec>(sizeof(CullRec));
  cb.tail = c.take<uint32_t>(2 * sizeof(uint32_t));
  cb.ent = c.take<uint2>((size_t)cb.cap * 8);
  cb.geo = c.take<void>(cells_geo_bytes((int)T, f.ccap()));
  return cb;
}

void pack_inputs(const art_frame_desc* d, const Frame& f, uint8_t* h) {
  if (!f.resident) {
    if (f.ns) memcpy(h + f.off_sph, d->sphere_colliders, (size_t)f.ns * sizeof(art_sphere));
    if (f.na) memcpy(h + f.off_aabb, d->aabb_colliders, (size_t)f.na * sizeof(art_aabb));
    if (f.no) memcpy(h + f.off_obb, d->obb_colliders, (size_t)f.no * sizeof(art_obb));
  }
  memcpy(h + f.off_tgt, d->audio_target_positions, (size_t)f.T * 12);
  memcpy(h + f.off_dirs, d->ray_directions, (size_t)f.R * sizeof(art_half3));
  if (f.fp.vol_n) memcpy(h + f.off_vol, d->dsp->reverb_volume_curve.baked, (size_t)f.fp.vol_n * 4);
  if (f.fp.muf_n) memcpy(h + f.off_muf, d->dsp->muffle_curve.baked, (size_t)f.fp.muf_n * 4);
  memcpy(h + f.off_tab, f.slot_batch.data(), (size_t)f.TC * sizeof(int2));
  memcpy(h + f.off_reset, f.muffle_reset.data(), (size_t)f.TC);
  memcpy(h + f.off_order, f.ray_order.data(), (size_t)f.R * 4);
}

}  // namespace art
