// art_trace_muffle.hpp — the muffle rays over the targets' direction-cell lists: muffle_kernel, and
// echo_muffle_kernel, the fused plan's joint launch of the echo waves (art_trace_echo.hpp) and the muffle waves.
#pragma once
#include <type_traits>

#include "art_trace_echo.hpp"

namespace art {

// ------------------------------------------------------------------------------------------
// Muffle rays (:150-173, CanRaySeeAudioTarget :405-449). One lane per hit record and target (grid
// y = target; more waves in flight for the latency-bound list walks): the lane's ray from `off` to
// the target (distance < MaxMuffleHitDistance,
// :165-168) is tested against the colliders of its direction cell around the target
// (art_cells.hip: not owned by t, widened bounding sphere on the ray) and stops at its first
// blocker; the wave counts its visible rays into the muffle accumulators with one atomic per
// distinct counter (its records come from one or two 64-ray groups). Any-hit is an OR over the
// colliders, so the cell lists' order is free.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int cube_cell(vec3 v) {
  const float ax = fabsf(v.x), ay = fabsf(v.y), az = fabsf(v.z);
  const int m = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
  const float c[3] = {v.x, v.y, v.z};
  const float n = fabsf(c[m]);
  const float u = c[(m + 1) % 3] / n, w = c[(m + 2) % 3] / n;
  const int i = min(max((int)floorf((u + 1.0f) * (0.5f * kCellG)), 0), kCellG - 1);
  const int j = min(max((int)floorf((w + 1.0f) * (0.5f * kCellG)), 0), kCellG - 1);
  const int f = 2 * m + (c[m] < 0.0f ? 1 : 0);
  return (f * kCellG + j) * kCellG + i;
}

// Sphere idx's test fields (centre, r^2) as one 16-B load (the record's tid is not fetched).
__device__ __forceinline__ SphereRec load_sphere(const DevScene& sc, uint32_t idx) {
  const float4 a = *reinterpret_cast<const float4*>(sc.sph + idx);
  SphereRec r;
  r.cx = a.x; r.cy = a.y; r.cz = a.z; r.r2 = a.w;
  return r;
}

// Exact test of collider `code` (rank << 28 | index, reference records) against segment s.
template <bool OBB>
__device__ __forceinline__ bool muffle_test(const DevScene& sc, const Seg& s, uint32_t code, float maxd, unsigned* nt) {
  const uint32_t type = code >> 28, idx = code & 0x0fffffffu;
  float d;
  bool h;
  if (type == 0) {
    ++nt[0];
    h = sphere_hit_dist(s, load_sphere(sc, idx), d);
  } else if (type == 1 || !OBB) {
    const AabbRec r = sc.aabb[idx];
    ++nt[1];
    h = aabb_test<false>(s, r, d);
  } else {
    ++nt[2];
    h = obb_test_staged(s, sc.obb + idx, d);
  }
  return h && d < maxd;
}

// Every collider not owned by target t, in reference order (lists unavailable or not applicable).
template <bool OBB>
__device__ bool muffle_brute(const DevScene& sc, const Seg& s, float maxd, int t, unsigned* nt) {
  for (int i = 0; i < sc.ns; ++i)
    if (sc.sph[i].tid != t && muffle_test<OBB>(sc, s, (uint32_t)i, maxd, nt)) return true;
  for (int i = 0; i < sc.na; ++i)
    if (sc.aabb[i].tid != t && muffle_test<OBB>(sc, s, (1u << 28) | (uint32_t)i, maxd, nt)) return true;
  for (int i = 0; i < sc.no; ++i)
    if (sc.obb[i].tid != t && muffle_test<true>(sc, s, (2u << 28) | (uint32_t)i, maxd, nt)) return true;
  return false;
}

// The muffle ray of target t from `off` (the hit point stepped back along the ray, :158), tp the
// target's position and maxd = distance(off, tp) (:165, the caller checks maxd < MaxMuffleHitDistance
// :168): true when a collider not owned by t blocks it (CanRaySeeAudioTarget :405-449). The ray
// walks the three type lists of its direction cell around the target, each by ascending near
// bound, stopping at the first entry past the segment; a segment longer than the lists' cell_far,
// a degenerate one or a dropped target tests every collider in reference order. nt / ne / nfb
// count exact tests, list entries and fallback rays (EX).
template <bool EX, bool OBB>
__device__ __forceinline__ bool muffle_blocked(const DevScene& sc, vec3 off, vec3 tp, float maxd, int t, unsigned* nt,
                                               unsigned& ne, unsigned& nfb) {
  bool blocked = false;
  const Seg s = make_seg(off, normalize(tp - off));               // :158-160
  const vec3 v = off - tp;                                        // the ray seen from the target
  const bool lists = sc.cell_ok[t] != 0u && maxd <= sc.cell_far[t] && (v.x != 0.0f || v.y != 0.0f || v.z != 0.0f) &&
                     isfinite(v.x) && isfinite(v.y) && isfinite(v.z);
  if (lists) {
    // the cell's Sphere, AABB and OBB lists in turn (a type-uniform test per loop), each by
    // ascending near bound: a walk stops at the first entry past the segment
    // (st[3] of the target's last cell is its block's first pad start: the target's own end)
    const uint32_t* st = sc.cell_start + (size_t)t * kCellStride + (size_t)cube_cell(v) * 3;
    const float lim = maxd * 1.00001f + 1e-6f;
    const uint32_t klim = near_key(__float_as_uint(lim));
    const uint4 se = make_uint4(st[0], st[1], st[2], st[3]);
    // two entries per step: both records are fetched before either is tested (two dependent
    // fetch chains in flight per lane instead of one); OBB records (64 B) one at a time, which
    // keeps the kernel within 64 VGPRs
    // (4-B entries carry the near key, whose float is a lower bound of the near bound: the per-entry
    // bound check then admits a little more)
    if (sc.cell_compact) {  // (wave-uniform; 8-B entries take the step-by-step walks below)
      // Software-pipelined walks over the 4-B entries: the first entries of all three lists are
      // fetched together as soon as the cell's starts arrive, and each step fetches the next step's
      // entries beside its records, so a walk costs one dependent fetch per step instead of two and
      // the AABB and OBB walks start without an entry fetch of their own. An entry past its list's
      // end reads as 0xffffffff (key 0xffff, beyond every segment) without a fetch.
      auto fetch = [&](uint32_t k, uint32_t e) { return k < e ? sc.cell_ent32[k] : 0xffffffffu; };
      auto nearf_of = [](uint32_t v) { return __uint_as_float(v & 0xffff0000u); };
      // (Measured: keeping the cell's bounds and first entries in one 48-B head per cell, fetched at
      // once, gained nothing further: the entries are already fetched beside one another)
      const uint32_t s0 = fetch(se.x, se.y), s1 = fetch(se.x + 1, se.y);
      const uint32_t a0 = fetch(se.y, se.z), a1 = fetch(se.y + 1, se.z);
      const uint32_t o0 = OBB ? fetch(se.z, se.w) : 0xffffffffu;
      auto walk2 = [&](uint32_t b, uint32_t e, uint32_t c0, uint32_t c1, auto load, auto test) {
        for (uint32_t k = b; k < e; k += 2) {  // c0, c1 = entries k, k + 1
          if ((c0 >> 16) > klim) break;        // this and every later entry lie beyond the segment
          const bool use1 = (c1 >> 16) <= klim;
          const auto r0 = load(c0 & 0xffffu);
          const auto r1 = load((use1 ? c1 : c0) & 0xffffu);
          const uint32_t n0 = fetch(k + 2, e), n1 = fetch(k + 3, e);  // (beside the records)
          if (EX) ne += use1 ? 2u : 1u;
          if (!(nearf_of(c0) > lim) && test(r0)) { blocked = true; break; }
          if (!use1) break;
          if (!(nearf_of(c1) > lim) && test(r1)) { blocked = true; break; }
          c0 = n0; c1 = n1;
        }
      };
      walk2(se.x, se.y, s0, s1, [&](uint32_t idx) { return load_sphere(sc, idx); },
            [&](const SphereRec& r) {
              ++nt[0];
              float d;
              return sphere_hit_dist(s, r, d) && d < maxd;
            });
      if (!blocked)
        walk2(se.y, se.z, a0, a1, [&](uint32_t idx) { return sc.aabb[idx]; },
              [&](const AabbRec& r) {
                ++nt[1];
                float d;
                return aabb_test<false>(s, r, d) && d < maxd;
              });
      if (OBB && !blocked) {  // OBB records (64 B) one at a time, the next entry fetched beside each test
        uint32_t c = o0;
        for (uint32_t k = se.z; k < se.w; ++k) {
          if ((c >> 16) > klim) break;
          if (EX) ++ne;
          const uint32_t n = fetch(k + 1, se.w);
          if (!(nearf_of(c) > lim)) {
            ++nt[2];
            float d;
            if (obb_test_staged(s, sc.obb + (c & 0xffffu), d) && d < maxd) { blocked = true; break; }
          }
          c = n;
        }
      }
    } else {
      auto entry = [&](uint32_t k, uint32_t& idx, uint32_t& key, float& nearf) {  // 8-B entry k: index, near key, near bound
        const uint2 v = sc.cell_ent[k];
        idx = v.x & 0x0fffffffu; key = near_key(v.y); nearf = __uint_as_float(v.y);
      };
      auto walk = [&](uint32_t b, uint32_t e, auto load, auto test, auto pair) {
        uint32_t i0, k0, i1, k1;
        float n0, n1;
        if (!decltype(pair)::value) {
          for (uint32_t k = b; k < e; ++k) {
            entry(k, i0, k0, n0);
            if (k0 > klim) break;  // this and every later entry lie beyond the segment
            if (EX) ++ne;
            if (!(n0 > lim) && test(load(i0))) { blocked = true; break; }
          }
          return;
        }
        for (uint32_t k = b; k < e && !blocked; k += 2) {
          const bool has1 = k + 1 < e;
          entry(k, i0, k0, n0);
          entry(has1 ? k + 1 : k, i1, k1, n1);
          if (k0 > klim) break;             // this and every later entry lie beyond the segment
          const bool use1 = has1 && k1 <= klim;
          const auto r0 = load(i0);
          const auto r1 = load(use1 ? i1 : i0);
          if (EX) ne += use1 ? 2u : 1u;
          if (!(n0 > lim) && test(r0)) { blocked = true; break; }
          if (!use1) break;
          if (!(n1 > lim) && test(r1)) { blocked = true; break; }
        }
      };
      walk(se.x, se.y, [&](uint32_t idx) { return load_sphere(sc, idx); },
           [&](const SphereRec& r) {
             ++nt[0];
             float d;
             return sphere_hit_dist(s, r, d) && d < maxd;
           },
           std::true_type{});
      walk(se.y, se.z, [&](uint32_t idx) { return sc.aabb[idx]; },
           [&](const AabbRec& r) {
             ++nt[1];
             float d;
             return aabb_test<false>(s, r, d) && d < maxd;
           },
           std::true_type{});
      if (OBB)
        walk(se.z, se.w, [&](uint32_t idx) { return sc.obb + idx; },
             [&](const ObbRec* r) {
               ++nt[2];
               float d;
               return obb_test_staged(s, r, d) && d < maxd;
             },
             std::false_type{});
    }
  } else {
    if (EX) ++nfb;
    blocked = muffle_brute<OBB>(sc, s, maxd, t, nt);
  }
  return blocked;
}

// HM: one-hit frames with one batch slot whose path kernel does not run (the fused plan): lane i is
// ray slot i (64-ray group i / 64) and its muffle rays start from the hit record the cast's epilogue
// stored there (fold_path<true>: off and the accumulator base fan * T; TC == 1: batch slot 0).
// i = this lane's hit record / ray slot (i - lane wave-uniform); targets by, by + gy, ...
template <bool EX, bool OBB, bool HM>
__device__ __forceinline__ void muffle_body(const DevScene& sc, const FrameParams& fp, const VisPairs& vp,
                                            const uint32_t* __restrict__ count, uint32_t* __restrict__ acc,
                                            const EchoFromHits& eh, uint32_t i, int by, int gy) {
  const int lane = threadIdx.x & 63;
  // (fixed slots: every bounce's records, kNoRecord marking the slots with no hit)
  const uint32_t n = HM ? (uint32_t)fp.S * (uint32_t)((fp.R + 63) >> 6) * 64u : (vp.fixed ? vp.fixed * (uint32_t)fp.H : ldc(count, 1));
  if (__builtin_amdgcn_readfirstlane(i - (uint32_t)lane) >= n) return;
  bool valid = i < n;
  vec3 off = mk3(0.0f, 0.0f, 0.0f);
  uint32_t dbase = 0u;
  {
    // (compact records: fold_path; the hit record is fetched beside the marker, not after it: a
    // slot without a record holds a stale one, never used. HM: fold_path<true> marks the hit record
    // of a slot without a hit itself, one load per lane)
    const float4 r = vp.hrec[i < n ? i : 0u];
    if (!HM && vp.fixed) valid = valid && vp.out[i].y != kNoRecord;
    off = mk3(r.x, r.y, r.z);
    dbase = __float_as_uint(r.w);
    valid = valid && dbase != kNoRecord;
  }
  unsigned nt[3] = {0u, 0u, 0u}, ne = 0u, nfb = 0u;  // tests, list entries scanned, fallback rays
  for (int t = by; t < fp.T; t += gy) {  // workgroup-uniform
    const vec3 tp = load3(sc.targets, t);
    const float maxd = distance(off, tp);                             // :165
    const bool act = valid && maxd < fp.max_muffle;                   // :168
    bool blocked = false;
    if (act) {
      blocked = muffle_blocked<EX, OBB>(sc, off, tp, maxd, t, nt, ne, nfb);
    }
    const bool vis = act && !blocked;                                 // :171
    unsigned long long mv = __builtin_amdgcn_ballot_w64(vis);
    const uint32_t dest = dbase + (uint32_t)t;
    while (mv) {
      const uint32_t d0 = __builtin_amdgcn_readlane(dest, __builtin_ctzll(mv));
      const unsigned long long eq = __builtin_amdgcn_ballot_w64(vis && dest == d0);
      if (lane == 0) atomicAdd(&acc[d0], (uint32_t)__popcll(eq));
      mv &= ~eq;
    }
  }
  if (EX) {  // lane-tests executed (each lane's own tests; the loop is per lane)
    exec_add_tests(fp.exec + kExecMuffle, nt);
    exec_add(fp.exec + kExecMuffle, kExecCellEntries, wave_sum_u32(ne));
    exec_add(fp.exec + kExecMuffle, kExecMuffleFallback, wave_sum_u32(nfb));
  }
}

// Muffle block b of M ray blocks x mt targets in echo_muffle_kernel (its 4 one-wave workgroups on the
// XCD of block b, as below). Consecutive blocks are
// dispatched to the chip's 8 XCDs in turn (each with its own L2), so when mt divides 8 the XCD of
// block b serves one target, b % 8 % mt: each L2 then holds that target's direction-cell lists
// only, not all targets' (config 2: echo_muffle traffic 12.9 -> 10.8 MB per frame with the 4-B
// entries). The muffle blocks there fill the echo traversal's tails; in the standalone muffle_kernel
// the uneven work per target left XCDs idle (config 5: 171 -> 193 us), so it keeps the plain order.
// Any other shape keeps the plain (b % M, b / M) order. Round 6 (when the group count is a
// multiple of 8): each muffle wave runs on the XCD that traced its 64-ray
// group's echoes (echo_muffle_kernel), so a group's hit records are read from that XCD's L2 and
// each L2 holds every target's lists: echo+muffle config 4 594.5 -> 585.7 us, config 3 88.5 ->
// 87.4, config 2 54.2 -> 53.6 (HBM bytes per launch at config 4 73.3 -> 75.1 MB: the time is not
// set by the traffic).
__device__ __forceinline__ void muffle_block(uint32_t b, uint32_t M, int mt, uint32_t& rb, int& t) {
  if (8 % mt == 0 && ((unsigned long long)M * mt) % 8 == 0) {
    const uint32_t x = b & 7u;
    t = (int)(x % (uint32_t)mt);
    rb = (b >> 3) * (8u / (uint32_t)mt) + x / (uint32_t)mt;
  } else {
    rb = b % M;
    t = (int)(b / M);
  }
}

// 8 waves per SIMD; the counting OBB instantiations at 7, where they need no spills
constexpr int kMuffleObbWaves = 7;  // (the prefetching walks need 72 VGPRs with OBB tests)
template <bool EX, bool OBB, bool HM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(EX && OBB ? 5 : (OBB ? kMuffleObbWaves : (EX ? 7 : 8))))) void muffle_kernel(DevScene sc, FrameParams fp, VisPairs vp,
                                                     const uint32_t* __restrict__ count, uint32_t* __restrict__ acc,
                                                     EchoFromHits eh) {
  muffle_body<EX, OBB, HM>(sc, fp, vp, count, acc, eh, blockIdx.x * 256u + threadIdx.x, (int)blockIdx.y, (int)gridDim.y);
}

// echo_muffle_kernel<false, true>: 7 waves per SIMD (72 VGPRs: the muffle rays' prefetching list
// walks, muffle_blocked) without spills (round 6; 8 waves before them)
constexpr int kEchoMuffleObbWaves = 7;

// One-hit frames with one batch slot and no path kernel (the fused plan): the echo traversal and the muffle
// rays, both from the hit records of the cast's epilogue (fold_path<true>), as one launch on the launch stream: workgroups [0, 4 groups) are
// the echo batches (one wave each) (dispatched first, one round of waves), the rest the muffle blocks (mblocks x
// mt, filling the echo traversal's tails). No side stream, so no fork / join on the frame's path.
// With OBB tests the joint kernel runs at 6 waves per SIMD (5 counting), where it needs no spills.
// One-wave workgroups (4 per 64-ray echo group / 256-ray muffle block), so a muffle wave can start in
// any single wave slot an echo wave frees (with 4-wave workgroups a CU waited for 4 free slots:
// config 3 0.1686 -> 0.1660 ms/step, config 4 1.164 -> 1.149, config 2 even); the 4 waves of a
// group or block stay on one XCD (workgroup b runs on XCD b % 8).
// (The muffle workgroups dispatched before the echo workgroups measured slower: config 2 0.0940 -> 0.1062 ms/step.)
template <bool EX, bool OBB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(OBB ? (EX ? 5 : kEchoMuffleObbWaves) : kEchoWaves<EX, OBB>)))
void echo_muffle_kernel(DevScene sc, FrameParams fp, VisPairs vp, const uint32_t* __restrict__ count,
                        unsigned long long* ex, uint8_t* __restrict__ block, EchoFromHits eh, uint32_t* __restrict__ acc,
                        uint32_t groups, uint32_t mblocks, int mt, EchoLog el) {
  __shared__ uint32_t s_stk[16 * kBvhStack];
  __shared__ __attribute__((aligned(8))) uint16_t s_rec[EX || OBB ? 4 : 16 * 16];
  __shared__ __attribute__((aligned(16))) uint32_t s_deal[ART_REPLAY_DEAL && !EX && !OBB ? kDealWords : 4];
  const uint32_t ne = 4u * groups;  // echo workgroups
  const uint32_t b = blockIdx.x;
  ART_WAVE_TIMER(b < ne ? 1u : 2u);
  // (group or muffle block, wave): a group's 4 waves on one XCD when the counts are multiples of 8,
  // else consecutive
  auto split = [](uint32_t x, uint32_t n, uint32_t& u, int& wv) {
    if (n % 8u == 0u) {
      const uint32_t j = x >> 3;
      u = (j >> 2) * 8u + (x & 7u);
      wv = (int)(j & 3u);
    } else {
      u = x >> 2;
      wv = (int)(x & 3u);
    }
  };
  if (b < ne) {
    if (ART_MEASURE_PARTS == 2) return;
    uint32_t g;
    int w;
    split(b, groups, g, w);
    vis_quad_body<OBB, false, !EX && !OBB, true, EX>(sc, vp, count, EX ? ex : nullptr, g, w, s_stk, nullptr, -1, block, eh, &el, s_rec, s_deal);
    return;
  }
  if (groups % 8u == 0u) {
    // group-local muffle waves (muffle_block's note): the wave of (64-ray group G, target t) runs on the XCD
    // that traced G's echo rays (workgroup index % 8 == G % 8), so each XCD fetches only its own
    // groups' hit records (from its L2) and every target's cell lists
    const uint32_t m = b - ne, x = m & 7u, j = m >> 3;
    const int t = (int)(j % (uint32_t)mt);
    const uint32_t G = (j / (uint32_t)mt) * 8u + x;
    muffle_body<EX, OBB, true>(sc, fp, vp, count, acc, eh, G * 64u + threadIdx.x, t, mt);
    return;
  }
  uint32_t mb, rb;
  int sub, t;
  split(b - ne, mblocks * (uint32_t)mt, mb, sub);
  muffle_block(mb, mblocks, mt, rb, t);  // (groups is a multiple of 8 in the bench shapes)
  muffle_body<EX, OBB, true>(sc, fp, vp, count, acc, eh, rb * 256u + (uint32_t)sub * 64u + threadIdx.x, t, mt);
}

}  // namespace art
