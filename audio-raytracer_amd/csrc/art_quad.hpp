// art_quad.hpp — shared by every quad-per-ray BVH traversal (art_trace.hip, art_permeate.hip): sphere and node tests,
// quad exchanges (DPP), BVH node / leaf loads and tests, work-sharing pairing, counters, the diagnostic builds' device side.
#pragma once
#include "../../include/art_device.h"
#include "art_device_fns.hpp"
#include "art_frame_math.hpp"

namespace art {

constexpr int kNoHit = 0x7fffffff;
constexpr int kNoOwner = 0x7fffffff;  // echo rays skip no collider (AudioTargetId is 16-bit)

// Sphere test split so the common miss costs no branch: the square root and the two IEEE
// divisions run only for lanes whose discriminant is non-negative (RayIntersectsSphere :323-355).
// (A one-division form, selecting the quotient by the numerators' signs, measured 1-3 % slower in
// both traversals: DESIGN.md §4.)
__device__ __forceinline__ bool sphere_hit_dist(const Seg& s, const SphereRec& c, float& dist) {
  vec3 oc = s.o - mk3(c.cx, c.cy, c.cz);
  float b = 2.0f * dot(oc, s.d);
  float cc = dot(oc, oc) - c.r2;
  float disc = b * b - (2.0f * s.a2) * cc;  // 4 * a * c (:329)
  bool hit = false;
  dist = 0.0f;
  if (disc >= 0.0f) {
    float sq = sqrtf(disc);
    float t0 = (-b - sq) / s.a2;
    float t1 = (-b + sq) / s.a2;
    hit = (t0 >= 0.0f) || (t1 >= 0.0f);
    dist = (t0 >= 0.0f) ? t0 : t1;
  }
  return hit;
}

// Executed-work accounting (ART_CTX_COUNT_EXECUTED): one atomic per call from lane 0, off when
// `ex` is null (a uniform branch).
__device__ __forceinline__ void exec_add(unsigned long long* ex, int slot, unsigned long long v) {
  if (ex && v && (threadIdx.x & 63) == 0) atomicAdd(ex + slot, v);
}
// A wave's exact tests by collider type (nt: each lane's counts) into the stage whose counters start at ex,
// and its node visits (4 box tests each).
__device__ __forceinline__ void exec_add_tests(unsigned long long* ex, const unsigned* nt) {
  exec_add(ex, kExecSphere, wave_sum_u32(nt[0]));
  exec_add(ex, kExecAabb, wave_sum_u32(nt[1]));
  exec_add(ex, kExecObb, wave_sum_u32(nt[2]));
}
__device__ __forceinline__ void exec_add_tests(unsigned long long* ex, const unsigned* nt, unsigned nnode) {
  exec_add_tests(ex, nt);
  exec_add(ex, kExecCullBox, 4ull * wave_sum_u32(nnode));
}

#ifdef ART_DIAG
// Diagnostic build only (tools/build_variant.sh diag -DART_DIAG): log2 histograms of per-wave
// cycles (0 nearest, 1 echo) and per-ray traversal steps (2 nearest, 3 echo), printed by
// art_destroy. Each source that traverses (art_trace.hip, art_permeate.hip) has its own copy; the dump adds them.
static __device__ unsigned long long g_diag[4][64];
__device__ __forceinline__ void diag_add(int k, unsigned long long v) {
  atomicAdd(&g_diag[k][v ? 64 - __builtin_clzll(v) : 0], 1ull);
}
#define ART_DIAG_STEP(x) (++(x))
#else
#define ART_DIAG_STEP(x) ((void)0)
#endif

#ifdef ART_WAVE_TIMES
// Diagnostic build only (tools/build_variant.sh wt -DART_WAVE_TIMES): every wave of the nearest and
// echo+muffle launches writes (start | kind << 60, end) in wall-clock ticks and its (block, HW_ID,
// XCC_ID) to its own slot (nearest waves in the first half, echo+muffle waves in the second; no
// atomics, each frame overwrites the previous one's), which art_destroy writes to
// $ART_WAVE_TIMES_OUT (tools/wave_times.py reads it): the launches' wave timelines of the last frame.
constexpr unsigned kWtCap = 1u << 18;
__device__ unsigned long long g_wt[kWtCap][2];
__device__ uint32_t g_wt_id[kWtCap][3];
struct WaveTimer {
  unsigned long long t0;
  unsigned kind;
  __device__ explicit WaveTimer(unsigned k) : t0(wall_clock64()), kind(k) {}
  __device__ ~WaveTimer() {
    const unsigned long long t1 = wall_clock64();
    if ((threadIdx.x & 63) == 0) {
      const unsigned i = (kind ? kWtCap / 2 : 0u) + (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) % (kWtCap / 2);
      g_wt[i][0] = t0 | ((unsigned long long)kind << 60);
      g_wt[i][1] = t1;
      g_wt_id[i][0] = blockIdx.x | (threadIdx.x >> 6) << 24;
      g_wt_id[i][1] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);   // HW_ID
      g_wt_id[i][2] = __builtin_amdgcn_s_getreg((15 << 11) | (0 << 6) | 20);  // XCC_ID
    }
  }
};
#define ART_WAVE_TIMER(k) WaveTimer art_wave_timer_(k)
#else
#define ART_WAVE_TIMER(k) ((void)0)
#endif

// A ray whose direction or origin is non-finite, or whose direction is zero, makes every box test
// inconclusive: its traversals visit every node (the exact tests alone decide).
__device__ __forceinline__ bool force_all(const Seg& s, float om) {
  return !(isfinite(om) && isfinite(s.d.x) && isfinite(s.d.y) && isfinite(s.d.z)) ||
         (s.d.x == 0.0f && s.d.y == 0.0f && s.d.z == 0.0f);
}

// The widened box of a BVH node / collider (margin factor * (scale + om)):
// entry distance of the segment, or false when it misses the box. CAP: the margin is at most the ray's
// `cap` (node_margin_cap, art_frame_math.hpp; +infinity or NaN: no cap). The counting (EX) kernels and the
// permeation loss rays keep the uncapped margin.
__device__ __forceinline__ float capped_margin(float m, float cap) { return __builtin_fminf(m, cap); }
// A ray's cap from the BVH root's stored box (it follows refits and store syncs) and its margin operand.
__device__ __forceinline__ float ray_margin_cap(const DevScene& sc, float om, bool has_obb) {
  const CullRec root = ldc(sc.bvh, 0);
  return node_cap_eval(sc.cap, node_abs_sum(root.lox, root.loy, root.loz, root.hix, root.hiy, root.hiz) + om,
                       has_obb ? kCullObb : kCullBox, 0.0f);
}
template <bool CAP = false>
__device__ __forceinline__ bool node_entry(const Seg& s, const CullRec& r, float om, float& tn, float cap = 0.0f) {
  float m = __builtin_fmaf(r.factor, om, r.fscale);  // factor * (scale + om), fscale = factor * scale
  if (CAP) m = capped_margin(m, cap);
  float tf;
  return slab<false>(s.o.x, s.o.y, s.o.z, s.inv.x, s.inv.y, s.inv.z, r.lox - m, r.loy - m, r.loz - m, r.hix + m, r.hiy + m,
                     r.hiz + m, tn, tf);
}

// ------------------------------------------------------------------------------------------
// Quad-per-ray BVH traversal. The BVH (DevScene::bvh) is a complete 4-ary tree over the Morton
// order of the colliders' bounds, kBvhLeaf colliders per leaf. 4 lanes hold one ray: lane q of the
// quad tests child q of an inner node or slot q of a leaf, the quad exchanges the four results
// through DPP quad permutes, and every lane applies the same near-first ordering, so the ray's
// stack and current node stay identical in the quad (one test per lane per step, 4x the waves of
// one lane per ray).
// Exactness: a collider the ray can hit lies in every ancestor's widened box
// at least 3/4 of the margin inside, so its computed distance is strictly greater than each
// ancestor's computed entry; pruning at entry <= best never drops the winner or a tie, and ties are
// broken by the global order code (type rank << 28 | index), the reference's first minimum over
// Sphere, AABB, OBB order (ShootRayCast :225-280).
// ------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ int quad_perm(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, false); }
constexpr int kQuadXor1 = 1 | (0 << 2) | (3 << 4) | (2 << 6), kQuadXor2 = 2 | (3 << 2) | (0 << 4) | (1 << 6);
constexpr int kQuadRot1 = 1 | (2 << 2) | (3 << 4) | (0 << 6), kQuadRot3 = 3 | (0 << 2) | (1 << 4) | (2 << 6);

// (distance, order) keys (nearest_key) minimum over the quad: one 64-bit compare per DPP round.
__device__ __forceinline__ unsigned long long quad_min_u64(unsigned long long v) {
  {
    const unsigned long long o = ((unsigned long long)(uint32_t)quad_perm<kQuadXor1>((int)(v >> 32)) << 32) |
                                 (uint32_t)quad_perm<kQuadXor1>((int)v);
    v = o < v ? o : v;
  }
  const unsigned long long o = ((unsigned long long)(uint32_t)quad_perm<kQuadXor2>((int)(v >> 32)) << 32) |
                               (uint32_t)quad_perm<kQuadXor2>((int)v);
  return o < v ? o : v;
}

// Quad reductions without ballots (the result lands in every lane of the quad).
__device__ __forceinline__ uint32_t quad_min_u32(uint32_t v) {
  v = min(v, (uint32_t)quad_perm<kQuadXor1>((int)v));
  return min(v, (uint32_t)quad_perm<kQuadXor2>((int)v));
}

// The BVH node and leaf arrays as buffer resources (wave-uniform bases, 32-bit lane offsets).
struct BvhRes {
  __amdgpu_buffer_rsrc_t nodes, leaves;
};
__device__ __forceinline__ BvhRes bvh_res(const DevScene& sc) {
  BvhRes b;
  const int leaf0 = sc.bvh_leaf0, nleaf = 3 * leaf0 + 1, total = leaf0 + nleaf;
  b.nodes = __builtin_amdgcn_make_buffer_rsrc(const_cast<CullRec*>(sc.bvh), 0, total * (int)sizeof(CullRec), 0x00020000);
  b.leaves = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(sc.bvh_leaf), 0, nleaf * kBvhLeaf * 64, 0x00020000);
  return b;
}
__device__ __forceinline__ CullRec load_node(const BvhRes& b, int i) {
  const float4 a = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(b.nodes, i * 32, 0, 0));
  const float4 c = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(b.nodes, i * 32 + 16, 0, 0));
  CullRec r;
  r.lox = a.x; r.loy = a.y; r.loz = a.z; r.fscale = a.w;
  r.hix = c.x; r.hiy = c.y; r.hiz = c.z; r.factor = c.w;
  return r;
}

// Exact test of a 32-B leaf slot already fetched (qa, qb: an OBB-free scene's slot, a sphere or an AABB)
// against segment s; tid = the collider's AudioTargetId.
__device__ __forceinline__ bool leaf_rec_test(const Seg& s, float4 qa, float4 qb, float& dist, int& tid, unsigned* nt) {
  const int cc = __float_as_int(qb.w);
  dist = 0.0f;
  tid = kNoOwner;
  if (cc < 0) return false;  // empty slot past the last collider
  tid = __float_as_int(qb.z);
  if ((cc >> 28) == 0) {
    SphereRec r;
    r.cx = qa.x; r.cy = qa.y; r.cz = qa.z; r.r2 = qa.w;
    ++nt[0];
    return sphere_hit_dist(s, r, dist);
  }
  AabbRec r;
  r.mnx = qa.x; r.mny = qa.y; r.mnz = qa.z; r.mxx = qa.w; r.mxy = qb.x; r.mxz = qb.y;
  ++nt[1];
  return aabb_test<false>(s, r, dist);
}

// Exact test of leaf slot `sl` (64 B: the hot record's test fields and the order code, art_bvh.hip
// bvh_leaf_kernel) against segment s; tid = the collider's AudioTargetId. OBB = false: the scene has
// no OBBs (no rank-2 slots), their test compiles out. PERM: the permeation job's first-hit cast,
// whose OBB test rotates by the inverse of the stored rotation (AudioPermeationJobBatched.cs
// :172-179, App. B Q5), read from the cold record (obbc).
template <bool OBB, bool PERM = false>
__device__ __forceinline__ bool leaf_slot_test(const Seg& s, const BvhRes& br, int slot, int& cc, float& dist, int& tid,
                                               unsigned* nt, const ObbCold* obbc = nullptr) {
  // (slots are 64 B with OBBs in the scene, 32 B without: art_bvh.hip bvh_leaf_kernel)
  auto ld = [&](int k) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(br.leaves, slot * (OBB ? 64 : 32) + 16 * k, 0, 0));
  };
  const float4 qa = ld(0), qb = ld(1);
  cc = __float_as_int(qb.w);
  if (!OBB) return leaf_rec_test(s, qa, qb, dist, tid, nt);
  dist = 0.0f;
  tid = kNoOwner;
  if (cc < 0) return false;  // empty slot past the last collider
  const int t = cc >> 28;
  if (t == 0) {
    SphereRec r;
    r.cx = qa.x; r.cy = qa.y; r.cz = qa.z; r.r2 = qa.w;
    tid = __float_as_int(qb.z);
    ++nt[0];
    return sphere_hit_dist(s, r, dist);
  }
  if (t == 1) {
    AabbRec r;
    r.mnx = qa.x; r.mny = qa.y; r.mnz = qa.z; r.mxx = qa.w; r.mxy = qb.x; r.mxz = qb.y;
    tid = __float_as_int(qb.z);
    ++nt[1];
    return aabb_test<false>(s, r, dist);
  }
  // RayIntersectsOBB (:314-320) in the order that keeps the fewest values live: the rotated
  // direction's reciprocals first (the direction dies), then the rotated origin, and the local
  // bounds fetched only then (same operations as obb_test)
  quat q;
  if (PERM) {
    q = inverse_q(obbc[cc & 0x0fffffff]);
  } else {
    q.x = qa.w; q.y = qb.x; q.z = qb.y; q.w = qb.z;
  }
  const vec3 ld3 = qmul(q, s.d);
  const float ix = recip_exact(ld3.x), iy = recip_exact(ld3.y), iz = recip_exact(ld3.z);
  const vec3 lo = qmul(q, s.o - mk3(qa.x, qa.y, qa.z));
  __builtin_amdgcn_sched_barrier(0);
  const float4 qc = ld(2), qe = ld(3);
  tid = __float_as_int(qe.z);
  ++nt[2];
  float tNear, tFar;
  const bool hit = slab<false>(lo.x, lo.y, lo.z, ix, iy, iz, qc.x, qc.y, qc.z, qc.w, qe.x, qe.y, tNear, tFar);
  dist = tNear > 0.0f ? tNear : tFar;
  return hit;
}

// Population count of a 64-bit lane mask as two 32-bit counts: an int result that compares with
// 32-bit scalar / vector compares (a 64-bit count compares with VALU 64-bit compares).
__device__ __forceinline__ int pop64(unsigned long long x) {
  return __builtin_popcount((uint32_t)x) + __builtin_popcount((uint32_t)(x >> 32));
}

// Work sharing inside a wave (nearest and echo traversals): a wave lasts as long as its longest
// traversal, so a quad whose traversal has ended takes over the bottom entry of a busy quad's
// stack (the largest pending subtree) together with that quad's ray, and traverses it for the
// ray's home quad.
// Idle quads a wave waits for before it shares work (round 4: waiting for 3 in the nearest and 2 in
// the echo traversal runs the steal sequence, 13 lane shuffles and a select, less often; config 2
// nearest 55.4 -> 52.7 us, config 3 74.1 -> 70.5 us, config 5 91.4 -> 89.0 us per bounce).
constexpr int kStealMinIdle = 3, kVisStealMinIdle = 2;
constexpr unsigned long long kQuad0 = 0x1111111111111111ull;  // lane 0 of every quad

// Work sharing's pairing: the quad base lane (l4) of the donor whose rank among the donors equals
// this thief's rank ir. Two cross-lane moves instead of a select-bit search: lane 0 of each robbed
// donor (rank dr) forwards its l4 to lane 4 dr + 1 (ds_permute; every other lane writes into a
// 4k + 2 lane nobody reads), then each lane reads lane 4 ir + 1 (ds_bpermute). Both run in every
// lane of the wave; the caller uses the result in its thieves only.
__device__ __forceinline__ int rank_match(int l4, int qd, bool robbed, int dr, int ir) {
  const int dst = (robbed && qd == 0) ? 4 * dr + 1 : l4 + 2;
  const int tab = __builtin_amdgcn_ds_permute(dst << 2, l4);
  return __builtin_amdgcn_ds_bpermute(((4 * ir + 1) & 63) << 2, tab);
}

// Work sharing's roles of this lane's quad, from the wave's masks (lane 0 of each quad) of the quads with work (act),
// with a spare stack entry (donors; has_work: this one) and without work (idle): the k-th idle quad is a thief and takes
// the k-th donor's stack bottom; src = the lane a thief reads its new ray from (its own otherwise). Every lane takes part.
struct StealRole { bool thief, robbed; int src; };
__device__ __forceinline__ StealRole steal_pairing(int lane, int qd, unsigned long long act, unsigned long long donors,
                                                   unsigned long long idle, bool has_work) {
  // (the quad's lane masks are recomputed here, not hoisted out of the caller's loop: four live VGPRs)
  int l4 = lane & ~3;
  asm volatile("" : "+v"(l4));
  const unsigned long long below = (1ull << l4) - 1ull;
  const int ir = pop64(idle & below), dr = pop64(donors & below);
  StealRole r;
  r.thief = (act >> l4 & 1ull) == 0ull && ir < pop64(donors);
  r.robbed = has_work && dr < pop64(idle);
  const int match = rank_match(l4, qd, r.robbed, dr, ir);  // (every lane takes part)
  r.src = (r.thief ? match : l4) + qd;
  return r;
}
// Segment s of lane src, its derived values too (1/d, 2a: the home's own values, so no divisions).
__device__ __forceinline__ Seg shfl_seg(const Seg& s, int src) {
  Seg r;
  r.o = mk3(__shfl(s.o.x, src), __shfl(s.o.y, src), __shfl(s.o.z, src));
  r.d = mk3(__shfl(s.d.x, src), __shfl(s.d.y, src), __shfl(s.d.z, src));
  r.inv = mk3(__shfl(s.inv.x, src), __shfl(s.inv.y, src), __shfl(s.inv.z, src));
  r.a2 = __shfl(s.a2, src);
  return r;
}

// (distance, order) as one ordered 64-bit key; distances are >= 0 or -0, the two zeros equal
__device__ __forceinline__ unsigned long long nearest_key(float d, int code) {
  return ((unsigned long long)(d == 0.0f ? 0u : __float_as_uint(d)) << 32) | (uint32_t)code;
}

}  // namespace art
