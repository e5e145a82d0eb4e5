// art_trace_echo.hpp — echo visibility: the any-hit quad traversal, the echo rays from the hits or the cast's hit
// records, the bounce-0 leaf replay, vis_kernel (echo_muffle_kernel, art_trace_muffle.hpp, runs the same body).
#pragma once
#if !defined(ART_REPLAY_DEAL) || !defined(ART_MEASURE_PARTS)
#error "include after art_trace.hip's switch block (ART_REPLAY_DEAL, ART_MEASURE_PARTS), here and in art_trace_muffle.hpp"
#endif
#include "art_trace_rays.hpp"

namespace art {

template <bool EX, bool OBB>
constexpr int kEchoWaves = EX ? 6 : (OBB ? 7 : 8);

// ------------------------------------------------------------------------------------------
// Visibility work. The path kernel emits every echo ray and one hit record per hit; visibility
// never feeds back into ray paths (echo :124-145 and muffle :150-173 only write outputs), so the
// verdicts can be computed beside the next bounces. Struct of arrays:
//   seg[2 i], seg[2 i + 1]  echo pair i, emission order: (o.xyz, maxd), (d.xyz, kNoOwner) 32 B, read by
//                           the echo traversal (1/d and dot(d, d) recomputed by make_seg)
//   out[i]                  (u16 index of the echo in the fan blocks, echo half) 8 B: the traversal
//                           stores the half when no collider blocks the ray
//   hrec[j]                 hit record j: (off.xyz, dest) 16 B — the muffle rays' common start
//                           (:158) and the muffle accumulator index (fan * TC + batch slot) * T of
//                           target 0; muffle_kernel casts its T rays
// counts[0] / counts[1] = echo pairs / hit records emitted.
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ void load_pair_seg(const VisPairs& vp, uint32_t i, Seg& s, float& maxd, int& owner) {
  const float4 q0 = vp.seg[2 * (size_t)i], q1 = vp.seg[2 * (size_t)i + 1];
  s = make_seg(mk3(q0.x, q0.y, q0.z), mk3(q1.x, q1.y, q1.z));
  maxd = q0.w;
  owner = __float_as_int(q1.w);
}

// ------------------------------------------------------------------------------------------
// Echo visibility by quad-per-segment BVH traversal. An echo batch is one wave's rays of one fan
// traced back to the fan origin: 64 segments fanning over an eighth of the sphere, whose box and
// cone admit ~10 % of the colliders, so a sweep would spend most of its time there. Per segment
// the BVH visits only the nodes along it: a segment enters a node when its widened box is entered
// before maxd (a blocker's computed distance d < maxd lies strictly after every ancestor's
// entry), 4 lanes per segment (lane q: child q / leaf slot q; the quad agrees through ballots),
// the first blocker ends the segment; a segment no collider blocks stores its echo.
// Work sharing inside the wave: a wave lasts as long as its longest traversal, so a quad whose
// traversal has ended takes over the bottom entry of a busy quad's stack (the largest pending
// subtree) together with that quad's segment, and traverses it for the segment's home quad. The
// subtrees of a segment are then split between quads; any of them finding a blocker marks the home
// blocked (wave-uniform mask), which ends every traversal of that segment. Any-hit is an OR over
// the subtrees, so the split does not change a verdict.
// ------------------------------------------------------------------------------------------
// One-hit frames with one batch slot and hit outputs (H == 1, TC == 1) trace the echo rays straight from the
// nearest hits (HM: `blk` = a 64-ray group), so the traversal does not wait for the path kernel:
// the segment, its output index and value are the path kernel's own expressions (:111, :124-145,
// the zero-distance re-evaluation included), and the traversal stores the echo half or, when a
// collider blocks it, the reset value 0 (the path kernel, running beside it, then leaves those
// slots alone). With H == 1 no later batch resets a ray's slot, so every hit slot is live. (Without hit
// outputs the fused plan runs instead, from the cast's hit records: vis_quad_body's ONE.)
struct EchoFromHits {
  FrameParams fp;
  FanLayout L;
  const float* origins;
  const int* ray_order;
  const int2* pre;
};
// The hit of ray slot r of 64-ray group g from its nearest-hit record, as path_kernel computes it
// (:111, :124, the zero-distance re-evaluation included): false for a slot past the fan's rays
// (slot_ok false) or a miss.
__device__ __forceinline__ bool hit_from_pre(const DevScene& sc, const EchoFromHits& eh, uint32_t g, int r, bool& slot_ok,
                                             int& fan, int& ray, vec3& O, vec3& o, vec3& off, int& type, int& idx) {
  const FrameParams& fp = eh.fp;
  const int nrb = (fp.R + 63) >> 6;
  fan = (int)(g / (uint32_t)nrb);
  const int slot = (int)(g - (uint32_t)fan * nrb) * 64 + r;
  slot_ok = fan < fp.S && slot < fp.R;
  if (!slot_ok) return false;
  ray = eh.ray_order[slot];
  const int2 ph = eh.pre[(size_t)g * 64 + r];
  if (ph.y == kNoHit) return false;  // a miss: no echo ray, no muffle rays
  O = load3(eh.origins, fan);
  const vec3 d = load_dir(sc.dirs, ray);
  const Seg s0 = make_seg(O, d);
  float dist = __int_as_float(ph.x);
  winner_of(sc, s0, ph.y, type, idx, dist);  // as path_kernel
  o = O + d * dist;      // :111
  off = o - d * kEps;    // :124, :158
  return true;
}
__device__ __forceinline__ bool echo_seg_from_hit(const DevScene& sc, const EchoFromHits& eh, uint32_t g, int r, Seg& s,
                                                  float& maxd, uint32_t& out_at, uint16_t& out_val, bool& slot_ok) {
  int fan = 0, ray = 0, type = kNone, idx = 0;
  vec3 O, o, off;
  const bool hit = hit_from_pre(sc, eh, g, r, slot_ok, fan, ray, O, o, off, type, idx);
  out_at = slot_ok ? (uint32_t)(((size_t)fan * eh.L.stride + eh.L.echo_off) / 2) + (uint32_t)ray : 0u;  // ray * H + 0
  if (!hit) return false;
  const float dist0 = distance(O, o);            // :130
  s = make_seg(off, normalize(O - off));
  maxd = dist0;
  out_val = (uint16_t)f32tof16(dist0 * echo_of(sc, type, idx));   // :142-144
  return true;
}

// Any-hit traversal of the wave's 16 segments, one per quad (lane & 3 = the quad's child / slot;
// s_wave = the wave's 16 stacks of kBvhStack entries): true in every lane of a quad whose segment
// no collider blocks (hit and d < maxd, tid != owner: CanRaySeePoint :365-397 / :411-447 with
// owner = the target). `valid` must be quad-uniform; an invalid segment is reported visible.
// Work sharing as in the nearest traversal (a blocker of a shared segment ends every traversal of
// it); nt / nnode accumulate the exact tests and node visits (EX counters).
// CAP (every kernel but the counting ones): the node margins are capped by the segment's node_margin_cap
// (art_frame_math.hpp) for its operand |o|_1 + maxd; a thief takes the home segment's cap along.
template <bool OBB, bool PARK = false, bool CAP = false>
__device__ __forceinline__ bool quad_echo_core(const DevScene& sc, Seg s, float maxd, int owner, bool valid, int lane,
                                               uint32_t* s_wave, unsigned* nt, unsigned& nnode) {
  const int qd = lane & 3, wq = lane >> 2;
  if (sc.bvh_levels == 0) return true;                         // no colliders: nothing blocks
  float om = fabsf(s.o.x) + fabsf(s.o.y) + fabsf(s.o.z) + maxd;
  bool force = force_all(s, om);
  float cap = CAP ? ray_margin_cap(sc, om, OBB) : 0.0f;
  unsigned long long fmk = __builtin_amdgcn_ballot_w64(force);  // (the forced lanes as a lane mask, as in the nearest core)
  const int leaf0 = sc.bvh_leaf0, qshift = lane & ~3;
  const BvhRes br = bvh_res(sc);
  uint32_t* const my = s_wave + wq * kBvhStack;                // entries [bp, sp) pending
  uint32_t wblocked = 0u;                                      // wave-uniform: home quads found blocked
  int home = wq;
  int g = valid ? 0 : -1, sp = 0, bp = 0;
  unsigned nsteps = 0;
  (void)nsteps;
#ifdef ART_DIAG
  const unsigned long long t0 = clock64();
#endif
  auto pop = [&]() {
    const bool has = sp > bp;
    const int t = (int)my[has ? sp - 1 : 0];
    g = has ? t : -1;
    sp = has ? sp - 1 : sp;
    if (sp == bp) sp = bp = 0;
  };
  // PARK: the speculative while-while of the nearest traversal (a quad that reaches a leaf parks it
  // and keeps descending; the wave tests leaves once every quad with work holds one), so a quad
  // that found its leaf early does not idle while the others descend. Any-hit needs every entered
  // leaf tested anyway, so the order changes nothing but the lanes' occupancy. Measured (round 6):
  // the echo half of echo_muffle_kernel config 2 53.0 -> 50.9 us, config 4 495 -> 490 us; the
  // folded frames' vis_kernel (config 5) 440 -> 444 us, so vis_kernel keeps the plain loop.
  int pend = -1;
  for (;;) {
    const unsigned long long act = __builtin_amdgcn_ballot_w64((g & (PARK ? pend : -1)) >= 0) & kQuad0;  // g >= 0 || (PARK && pend >= 0)
    if (!act) break;
    const unsigned long long donors = __builtin_amdgcn_ballot_w64(g >= 0 && sp > bp) & kQuad0, idle = ~act & kQuad0;
    if (donors && pop64(idle) >= kVisStealMinIdle) {  // wave-uniform: the k-th idle quad takes the k-th donor's stack bottom
      const StealRole sr = steal_pairing(lane, qd, act, donors, idle, g >= 0 && sp > bp);
      const bool thief = sr.thief, robbed = sr.robbed; const int src = sr.src;
      const int dbp = __shfl(bp, src), dhome = __shfl(home, src), downer = __shfl(owner, src);
      const Seg ds = shfl_seg(s, src);
      // the segment's other derived values too (|o|_1 + maxd, force: the home's own)
      const float dmaxd = __shfl(maxd, src), dom = __shfl(om, src);
      const int dforce = __shfl((int)force, src);
      float dcap = 0.0f;
      if (CAP) dcap = __shfl(cap, src);
      if (thief) {
        g = (int)s_wave[(src >> 2) * kBvhStack + dbp];
        sp = bp = 0;
        home = dhome; owner = downer; maxd = dmaxd;
        s = ds;
        om = dom;
        cap = dcap;
        force = dforce != 0;
      }
      fmk = __builtin_amdgcn_ballot_w64(force);
      if (robbed && ++bp == sp) sp = bp = 0;
    }
    for (;;) {  // quad-uniform steps
      if (PARK) {
        if (g >= leaf0 && pend < 0) { pend = g; pop(); }
        // (after the park, a quad with no parked leaf and a node holds an inner node)
        if (__builtin_amdgcn_ballot_w64((pend & ~g) < 0) == 0ull) break;  // pend < 0 && g >= 0, one compare
        if (!(g >= 0 && g < leaf0)) continue;
      } else if (!(g >= 0 && g < leaf0)) {
        break;
      }
      const int c0 = 4 * g + 1;
      if (qd == 0) ++nnode;
      ART_DIAG_STEP(nsteps);
      const CullRec r = load_node(br, c0 + qd);
      float tn;
      const bool h = node_entry<CAP>(s, r, om, tn, cap);
      // the entered lanes as a mask of scalar ANDs / ORs of single-compare ballots (a ballot of the
      // combined flag would round-trip it through a 0/1 VGPR); empty nodes: art_bvh.hip cull_stored
      const unsigned long long em = fmk | (__builtin_amdgcn_ballot_w64(h) & __builtin_amdgcn_ballot_w64(tn <= maxd));
      const bool enter = __builtin_amdgcn_inverse_ballot_w64(em);
      const uint32_t eb = (uint32_t)(em >> qshift) & 0xFu;
      if (eb) {
        const int first = __builtin_ctz(eb);
        const uint32_t rest = eb & (eb - 1u);
        if (enter && qd != first) my[sp + __popc(rest & ((1u << qd) - 1u))] = (uint32_t)(c0 + qd);
        sp += __popc(rest);
        g = c0 + first;
      } else {
        pop();
      }
    }
    bool hit_quad = false;
    const int leaf = PARK ? pend : g;
    if (leaf >= leaf0) {
      ART_DIAG_STEP(nsteps);
      int cc, tid;
      float d;
      const bool hh = leaf_slot_test<OBB>(s, br, (leaf - leaf0) * kBvhLeaf + qd, cc, d, tid, nt);
      const bool blk_here = hh && d < maxd && tid != owner;  // :373-394, :411-447
      hit_quad = ((uint32_t)(__builtin_amdgcn_ballot_w64(blk_here) >> qshift) & 0xFu) != 0u;
      if (!PARK && !hit_quad) pop();
    }
    pend = -1;
    for (unsigned long long bq = __builtin_amdgcn_ballot_w64(hit_quad) & kQuad0; bq; bq &= bq - 1ull)
      wblocked |= 1u << __builtin_amdgcn_readlane(home, __builtin_ctzll(bq));
    if ((wblocked >> home) & 1u) { g = -1; sp = bp = 0; }  // the segment is decided: every quad on it stops
  }
#ifdef ART_DIAG
  if (qd == 0 && valid) diag_add(3, nsteps);
  if (lane == 0) diag_add(1, clock64() - t0);
#endif
  return !((wblocked >> wq) & 1u);
}

// ART_REPLAY_DEAL 1: the replayed leaf tests of the wave's 16 rays are dealt evenly over its 16
// quads (quad q tests items q, q + 16, ... of the flattened (ray, leaf) list, segment and maxd of the
// item's ray from LDS): ceil(sum n / 16) steps instead of max n, no early exit. A verdict is an OR
// over a ray's leaves, so the order changes no result. s_deal: 16 segments (3 float4) and the item
// list (16 * kLogK u32) in LDS. 0: each quad tests its own record, to its first blocker.
// Measured: config 2 0.0940 -> 0.0905 ms/step with the dealing on.
constexpr int kDealWords = 16 * 12 + 16 * kLogK;
// REPLAY (ONE, echo_muffle_kernel's non-counting OBB-free instantiation): a quad whose ray has a leaf record
// (EchoLog, el.rec set: the nearest cast logged this frame) tests the record's leaves against the
// echo segment, 4 slots per step, to its first blocker; the rays marked kLogTraverse run
// quad_echo_core in the same wave, where the replaying quads are idle quads that share their work.
// s_rec: the wave's 16 records in LDS.
// ONE (echo_muffle_kernel): the one-hit fused plan's records at fixed slots (fold_path<true>); the cast
// stored each hit's echo half already, so a quad stores only a blocked echo's reset 0.
// EX: the caller is a counting kernel (its traversal keeps the uncapped node margins, quad_echo_core's CAP off).
template <bool OBB, bool HM, bool REPLAY = false, bool ONE = false, bool EX = false>
__device__ __forceinline__ void vis_quad_body(const DevScene& sc, const VisPairs& vp, const uint32_t* count,
                                              unsigned long long* ex, uint32_t blk, int w, uint32_t* s_wave,
                                              const uint32_t* ecnt, int bounce, uint8_t* block, const EchoFromHits& eh,
                                              const EchoLog* el = nullptr, uint16_t* s_rec = nullptr,
                                              uint32_t* s_deal = nullptr) {
  const int lane = threadIdx.x & 63, qd = lane & 3;
  const int wq = lane >> 2, slot = w * 16 + wq;                // segment of the block's 64-pair batch
  if (sc.bvh_levels == 0 && !HM) return;                       // no colliders: nothing blocks (ONE: and no echo ray to count)
  bool valid;
  uint32_t p = 0u, out_at = 0u;
  uint16_t out_val = 0;
  Seg s;
  float maxd = 0.0f;
  int owner = kNoOwner;
  s.o = s.d = s.inv = mk3(0.0f, 0.0f, 0.0f);
  s.a2 = 0.0f;
  uint2 lrec = make_uint2(kLogTraverse, 0u);  // this lane's quarter of the ray's leaf record, fetched beside the hit
  if constexpr (REPLAY) {
    if (el->rec) lrec = reinterpret_cast<const uint2*>(el->rec)[((size_t)blk * 64 + (uint32_t)slot) * 4 + qd];
  }
  if (HM) {
    bool slot_ok;
    valid = echo_seg_from_hit(sc, eh, blk, slot, s, maxd, out_at, out_val, slot_ok);
    if (!__any(valid)) return;
  } else {
    if (ONE || vp.fixed) {  // bounce `bounce`'s compact records at fixed slots: 64-slot group blk (fold_path)
      p = (ONE ? 0u : (uint32_t)bounce * vp.fixed) + blk * 64u + (uint32_t)slot;
      const uint2 ov = vp.out[p];
      float4 hr = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (ONE) hr = vp.hrec[p];  // (beside the marker, not after it: a slot without a hit holds its own marker)
      valid = ov.y != kNoRecord;
      // (the fused plan runs no path kernel: the echo rays are counted here)
      if (ONE && ex) exec_add(ex, kExecEchoPairs, (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(valid) & kQuad0));
      if (!__any(valid)) return;
      if (valid) {  // the segment as fold_path's reference expressions give it: off -> fan origin (:124-130)
        const FrameParams& fp = eh.fp;
        const int nrb = (fp.R + 63) >> 6;
        const int fan = (int)(blk / (uint32_t)nrb);
        if (!ONE) hr = vp.hrec[p];
        const vec3 off = mk3(hr.x, hr.y, hr.z), O = load3(eh.origins, fan);
        s = make_seg(off, normalize(O - off));
        maxd = __uint_as_float(ov.x);
        owner = kNoOwner;
        if (!ONE) {
          const int ray = eh.ray_order[(int)(blk - (uint32_t)fan * nrb) * 64 + slot];
          out_at = (uint32_t)(((size_t)fan * eh.L.stride + eh.L.echo_off) / 2) + (uint32_t)(ray * fp.H + bounce);
          out_val = (uint16_t)(ov.y & 0xffffu);
        }
      }
    } else {
      // all echo pairs, or (bounce >= 0) those bounce `bounce` emitted: they follow the earlier bounces'
      uint32_t start = 0u, n;
      if (bounce < 0) {
        n = ldc(count, 0);
      } else {
        for (int j = 0; j < bounce; ++j) start += ldc(ecnt, j);
        n = start + ldc(ecnt, bounce);
      }
      const uint32_t base = start + blk * 64u;
      if (base + (uint32_t)(w * 16) >= n) return;                // this wave's 16 segments are past the emitted pairs
      valid = base + (uint32_t)slot < n;
      p = valid ? base + (uint32_t)slot : base;
      if (valid) load_pair_seg(vp, p, s, maxd, owner);
    }
  }
  unsigned nt[3] = {0u, 0u, 0u}, nnode = 0;
  bool replayed = false, blocked = false;  // quad-uniform
  if constexpr (REPLAY) {
    if (el->rec) {  // (wave-uniform)
      reinterpret_cast<uint2*>(s_rec)[wq * 4 + qd] = lrec;
      // (lanes read each other's LDS entries: order the writes before the reads, as permeate_bvh_kernel does)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();
      const uint32_t n = s_rec[wq * 16];
      replayed = valid && n <= (uint32_t)kLogK;  // (kLogTraverse: the echo traversal below)
      const BvhRes br = bvh_res(sc);
      const int qshift = lane & ~3;
#if ART_REPLAY_DEAL
      float4* const s_seg = reinterpret_cast<float4*>(s_deal);  // [16][3]: (o, maxd), (d, a2), (1/d, owner)
      uint32_t* const s_item = s_deal + 16 * 12;                // ray << 16 | leaf id, the rays' leaves back to back
      const uint32_t nq = replayed ? n : 0u;
      uint32_t inc = nq;  // inclusive prefix sums of the quads' leaf counts (a quad's lanes agree)
      for (int sft = 4; sft < 64; sft <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, sft);
        if (lane >= sft) inc += up;
      }
      const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63), start = inc - nq;
      if (qd == 0) s_seg[wq * 3] = make_float4(s.o.x, s.o.y, s.o.z, maxd);
      if (qd == 1) s_seg[wq * 3 + 1] = make_float4(s.d.x, s.d.y, s.d.z, s.a2);
      if (qd == 2) s_seg[wq * 3 + 2] = make_float4(s.inv.x, s.inv.y, s.inv.z, __int_as_float(owner));
      for (uint32_t j = (uint32_t)qd; j < nq; j += 4u) s_item[start + j] = ((uint32_t)wq << 16) | s_rec[wq * 16 + 1 + j];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();
      // item k's leaf slot of this lane (32 B: OBB-free scenes), fetched one step ahead of its test
      auto fetch = [&](uint32_t k, uint32_t& ray, float4& qa, float4& qb) {
        const uint32_t it = s_item[k];
        ray = it >> 16;
        const int at = ((int)(it & 0xffffu) * kBvhLeaf + qd) * 32;
        qa = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(br.leaves, at, 0, 0));
        qb = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(br.leaves, at + 16, 0, 0));
      };
      float4 na = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nb = na;
      uint32_t nray = 0u, wblk = 0u;  // wblk: wave-uniform mask of the rays found blocked
      bool on = (uint32_t)wq < total;
      if (on) fetch((uint32_t)wq, nray, na, nb);
      for (uint32_t base = 0u; base < total; base += 16u) {  // (wave-uniform)
        const float4 qa = na, qb = nb;
        const uint32_t ray = nray;
        const bool more = base + 16u + (uint32_t)wq < total;
        if (more) fetch(base + 16u + (uint32_t)wq, nray, na, nb);
        bool blk_here = false;
        if (on) {
          const float4 a = s_seg[ray * 3u], b = s_seg[ray * 3u + 1u], c = s_seg[ray * 3u + 2u];
          Seg sr;
          sr.o = mk3(a.x, a.y, a.z); sr.d = mk3(b.x, b.y, b.z); sr.inv = mk3(c.x, c.y, c.z); sr.a2 = b.w;
          int tid;
          float d;
          const bool hh = leaf_rec_test(sr, qa, qb, d, tid, nt);
          blk_here = hh && d < a.w && tid != __float_as_int(c.w);  // :373-394, quad_echo_core's test
        }
        const bool hit_quad = ((uint32_t)(__builtin_amdgcn_ballot_w64(blk_here) >> qshift) & 0xFu) != 0u;
        for (unsigned long long bq = __builtin_amdgcn_ballot_w64(hit_quad) & kQuad0; bq; bq &= bq - 1ull)
          wblk |= 1u << __builtin_amdgcn_readlane((int)ray, __builtin_ctzll(bq));
        on = more;
      }
      blocked = ((wblk >> wq) & 1u) != 0u;
#else
      // leaf j's slot of this lane (32 B: OBB-free scenes), fetched one step ahead of its test
      auto fetch = [&](uint32_t j, float4& qa, float4& qb) {
        const int at = ((int)s_rec[wq * 16 + 1 + j] * kBvhLeaf + qd) * 32;
        qa = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(br.leaves, at, 0, 0));
        qb = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(br.leaves, at + 16, 0, 0));
      };
      float4 na = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nb = na;
      bool on = replayed && n > 0u;
      if (on) fetch(0u, na, nb);
      for (uint32_t j = 0; __any(on); ++j) {
        const float4 qa = na, qb = nb;
        const bool more = on && j + 1u < n;
        if (more) fetch(j + 1u, na, nb);
        bool blk_here = false;
        if (on) {
          int tid;
          float d;
          const bool hh = leaf_rec_test(s, qa, qb, d, tid, nt);
          blk_here = hh && d < maxd && tid != owner;  // :373-394, quad_echo_core's test
        }
        blocked = blocked || ((uint32_t)(__builtin_amdgcn_ballot_w64(blk_here) >> qshift) & 0xFu) != 0u;
        on = more && !blocked;
      }
#endif
    }
    if (el->count) {
      const uint32_t nr = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(replayed) & kQuad0);
      const uint32_t nv = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(valid && !replayed) & kQuad0);
      if (lane == 0) atomicAdd(el->count + (blockIdx.x & (kEchoCountSlots - 1)), (unsigned long long)nr | ((unsigned long long)nv << 32));
    }
  }
  bool visible = quad_echo_core<OBB, HM || ONE, !EX>(sc, s, maxd, owner, valid && !replayed, lane, s_wave, nt, nnode);
  if (REPLAY && replayed) visible = !blocked;
  if (HM) {
    if (valid && qd == 0) reinterpret_cast<uint16_t*>(block)[out_at] = visible ? out_val : (uint16_t)0;  // :76, :142-144
  } else if (ONE) {
    if (valid && !visible && qd == 0) {  // a blocked echo: the reset value over the cast's provisional half (:76)
      const FrameParams& fp = eh.fp;
      const int nrb = (fp.R + 63) >> 6;
      const int fan = (int)(blk / (uint32_t)nrb);
      const int ray = eh.ray_order[(int)(blk - (uint32_t)fan * nrb) * 64 + slot];
      reinterpret_cast<uint16_t*>(block)[(uint32_t)(((size_t)fan * eh.L.stride + eh.L.echo_off) / 2) + (uint32_t)ray] = 0;
    }
  } else if (vp.fixed) {
    if (valid && visible && qd == 0) reinterpret_cast<uint16_t*>(block)[out_at] = out_val;  // :142-144
  } else if (valid && visible && qd == 0) {  // visible: the echo is stored (:142-144)
    const uint2 o = vp.out[p];
    reinterpret_cast<uint16_t*>(block)[o.x] = (uint16_t)(o.y & 0xffffu);
  }
  if (ex) exec_add_tests(ex + kExecEcho, nt, nnode);
}

// The echo traversal: one 64-pair batch per workgroup. EX: count the executed tests (fp.exec);
// without it the counters compile out. 8 waves per SIMD.
template <bool EX, bool OBB, bool HM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kEchoWaves<EX, OBB>)))
void vis_kernel(DevScene sc, VisPairs vp, const uint32_t* __restrict__ count, unsigned long long* ex,
                const uint32_t* __restrict__ ecnt, int bounce, uint8_t* __restrict__ block, EchoFromHits eh) {
  __shared__ uint32_t s_stk[64 * kBvhStack];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  vis_quad_body<OBB, HM, false, false, EX>(sc, vp, count, EX ? ex : nullptr, blockIdx.x, w, s_stk + w * 16 * kBvhStack, ecnt, bounce, block, eh);
}

}  // namespace art
