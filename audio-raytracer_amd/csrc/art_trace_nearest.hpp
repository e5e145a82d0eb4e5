// art_trace_nearest.hpp — the nearest-hit cast: node table, near-first descent, quad_nearest_core (also the
// permeation job's first-hit cast, art_permeate.hip), the folded path epilogue, nearest_first_kernel.
#pragma once
#include <cfloat>
#include <type_traits>

#include "art_trace_rays.hpp"

namespace art {

// Shared-origin node table (TAB kernels): every ray of a workgroup starts at the fan origin O, so a
// node's widened box relative to O, (lo - m) - O and (hi + m) - O with m = factor * (scale + |O|_1),
// capped per ray as node_entry's (CAP: every kernel but the counting ones), is the same for all of
// them. Built once per workgroup in LDS (node_table_build), the node test is
// then the slab's multiplies and min / max on the very operands node_entry computes (bit-identical:
// the same operations in the same order, DESIGN.md §5 item 8 unchanged). Up to kTabNodes nodes
// (the BVH of <= 4096 colliders: 1365 nodes, 32 KB).
constexpr int kTabNodes = 1365;
struct NodeTab {
  float4 a[kTabNodes];  // (lo.x, lo.y, lo.z, hi.x) relative to O, widened
  float2 b[kTabNodes];  // (hi.y, hi.z)
};
template <bool CAP, bool OBB>
__device__ __forceinline__ void node_table_build(const DevScene& sc, vec3 O, NodeTab* tab) {
  const BvhRes br = bvh_res(sc);
  const int nn = sc.bvh_leaf0 + 3 * sc.bvh_leaf0 + 1;
  const float om = fabsf(O.x) + fabsf(O.y) + fabsf(O.z);  // quad_nearest_core's om of every ray at O
  const float cap = CAP ? ray_margin_cap(sc, om, OBB) : 0.0f;  // (one value per workgroup: nothing per step)
  for (int i = (int)threadIdx.x; i < nn; i += (int)blockDim.x) {
    const CullRec r = load_node(br, i);
    float m = __builtin_fmaf(r.factor, om, r.fscale);  // node_entry's margin
    if (CAP) m = capped_margin(m, cap);
    tab->a[i] = make_float4((r.lox - m) - O.x, (r.loy - m) - O.y, (r.loz - m) - O.z, (r.hix + m) - O.x);
    tab->b[i] = make_float2((r.hiy + m) - O.y, (r.hiz + m) - O.z);
  }
}
__device__ __forceinline__ bool node_entry_tab(const Seg& s, const NodeTab* tab, int i, float& tn) {
  const float4 a = tab->a[i];
  const float2 b = tab->b[i];
  const float t0x = a.x * s.inv.x, t0y = a.y * s.inv.y, t0z = a.z * s.inv.z;  // slab<false>'s (mn - o) * inv
  const float t1x = a.w * s.inv.x, t1y = b.x * s.inv.y, t1z = b.y * s.inv.z;
  tn = fmax_ieee(fmax_ieee(fmin_ieee(t0x, t1x), fmin_ieee(t0y, t1y)), fmin_ieee(t0z, t1z));
  const float tf = fmin_ieee(fmin_ieee(fmax_ieee(t0x, t1x), fmax_ieee(t0y, t1y)), fmax_ieee(t0z, t1z));
  return !(tn > tf || tf < 0.0f);
}

// One inner step of a quad traversal (lane qd holds child c0 + qd; `enter` / entry `en` its
// verdict): descend into the nearest entered child and push the other entered children far first
// onto the ray's stack, or pop when none is entered. Near-first order by rank: each lane's key is
// its child's entry bits with the child index in the two low bits (unique in the quad; non-entered
// children 0xffffffff), its rank the number of smaller keys among the quad's other three (three DPP
// rotations); the quad minimum of the keys names the nearest child, 1 + the largest rank of an
// entered lane counts them. No ballots: every value is a quad DPP reduction (measured 3 % faster in
// the nearest traversal; the echo any-hit keeps its ballot form, index order, which measured 6 %
// faster there than this near-first form).
__device__ __forceinline__ void quad_descend(bool enter, float en, bool force, int qd, int c0, uint32_t* my, int& g,
                                             int& sp, int& bp) {
  const uint32_t key = enter ? (((uint32_t)__float_as_int(en) & (force ? 0u : ~3u)) | (uint32_t)qd) : 0xffffffffu;
  const uint32_t k1 = (uint32_t)quad_perm<kQuadRot1>((int)key), k2 = (uint32_t)quad_perm<kQuadXor2>((int)key),
                 k3 = (uint32_t)quad_perm<kQuadRot3>((int)key);
  const int rank = (int)(k1 < key) + (int)(k2 < key) + (int)(k3 < key);
  const uint32_t kmin = min(min(key, k1), min(k2, k3));
  // entered children (one ballot of the key itself: an entered key is at most 0x7f800003, en >= 0)
  const int nent = __popc((uint32_t)(__builtin_amdgcn_ballot_w64(key != 0xffffffffu) >> (__lane_id() & ~3)) & 0xFu);
  const int spn = sp + nent - 1;  // the stack pointer after the push (one add shared by both uses)
  if (enter && rank > 0) my[spn - rank] = (uint32_t)(c0 + qd);
  if (nent) {
    g = c0 + (int)(kmin & 3u);
    sp = spn;
  } else {  // branch-free pop: the stack slot is read unconditionally (clamped), -1 when empty
    const int t = (int)my[sp > 0 ? sp - 1 : 0];
    g = sp > 0 ? t : -1;
    sp = sp > 0 ? sp - 1 : 0;
    if (sp == bp) sp = bp = 0;  // the entries below bp were taken
  }
}

// Waves per SIMD of the traversal kernels: 8 (64 VGPRs). Register spills inside the divergent
// traversal loops hung a fused kernel once, so the counting instantiations and
// the echo traversal's OBB one run at the occupancy that holds them without spills. No kernel of
// the trace stage or of art_permeate.hip has a scratch instruction, the OBB nearest one at 8 waves
// included (its round-3 spills went with the round-4 leaf layout; profiles/r06_spill_check.txt).
// One reports a private segment all the same: echo_muffle_kernel<false, true>, ScratchSize 20 with
// no scratch instruction in its body and uses_flat_scratch 0 (profiles/trace_split_resources.txt);
// every other kernel reports ScratchSize 0.
constexpr int kNearestObbWaves = 8;  // (7, without the round-3 spills, measured slower: DESIGN.md §4.0, config 3 nearest 132 -> 175 us)
template <bool EX, bool OBB>
constexpr int kNearestWaves = EX ? 6 : (OBB ? kNearestObbWaves : 8);

// Nearest hit of the quad's ray s (identical in the 4 lanes; `my` = the ray's kBvhStack-entry
// stack inside the wave's 16 stacks; s_bound / s_key = the wave's 16 shared pruning bounds and
// result keys): (distance, order) minimum in best / code of every lane of the quad.
// With work sharing, the quads that traverse parts of one ray's tree prune against the smallest
// distance any of them found (s_bound, published once the wave has shared work), and the ray's
// result is the (distance, order) minimum of their results (a 64-bit LDS minimum of (distance
// bits, order); the two zeros compare equal, as in the reference's `<`, and the path kernel
// re-evaluates a zero distance).
// PERM: the permeation job's first-hit cast (ShootRayCast :101-141: INFINITY sentinel, inverse OBB
// rotation); otherwise the raytracer's (:225-280: float.MaxValue sentinel).
// TAB: every ray of the workgroup starts at one origin (a fan's bounce-0 casts), and `tab` holds
// each BVH node's widened box relative to it (node_table): a node test is 6 multiplies and the
// min / max, with the same operands as node_entry's.
// LOG: every leaf a quad tests is appended to its ray's log (s_log = the wave's 16 records of 16 u16,
// s_lcnt = their counters; a thief appends to the home ray's), and the node margins use
// log_margin_om (the echo replay, art_trace_rays.hpp).
// Every instantiation but the counting ones (EX) caps the node margins by the ray's node_margin_cap
// (art_frame_math.hpp; TAB: in the table). A thief takes the home ray's cap along with its om.
template <bool EX, bool OBB, bool PERM = false, bool TAB = false, bool LOG = false>
__device__ __forceinline__ void quad_nearest_core(const DevScene& sc, Seg s, bool alive, int lane, uint32_t* my,
                                                  int* s_bound, unsigned long long* s_key, float& best, int& code,
                                                  unsigned long long* ex, const NodeTab* tab = nullptr,
                                                  uint16_t* s_log = nullptr, int* s_lcnt = nullptr) {
  const int qd = lane & 3, wq = lane >> 2;
  uint32_t* const s_wave = my - wq * kBvhStack;
  best = FLT_MAX;
  code = kNoHit;
  if (sc.bvh_levels == 0) return;  // no colliders: every ray misses
  if (qd == 0) s_key[wq] = ~0ull;  // the ray's shared result key, opened before the loop
  unsigned nt[3] = {0u, 0u, 0u}, nnode = 0;
  float om = fabsf(s.o.x) + fabsf(s.o.y) + fabsf(s.o.z);
  constexpr bool CAP = !EX && !TAB;  // (TAB: node_table_build capped the table's boxes)
  float cap = 0.0f;
  if (LOG) {
    float xcap;
    om = log_margin_om(sc, s.o, fabsf(s.d.x) + fabsf(s.d.y) + fabsf(s.d.z), xcap, &cap);
    if (qd == 0) s_lcnt[wq] = 0;
  } else if (CAP) {
    cap = ray_margin_cap(sc, om, OBB);
  }
  bool force = force_all(s, om);
  // the forced lanes as a lane mask (wave-uniform, kept in SGPRs): a node test ORs it in with scalar
  // instructions (__builtin_amdgcn_inverse_ballot_w64) instead of a per-lane 0/1 value
  unsigned long long fmk = __builtin_amdgcn_ballot_w64(force);
  const int leaf0 = sc.bvh_leaf0;
  const BvhRes br = bvh_res(sc);
  int g = alive ? 0 : -1, sp = 0, bp = 0, home = wq;
  float lim = FLT_MAX;   // pruning bound: best, and (shared work) the other quads' results for the ray
  bool shared = false;   // wave-uniform: work was shared in this wave
  // this quad's own (distance, order) minimum over the leaves it tested, as a nearest_key (~0: none)
  unsigned long long mykey = ~0ull;
  unsigned nsteps = 0;
  (void)nsteps;
  // The order in which the three lambdas below are defined is load-bearing for the register allocation, not for
  // the logic: with inner_step ahead of leaf_step the compiler gives nearest_first_kernel<true, true, false, false,
  // false> and <true, true, true, false, false> 66 VGPRs instead of 64, 7 waves per SIMD instead of 8
  // (profiles/trace_split_resources.txt). Re-check the kernels' resources (tools/spill_check.py) after any edit here.
  // branch-free pop of entries [bp, sp): the slot is read unconditionally (clamped), -1 when empty
  auto pop = [&]() {
    const bool has = sp > bp;
    const int t = (int)my[has ? sp - 1 : 0];
    g = has ? t : -1;
    sp = has ? sp - 1 : sp;
    if (sp == bp) sp = bp = 0;
  };
  auto leaf_step = [&](int leaf) {
    ART_DIAG_STEP(nsteps);
    if (LOG && qd == 0) {  // (one quad visits a node, so a ray's log holds a leaf once)
      const int at = atomicAdd(s_lcnt + home, 1);
      if (at < kLogK) s_log[home * 16 + 1 + at] = (uint16_t)(leaf - leaf0);
    }
    int cc, tid;
    float dd;
    const bool h = leaf_slot_test<OBB, PERM>(s, br, (leaf - leaf0) * kBvhLeaf + qd, cc, dd, tid, nt, sc.obbc);
    // no hit, NaN and FLT_MAX-or-more never win (strict < against float.MaxValue; the permeation
    // cast: against INFINITY, so a hit at FLT_MAX counts). A hit distance is >= 0 or -0, so the key
    // (distance bits, order code) orders as the reference's sequential strict-< first minimum.
    const unsigned long long k = quad_min_u64(h && (PERM ? dd < INFINITY : dd < FLT_MAX) ? nearest_key(dd, cc) : ~0ull);
    if (k < mykey) {
      mykey = k;
      const float d = __uint_as_float((uint32_t)(k >> 32));
      lim = fminf(lim, d);
      if (shared && qd == 0) atomicMin(s_bound + home, __float_as_int(d));
    }
  };
  // A child is entered when its widened box is entered at or before the bound (a winner or tie
  // lies strictly after every ancestor's entry); quad_descend orders the entered ones.
  auto inner_step = [&]() {
    const int c0 = 4 * g + 1;
    if (EX && qd == 0) ++nnode;
    ART_DIAG_STEP(nsteps);
    float tn;
    bool h;
    if (TAB) {
      h = node_entry_tab(s, tab, c0 + qd, tn);
    } else {
      h = node_entry<CAP>(s, load_node(br, c0 + qd), om, tn, cap);
    }
    const float en = fmaxf(tn, 0.0f);
    const bool enter = __builtin_amdgcn_inverse_ballot_w64(fmk) | (h & (en <= lim));  // (empty nodes: art_bvh.hip cull_stored)
    quad_descend(enter, en, force, qd, c0, my, g, sp, bp);  // (its pop keeps sp == bp => 0)
  };
  // Speculative while-while (Aila & Laine): a quad that reaches a leaf parks it and keeps
  // descending; the wave tests leaves once every quad with work holds one, so both kinds of step
  // run with most quads busy. The order in which leaves are tested does not change the minimum.
  int pend = -1;
  for (;;) {
    const unsigned long long act = __builtin_amdgcn_ballot_w64((g & pend) >= 0) & kQuad0;  // g >= 0 || pend >= 0
    if (!act) break;
    {  // Wave priority by unfinished rays: the waves with the most rays left (the ones that set the
       // kernel's length) issue first, the nearly finished ones fill the gaps (s_setprio, 0..3)
      const int na = pop64(act);
      if (na > 12) __builtin_amdgcn_s_setprio(3);
      else if (na > 8) __builtin_amdgcn_s_setprio(2);
      else if (na > 4) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    const unsigned long long donors = __builtin_amdgcn_ballot_w64(sp > bp) & kQuad0, idle = ~act & kQuad0;
    if (donors && pop64(idle) >= kStealMinIdle) {  // wave-uniform: the k-th idle quad takes the k-th donor's stack bottom
      if (!shared) {       // publish every ray's bound once
        shared = true;
        if (qd == 0) s_bound[wq] = __float_as_int(lim);
      }
      const StealRole sr = steal_pairing(lane, qd, act, donors, idle, sp > bp);
      const bool thief = sr.thief, robbed = sr.robbed; const int src = sr.src;
      const int dbp = __shfl(bp, src), dhome = __shfl(home, src);
      const Seg ds = shfl_seg(s, src);
      // the ray's other derived values too (|o|_1, force: the home's own values)
      const float dlim = __shfl(lim, src), dom = __shfl(om, src);
      const int dforce = __shfl((int)force, src);
      float dcap = 0.0f;
      if (CAP) dcap = __shfl(cap, src);
      if (thief && mykey != ~0ull && qd == 0) atomicMin(s_key + home, mykey);
      if (thief) {
        g = (int)s_wave[(src >> 2) * kBvhStack + dbp];
        sp = bp = 0;
        home = dhome;
        s = ds;
        om = dom;
        cap = dcap;
        force = dforce != 0;
        lim = dlim;
        mykey = ~0ull;  // (the finished ray's result went to its key above)
      }
      fmk = __builtin_amdgcn_ballot_w64(force);
      if (robbed && ++bp == sp) sp = bp = 0;
    }
    if (shared) lim = fminf(lim, __int_as_float(s_bound[home]));
    for (;;) {
      if (g >= leaf0 && pend < 0) { pend = g; pop(); }
      const bool inner = g >= 0 && g < leaf0;
      // (after the park above, a quad with no parked leaf and a node holds an inner node, so "some
      // quad has no parked leaf and work" implies "some quad is inner": one ballot decides)
      if (__builtin_amdgcn_ballot_w64((pend & ~g) < 0) == 0ull) break;  // pend < 0 && g >= 0, one compare
      if (inner) inner_step();
    }
    if (pend >= 0) { leaf_step(pend); pend = -1; }
  }
#ifdef ART_DIAG
  if (qd == 0 && alive) diag_add(2, nsteps);
#endif
  unsigned long long k = mykey;
  if (shared) {  // the ray's result: the minimum over the quads that traversed it
    if (mykey != ~0ull && qd == 0) atomicMin(s_key + home, mykey);
    k = s_key[wq];
  }
  best = k == ~0ull ? FLT_MAX : __uint_as_float((uint32_t)(k >> 32));
  code = k == ~0ull ? kNoHit : (int)(uint32_t)k;
  if (ex) exec_add_tests(ex + kExecNearest, nt, nnode);
}

// ------------------------------------------------------------------------------------------
// Nearest hits of one bounce: one 64-ray group per workgroup, wave w traverses rays 16w .. 16w+15
// with 4 lanes each (quad_nearest_core), 8 waves per SIMD. hits[g * 64 + r] = (distance bits,
// code) of the group's ray slot r. Bounce 0 starts every ray at its fan's origin; later bounces
// read the path kernel's ray state and traverse only the rays its live list holds (the workgroups
// past the list return at once).
// ------------------------------------------------------------------------------------------
// FOLD (multi-hit frames with one batch slot and no hit outputs): the path kernel's work for each
// ray runs in this kernel's epilogue (fold_path), every ray keeps its slot for all bounces (no live
// list: a finished ray's quad only helps the others through work sharing), and the echo segments and
// hit records go to fixed per-bounce slots (VisPairs::fixed): no path launch and no reservation
// atomics per bounce.
// ONE (the one-hit fused plan, any non-FOLD bounce-0 cast): the same record at the ray's slot and
// nothing else of the path: the echo slot takes the provisional echo half (0 for a miss; an echo
// wave that finds a blocker stores the reset 0 over it), and a slot without a hit marks its hit
// record too (hrec.w = kNoRecord), so a muffle wave reads the hit records alone.
template <bool ONE = false>
__device__ __forceinline__ void fold_path(const DevScene& sc, const FrameParams& fp, const FanLayout& L, uint8_t* block,
                                          const float* origins, const VisPairs& vp, float4* state, int step, uint32_t sidx,
                                          int fan, int ray,
                                          bool slot_ok, vec3 o, vec3 d, float life, int hits, bool alive, float dist, int code,
                                          bool lead) {
  const int H = fp.H;
  const vec3 O = load3(origins, fan);
  const bool hit = alive && code != kNoHit;
  int type = kNone, idx = 0;
  if (hit) {
    winner_of(sc, make_seg(o, d), code, type, idx, dist);
    o = o + d * dist;  // :111
    life -= dist;      // :112
    hits += 1;         // :113
  }
  uint16_t* echo = reinterpret_cast<uint16_t*>(block + (size_t)fan * L.stride + L.echo_off);
  const size_t rec = (size_t)step * vp.fixed + sidx;
  if (lead) {  // this bounce's echo ray (:124-145) and the muffle rays' hit record (:150-173), or none
    if (hit) {   // (the echo's index is ray * H + hits - 1 = ray * H + step: every earlier bounce hit)
      const vec3 off = o - d * kEps;                 // :124, :158
      const float dist0 = distance(O, o);            // :130 (un-offset hit point)
      const uint32_t half = f32tof16(dist0 * echo_of(sc, type, idx));  // :142-144
      vp.out[rec] = make_uint2(__float_as_uint(dist0), half);
      vp.hrec[rec] = make_float4(off.x, off.y, off.z, __uint_as_float((uint32_t)fan * (uint32_t)fp.T));  // batch slot 0
      // FOLD: a blocked echo keeps the reset value (:76); the echo traversal stores the rest
      echo[ray * H + hits - 1] = ONE ? (uint16_t)half : (uint16_t)0;
    } else {
      vp.out[rec] = make_uint2(0u, kNoRecord);
      if (ONE) {
        vp.hrec[rec] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kNoRecord));
        if (slot_ok) echo[ray] = 0;  // a miss keeps the reset value (:76, :200-207)
      }
    }
  }
  if (ONE) return;
  // termination / reflection (:179-193, ReflectRay :456-532)
  bool next = hit;  // a miss ends the ray (:200-207)
  if (hit) next = (hits >= H || life <= 0.0f) ? false : reflect_at_hit(sc, fp, type, idx, o, d, life);
  if (lead && slot_ok && alive) {  // (an ended ray's state already says so: later bounces leave it)
    state[2 * (size_t)sidx] = make_float4(o.x, o.y, o.z, life);
    state[2 * (size_t)sidx + 1] = make_float4(d.x, d.y, d.z, __int_as_float(hits | (next ? 256 : 0)));
    if (alive && !next)  // the ray stops here: slots past its last hit keep the reset value 0 (:72-80)
      for (int k = hits; k < H; ++k) echo[ray * H + k] = 0;
  }
}

// EX: count the executed tests (fp.exec); OBB: the scene has OBBs; FOLD: fold_path above.
// TAB (bounce 0 only, 64-ray groups per fan a multiple of 4, <= kTabNodes BVH nodes): workgroups of
// 1024 lanes, the 4 consecutive 64-ray groups of one fan, all rays at the fan origin, traverse with
// the shared-origin node table in LDS (node_table_build; 2 workgroups and 8 waves per SIMD per CU,
// 70 KB of LDS each).
// LOG (bounce 0 of the one-hit fused plan on OBB-free scenes, not EX / FOLD / TAB): the cast logs each ray's tested leaves for
// the echo replay (EchoLog above; quad_nearest_core<..., LOG>) and stores the records beside the hits.
template <bool EX, bool OBB, bool FOLD, bool TAB = false, bool LOG = false>
__global__ __launch_bounds__(TAB ? 1024 : 256) __attribute__((amdgpu_waves_per_eu(kNearestWaves<EX, OBB>))) void nearest_first_kernel(
    DevScene sc, FrameParams fp, const float* __restrict__ origins, const int* __restrict__ ray_order,
    int2* __restrict__ hits, float4* __restrict__ state, int step, uint32_t* __restrict__ zero, uint32_t nzero,
    uint32_t* __restrict__ counters, FanLayout L, uint8_t* __restrict__ block, VisPairs vp, EchoLog el) {
  static_assert(!LOG || (!EX && !FOLD && !TAB && !OBB), "the logging cast is the plain bounce-0 cast of OBB-free scenes");
  constexpr int kGroupsPerWg = TAB ? 4 : 1;
  __shared__ uint32_t s_stk[kBvhStack * 64 * kGroupsPerWg];
  __shared__ int s_bound[64 * kGroupsPerWg];
  __shared__ unsigned long long s_key[64 * kGroupsPerWg];
  __shared__ std::conditional_t<TAB, NodeTab, int> s_tab;
  __shared__ __attribute__((aligned(8))) uint16_t s_log[LOG ? 16 * 64 * kGroupsPerWg : 4];
  __shared__ int s_lcnt[LOG ? 64 * kGroupsPerWg : 1];
  if (step == 0 && el.count && !el.keep_count && blockIdx.x == 0 && threadIdx.x < kEchoCountSlots) el.count[threadIdx.x] = 0ull;
  ART_WAVE_TIMER(0);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nrb = (fp.R + 63) >> 6;
  const int ngroups = fp.S * nrb;
  const int g = (int)blockIdx.x * kGroupsPerWg + (w >> 2);  // TAB: 4 groups of one fan per workgroup
  const int rr = 16 * (w & 3) + (lane >> 2);
  uint32_t* my = s_stk + (16 * w + (lane >> 2)) * kBvhStack;
  if constexpr (TAB) {  // the fan origin's node table (every ray of the workgroup starts there)
    node_table_build<!EX, OBB>(sc, load3(origins, g / nrb), &s_tab);
    __syncthreads();
  }
  unsigned long long* ex = EX ? fp.exec : nullptr;
  float best;
  int code;
  vec3 o, d;
  bool alive, write;
  uint32_t out;  // ray slot (< 2^31: fast_fans_per_launch)
  float life = fp.max_life;
  int nhits = 0, fan = 0, ray = 0;
  bool slot_ok = true;
  if (FOLD) {  // every ray in its slot for every bounce (loaded twice more below: one helper cost two kernels 2 VGPRs)
    if (step == 0) {
      for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nzero; i += gridDim.x * blockDim.x) zero[i] = 0u;
      if (counters && blockIdx.x == 0 && threadIdx.x < 4) counters[threadIdx.x] = 0u;
    }
    fan = g / nrb;
    const int sl = (g - fan * nrb) * 64 + rr;
    slot_ok = sl < fp.R;
    ray = slot_ok ? ray_order[sl] : 0;
    out = (uint32_t)g * 64u + (uint32_t)rr;
    if (step == 0) {
      o = load3(origins, fan);
      d = load_dir(sc.dirs, ray);
      alive = slot_ok;
    } else {
      const float4 a = state[2 * (size_t)out], b = state[2 * (size_t)out + 1];
      o = mk3(a.x, a.y, a.z);
      life = a.w;
      d = mk3(b.x, b.y, b.z);
      nhits = __float_as_int(b.w) & 0xff;
      alive = slot_ok && ((__float_as_int(b.w) >> 8) & 1) != 0;
    }
    write = false;
  } else if (step > 0) {  // the previous bounce's list of live ray slots
    const uint32_t* live = live_list(state, ngroups);
    const uint32_t cnt = live[(size_t)ngroups * 64 + step];
    if ((uint32_t)g * 64u >= cnt) return;  // the whole workgroup: past the list
    const uint32_t e = (uint32_t)g * 64u + (uint32_t)rr;
    const bool ok = e < cnt;
    const uint32_t i = ok ? live[e] : 0u;
    const float4 a = state[2 * (size_t)i], b = state[2 * (size_t)i + 1];
    o = mk3(a.x, a.y, a.z);
    d = mk3(b.x, b.y, b.z);
    alive = ok && ((__float_as_int(b.w) >> 8) & 1) != 0;
    write = ok;
    out = i;
    asm volatile("" : "+v"(out));  // (a 32-bit copy, apart from the 64-bit state offset above)
  } else {
    if (state && blockIdx.x == 0 && threadIdx.x < 2 * kLiveCounters)  // multi-hit frame: clear the counters
      live_list(state, ngroups)[(size_t)ngroups * 64 + threadIdx.x] = 0u;
    // the frame's muffle accumulators and pair counters, consumed only by later launches (no
    // memset dispatch between frames)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nzero; i += gridDim.x * blockDim.x) zero[i] = 0u;
    if (counters && blockIdx.x == 0 && threadIdx.x < 4) counters[threadIdx.x] = 0u;
    const int fan = g / nrb;  // (twin of the FOLD branch's bounce-0 load above)
    const int slot = (g - fan * nrb) * 64 + rr;
    alive = slot < fp.R;
    const int ray = alive ? ray_order[slot] : 0;
    o = load3(origins, fan);
    d = load_dir(sc.dirs, ray);
    write = true;
    out = (uint32_t)g * 64u + (uint32_t)rr;
  }
  if (EX && step < kExecBounces)  // live rays traced this bounce (one per quad)
    exec_add(ex, kExecBounce0 + step, (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(alive) & kQuad0));
#ifdef ART_DIAG
  const unsigned long long t0 = clock64();
#endif
  quad_nearest_core<EX, OBB, false, TAB, LOG>(sc, make_seg(o, d), alive, lane, my, s_bound + 16 * w, s_key + 16 * w, best,
                                              code, ex, TAB ? reinterpret_cast<const NodeTab*>(&s_tab) : nullptr,
                                              s_log + 256 * (LOG ? w : 0), s_lcnt + 16 * (LOG ? w : 0));
  // The one-hit fused plan (vp.fixed set on a non-FOLD cast, bounce 0 only): the ray's hit record and
  // provisional echo half from this epilogue (fold_path<true>), no nearest-hit store.
  const bool one = !FOLD && vp.fixed != 0u;  // (kernel-uniform)
  if (FOLD || one) {
    // The ray's state is fetched again rather than kept live across the traversal (a memory
    // clobber: the compiler may not reuse the values loaded before it): 64 VGPRs, no spills.
    asm volatile("" ::: "memory");
    {  // (twin of the FOLD entry's load above)
      const int rr2 = 16 * (w & 3) + (lane >> 2);
      fan = g / nrb;
      const int sl = (g - fan * nrb) * 64 + rr2;
      slot_ok = sl < fp.R;
      ray = slot_ok ? ray_order[sl] : 0;
      out = (uint32_t)g * 64u + (uint32_t)rr2;
      if (!FOLD || step == 0) {
        o = load3(origins, fan);
        d = load_dir(sc.dirs, ray);
        life = fp.max_life;
        nhits = 0;
        alive = slot_ok;
      } else {
        const float4 a = state[2 * (size_t)out], b = state[2 * (size_t)out + 1];
        o = mk3(a.x, a.y, a.z);
        life = a.w;
        d = mk3(b.x, b.y, b.z);
        nhits = __float_as_int(b.w) & 0xff;
        alive = slot_ok && ((__float_as_int(b.w) >> 8) & 1) != 0;
      }
    }
    if (FOLD) {
      if (EX) exec_add(fp.exec, kExecEchoPairs, (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(alive && code != kNoHit) & kQuad0));
      fold_path(sc, fp, L, block, origins, vp, state, step, out, fan, ray, slot_ok, o, d, life, nhits, alive, best, code,
                (lane & 3) == 0);
      return;
    }
    if constexpr (LOG) {
      // The ray's record: its leaves, or kLogTraverse for a ray the replay may not decide, from the
      // ray fetched again above (the logging cast runs in the fused plan only).
      const int qd = lane & 3, rq = 16 * w + (lane >> 2);  // the workgroup's ray
      const vec3 O = o, dd = d;
      const float d1 = fabsf(dd.x) + fabsf(dd.y) + fabsf(dd.z);
      bool trav = true;
      uint32_t cnt = 0u;
      if (sc.bvh_levels > 0) {
        float xcap;
        const float om = log_margin_om(sc, O, d1, xcap);  // the cast's own operand, so the same forced rays
        cnt = (uint32_t)s_lcnt[rq];
        Seg sd;  // (force_all reads the direction only)
        sd.o = O; sd.d = sd.inv = dd; sd.a2 = 0.0f;
        trav = force_all(sd, om) || cnt > (uint32_t)kLogK || !(best * d1 <= xcap);
      }
      uint2 v = reinterpret_cast<const uint2*>(s_log)[rq * 4 + qd];
      if (qd == 0) v.x = (v.x & 0xffff0000u) | (trav ? kLogTraverse : cnt);
      if (write) reinterpret_cast<uint2*>(el.rec)[(size_t)out * 4 + qd] = v;
    }
    fold_path<true>(sc, fp, L, block, origins, vp, nullptr, 0, out, fan, ray, slot_ok, o, d, life, 0, alive, best, code,
                    (lane & 3) == 0);
  } else {
    // (the ray slot stays a 32-bit value across the traversal: an opaque copy keeps the compiler from
    // widening it to a 64-bit offset before the loop, two more live VGPRs)
    asm volatile("" : "+v"(out));
    if ((lane & 3) == 0 && write) hits[out] = make_int2(__float_as_int(best), code);
  }
#ifdef ART_DIAG
  if (lane == 0) diag_add(0, clock64() - t0);
#endif
}

}  // namespace art
