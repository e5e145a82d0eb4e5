// art_trace_rays.hpp — what the trace stage's kernels hand to one another (no kernel here): the echo replay's leaf
// log, the ray state between bounces, the visibility work (VisPairs), the winner's re-evaluation and reflection.
#pragma once
#include "art_quad.hpp"

namespace art {

// Bounce-0 echo replay (one-hit fused plan): the bounce-0 nearest cast
// (nearest_first_kernel<..., LOG>) logs the leaves it tests for each ray, with node margins wide
// enough that every collider the ray's echo test can report lies in a logged leaf; the echo waves of
// echo_muffle_kernel then test those leaves' slots against the echo segment instead of traversing.
// A ray's record is 16 u16: [0] the number of logged leaves or kLogTraverse, [1 ..] kLogK leaf ids.
// A ray keeps the echo traversal (kLogTraverse) when its log overflowed, when its direction or origin
// is degenerate (force_all), or when its hit lies past the distance the margins were sized for:
// best * |d|_1 > kLogCapFrac * the L1 diagonal of the BVH root's box.
constexpr int kLogK = 15;
constexpr uint32_t kLogTraverse = 0xffffu;
constexpr float kLogCapFrac = 0.3f;
struct EchoLog {
  uint16_t* rec;              // [ray slots][16]; nullptr: no log, every echo ray traverses
  // echo rays decided by replay (low word) | by traversal (high word): kEchoCountSlots partial sums, an
  // echo wave adds to the slot of its workgroup index (one shared counter serialized the frame's
  // 8192 atomics: echo_muffle_kernel 47 -> 141 us at config 2); cleared by the frame's first cast
  unsigned long long* count;
  int keep_count;             // a later fan chunk of the frame: the counts go on
};
// The logging cast's margin operand for a ray (O, d) in place of |O|_1 (node_entry's om), and the cap
// xcap on best * |d|_1 it covers: 1.05 |O|_1 + 4 |d|_1 + the reach term (replay).
// The reach term covers how far outside a sphere an echo blocker can be reported at reach xcap:
// 0.4 xcap by the square-root form of the sphere lemma, or, with no sphere smaller than r_min,
// kLogReachSq (r + xcap)^2 / r + kLogReachLin xcap at r = min(r_min, xcap) by its r-aware form
// (sphere_report_slack, art_frame_math.hpp; (r + X)^2 / r decreases on (0, X], and beyond X the
// sphere's own scale covers it). The linear part is sized by the boxes, whose smaller factor (1e-4)
// has to cover the echo ray's deviation from the primary segment, 1.4e-6 xcap, with the same operand.
// A non-finite or zero operand gives NaN or infinity there, and the fminf keeps 0.4 xcap.
// cap (when asked for): the ray's node margin cap (node_margin_cap, art_frame_math.hpp) for this operand. It
// bounds the base part b alone and the reach term keeps its full factor: cap(S_root + b) + kCullSphere * reach.
// Where the reach term is the square-root form 0.4 xcap, the replay's step 3 leans on the base part's
// kCullSphere * r for a sphere's own radius, so the ray takes no cap.
constexpr float kLogReachSq = 2e-4f, kLogReachLin = 2.8e-2f;
__device__ __forceinline__ float log_margin_om(const DevScene& sc, vec3 O, float d1, float& xcap, float* cap = nullptr) {
  const CullRec root = ldc(sc.bvh, 0);
  xcap = kLogCapFrac * ((root.hix - root.lox) + (root.hiy - root.loy) + (root.hiz - root.loz));
  const float b = 1.05f * (fabsf(O.x) + fabsf(O.y) + fabsf(O.z)) + 4.0f * d1;
  const float r = fminf(sc.r_min, xcap), rx = r + xcap;
  const float reach = ART_SPHERE_SLACK_SCALE * (kLogReachSq * (rx * (rx / r)) + kLogReachLin * xcap);
  const float root_reach = 0.4f * xcap, t = fminf(root_reach, reach);
  if (cap) {
    NodeCapCoef cc = sc.cap;
    if (!(reach < root_reach)) cc.on = 0.0f;
    *cap = node_cap_eval(cc, node_abs_sum(root.lox, root.loy, root.loz, root.hix, root.hiy, root.hiz) + b, kCullBox, t);
  }
  return b + t;
}

constexpr int kLiveCounters = 32;  // per-bounce live-list counters (H <= 32)

// Ray state between bounce launches: [groups * 64][2] float4 (o, life | d, hits | alive << 8),
// then the live list u32[groups * 64], its per-bounce counters u32[kLiveCounters] and the echo
// pairs each bounce emitted u32[kLiveCounters] (bounce k's echo pairs follow bounce k-1's).
__host__ __device__ __forceinline__ uint32_t* live_list(float4* state, int ngroups) {
  return reinterpret_cast<uint32_t*>(state + 2 * (size_t)ngroups * 64);
}
__host__ __device__ __forceinline__ uint32_t* echo_counts(float4* state, int ngroups) {
  return live_list(state, ngroups) + (size_t)ngroups * 64 + kLiveCounters;
}

// Visibility work (struct of arrays, below): echo segments and outputs, hit records. `fixed`
// (multi-hit frames with one batch slot and no hit outputs, nearest_first_kernel<..., FOLD>): the
// records sit at fixed positions bounce * fixed + ray slot and are compact (round 6): no echo
// segment, out = (echo distance bits, echo half) with out.y = kNoRecord marking a slot with no hit
// that bounce (then nothing else is written for it), hrec = (off.xyz, muffle destination); the
// echo traversal rebuilds the segment from off and the fan origin, and the echo's index from the
// slot (fold_path).
constexpr uint32_t kNoRecord = 0xffffffffu;
struct VisPairs {
  float4* seg;
  uint2* out;
  float4* hrec;
  uint32_t echo_cap;  // multiple of 64
  uint32_t fixed;     // 0: records compacted in emission order; else ray slots per bounce
};

__device__ __forceinline__ float echo_of(const DevScene& sc, int type, int idx) {
  return type == kSphere ? sc.sphc[idx].echo : (type == kAabb ? sc.aabbc[idx].echo : sc.obbc[idx].echo);
}

// ReflectRay (:456-532) at hit point o of collider (type, idx), then the offset (:528) and the
// absorption (:531); false when the ray's life runs out (:189).
__device__ __forceinline__ bool reflect_at_hit(const DevScene& sc, const FrameParams& fp, int type, int idx, vec3& o, vec3& d,
                                               float& life) {
  vec3 n = mk3(0.0f, 0.0f, 0.0f);
  float absorption = 0.0f;
  if (type == kAabb) {
    const AabbCold b = sc.aabbc[idx];
    vec3 lp = o - mk3(b.cx, b.cy, b.cz);
    vec3 ap = abs3(lp);
    float dx = b.hx - ap.x, dy = b.hy - ap.y, dz = b.hz - ap.z;
    if (dx < dy && dx < dz) n.x = usign(lp.x);
    else if (dy < dx && dy < dz) n.y = usign(lp.y);
    else n.z = usign(lp.z);
    absorption = b.absorption;
  } else if (type == kObb) {
    const ObbRec b = sc.obb[idx];
    const ObbCold bc2 = sc.obbc[idx];
    vec3 lh = qmul(inverse_q(bc2), o - mk3(b.cx, b.cy, b.cz));  // :489 (Q5: inverse of the stored inverse)
    vec3 ap = abs3(lh);
    vec3 df = mk3(bc2.hx, bc2.hy, bc2.hz) - ap;
    vec3 ln = mk3(0.0f, 0.0f, 0.0f);
    if (df.x < df.y && df.x < df.z) ln.x = usign(lh.x);
    else if (df.y < df.x && df.y < df.z) ln.y = usign(lh.y);
    else ln.z = usign(lh.z);
    n = qmul(stored_q(b), ln);                                 // :510
    absorption = bc2.absorption;
  } else {
    const SphereRec c = sc.sph[idx];
    n = normalize(o - mk3(c.cx, c.cy, c.cz));                  // :516
    absorption = sc.sphc[idx].absorption;
  }
  d = reflect(d, n);                    // :525
  o = o + d * kEps;                     // :528
  life -= fp.max_life * absorption;     // :531
  return !(life < 0.0f);
}

// The winner's collider from its order code, and the exact (Unity min / max) re-evaluation of a zero
// distance (IEEE and Unity min / max differ only in the sign of an equal-magnitude zero pair).
__device__ __forceinline__ void winner_of(const DevScene& sc, const Seg& s, int code, int& type, int& idx, float& dist) {
  const int rank = code >> 28;
  idx = code & 0x0fffffff;
  type = rank == 0 ? kSphere : (rank == 1 ? kAabb : kObb);
  if (dist == 0.0f) {
    if (type == kSphere) sphere_hit_dist(s, sc.sph[idx], dist);  // (a -0 the result key made +0)
    if (type == kAabb) aabb_test<true>(s, sc.aabb[idx], dist);
    if (type == kObb) { const ObbRec r = sc.obb[idx]; obb_test<true>(s, r, stored_q(r), dist); }
  }
}

}  // namespace art
