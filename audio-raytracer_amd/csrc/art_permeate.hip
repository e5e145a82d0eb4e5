// art_permeate.hip — the permeation job over the collider BVH: the first-hit cast is quad_nearest_core<..., PERM>
// (art_trace_nearest.hpp). (No kernel here records a wave timeline: ART_WAVE_TIMES belongs to art_trace.hip.)
#undef ART_WAVE_TIMES
#include "art_quad.hpp"
#include "art_trace_nearest.hpp"

namespace art {

// ------------------------------------------------------------------------------------------
// Permeation job (AudioPermeationJobBatched.Execute :34-91) over the BVH. One wave per (batch slot,
// fan), 16 quads:
//   1. the slot's value is written by the highest-index ray of its last batch whose permeation
//      first hit exists (each hitting ray overwrites it, :85; App. B Q7): quads cast the batch's
//      rays from its end, 16 at a time (quad_nearest_core<PERM>: INFINITY sentinel, inverse OBB
//      rotation, :101-141 / :172-179), and the highest-index hitting ray wins;
//   2. its T loss rays (:61-85), one per quad: every collider whose widened box the ray enters at
//      t >= 0 is visited (no pruning: the loss sums penetrations along the whole ray), its loss
//      term evaluated (:225-328), the non-zero terms kept as (order code, term) in LDS, ranked by
//      order code and summed serially in reference order (Sphere, AABB, OBB, ascending index).
// Exactness: a collider the ray misses contributes exactly +0, and an entered-but-missed node's
// colliders are missed (DESIGN.md §5 item 8 for the slab tests; the sphere loss test's b^2 - c
// discriminant carries at most ~32 eps |oc|^2 of rounding, inside the sphere margin); +-0 terms never
// change the running sum (it starts at +0 and is never -0), so only non-zero terms are summed. A loss
// ray meeting more than kLossCap colliders is summed by the whole wave over every collider instead.
// ------------------------------------------------------------------------------------------
constexpr int kLossCap = 48;  // kept (code, term) entries per loss ray

// Loss term of global collider g (Sphere, AABB, OBB ranges) for segment s and target t (0 when t
// owns it), the reference expressions (:225-328).
__device__ __forceinline__ float loss_term_global(const DevScene& sc, const Seg& s, int g, int t) {
  if (g < sc.ns) {
    const SphereRec r = sc.sph[g];
    return r.tid != t ? perm_term_sphere(s, r, sc.sphc[g].density) : 0.0f;
  }
  g -= sc.ns;
  if (g < sc.na) {
    const AabbRec r = sc.aabb[g];
    return r.tid != t ? perm_term_slab(s.o.x, s.o.y, s.o.z, s.inv.x, s.inv.y, s.inv.z, r.mnx, r.mny, r.mnz, r.mxx, r.mxy,
                                       r.mxz, sc.aabbc[g].density)
                      : 0.0f;
  }
  g -= sc.na;
  if (g >= sc.no) return 0.0f;
  const ObbRec r = sc.obb[g];
  if (r.tid == t) return 0.0f;
  const quat q = stored_q(r);  // RayIntersectsOBBPermeation :294-300 rotates by the stored rotation
  const vec3 lo = qmul(q, s.o - mk3(r.cx, r.cy, r.cz));
  const vec3 ld = qmul(q, s.d);
  return perm_term_slab(lo.x, lo.y, lo.z, 1.0f / ld.x, 1.0f / ld.y, 1.0f / ld.z, r.lmnx, r.lmny, r.lmnz, r.lmxx, r.lmxy, r.lmxz,
                        sc.obbc[g].density);
}

// The whole wave over every collider in reference order (lanes over colliders, non-zero terms
// added serially): the overflow path. Wave-uniform result.
__device__ float loss_sum_wave(const DevScene& sc, const Seg& s, int t) {
  const int lane = threadIdx.x & 63, ctot = sc.ns + sc.na + sc.no;
  float sum = 0.0f;
  for (int base = 0; base < ctot; base += 64) {
    const float term = base + lane < ctot ? loss_term_global(sc, s, base + lane, t) : 0.0f;
    for (unsigned long long m = __builtin_amdgcn_ballot_w64(term != 0.0f); m; m &= m - 1ull)
      sum += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, term), __builtin_ctzll(m)));
  }
  return sum;
}

// Loss term of leaf slot `slot` (its order code in cc; 0 for an empty slot or a collider t owns).
template <bool OBB>
__device__ __forceinline__ float leaf_loss_term(const DevScene& sc, const Seg& s, const BvhRes& br, int slot, int t, int& cc) {
  auto ld = [&](int k) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(br.leaves, slot * (OBB ? 64 : 32) + 16 * k, 0, 0));
  };
  const float4 qa = ld(0), qb = ld(1);
  cc = __float_as_int(qb.w);
  if (cc < 0) return 0.0f;
  const int type = cc >> 28, idx = cc & 0x0fffffff;
  if (type == 0) {
    if (__float_as_int(qb.z) == t) return 0.0f;
    SphereRec r;
    r.cx = qa.x; r.cy = qa.y; r.cz = qa.z; r.r2 = qa.w;
    return perm_term_sphere(s, r, sc.sphc[idx].density);
  }
  if (type == 1 || !OBB) {
    if (__float_as_int(qb.z) == t) return 0.0f;
    return perm_term_slab(s.o.x, s.o.y, s.o.z, s.inv.x, s.inv.y, s.inv.z, qa.x, qa.y, qa.z, qa.w, qb.x, qb.y,
                          sc.aabbc[idx].density);
  }
  quat q;
  q.x = qa.w; q.y = qb.x; q.z = qb.y; q.w = qb.z;
  const vec3 ld3 = qmul(q, s.d);
  const float ix = recip_exact(ld3.x), iy = recip_exact(ld3.y), iz = recip_exact(ld3.z);
  const vec3 lo = qmul(q, s.o - mk3(qa.x, qa.y, qa.z));
  const float4 qc = ld(2), qe = ld(3);
  if (__float_as_int(qe.z) == t) return 0.0f;
  return perm_term_slab(lo.x, lo.y, lo.z, ix, iy, iz, qc.x, qc.y, qc.z, qc.w, qe.x, qe.y, sc.obbc[idx].density);
}

template <bool OBB>
__global__ __launch_bounds__(64) void permeate_bvh_kernel(DevScene sc, FrameParams fp, FanLayout L, const float* __restrict__ origins,
                                                         uint8_t* __restrict__ block, const int2* __restrict__ slot_batch) {
  __shared__ uint32_t s_stk[16 * kBvhStack];
  __shared__ int s_bound[16];
  __shared__ unsigned long long s_key[16];
  __shared__ uint32_t s_code[16][kLossCap];
  __shared__ float s_term[16][kLossCap], s_sorted[16][kLossCap];
  const int fan = blockIdx.y, slot = blockIdx.x, lane = threadIdx.x, qd = lane & 3, wq = lane >> 2;
  const int2 br = slot_batch[slot];
  if (br.y <= br.x) return;  // no batch maps to this slot: the value stays (stale / uninitialized, Q7)
  const vec3 O = load3(origins, fan);
  uint32_t* const my = s_stk + wq * kBvhStack;
  float* const ppr = reinterpret_cast<float*>(block + (size_t)fan * L.stride + L.perm_off);
  const int T = fp.T;

  // 1. the highest-index ray of [br.x, br.y) with a permeation first hit (ShootRayCast :58)
  int found = -1, code = kNoHit;
  float dist = 0.0f;
  int rtop = br.y - 1;  // the highest ray not yet cast
  {  // the batch's last ray alone first (it usually hits): quad 0 casts it and the wave's 15 idle
     // quads share its traversal (the work sharing of quad_nearest_core)
    float best;
    int c;
    quad_nearest_core<false, OBB, true>(sc, make_seg(O, load_dir(sc.dirs, rtop)), wq == 0, lane, my, s_bound, s_key, best,
                                        c, nullptr);
    const int c0 = __builtin_amdgcn_readlane(c, 0);
    if (c0 != kNoHit) {
      found = rtop;
      code = c0;
      dist = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, best), 0));
    }
    --rtop;
  }
  for (int r0 = rtop; r0 >= br.x && found < 0; r0 -= 16) {  // (wave-uniform)
    const int ray = r0 - wq;
    const bool alive = ray >= br.x;
    float best;
    int c;
    quad_nearest_core<false, OBB, true>(sc, make_seg(O, load_dir(sc.dirs, alive ? ray : br.x)), alive, lane, my, s_bound,
                                        s_key, best, c, nullptr);
    const unsigned long long hq = __builtin_amdgcn_ballot_w64(qd == 0 && alive && c != kNoHit);
    if (hq) {  // the lowest such quad holds the highest ray index
      const int src = __builtin_ctzll(hq);
      found = r0 - (src >> 2);
      code = __builtin_amdgcn_readlane(c, src);
      dist = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, best), src));
    }
  }
  if (found < 0) {  // reset (:43-46) and no ray hit
    for (int t = lane; t < T; t += 64) ppr[slot * T + t] = 0.0f;
    return;
  }
  const vec3 d = load_dir(sc.dirs, found);
  if (dist == 0.0f) {  // the exact (Unity min / max) distance of a zero first hit: only its sign can differ (twin of
    const Seg s0 = make_seg(O, d);  // winner_of, art_trace_rays.hpp, but the OBB test by the inverse rotation: sharing
    const int type = code >> 28, idx = code & 0x0fffffff;  // it missed the A/B bound of kernel_ms.permeate at config 5)
    if (type == 0) sphere_hit_dist(s0, sc.sph[idx], dist);
    else if (type == 1) aabb_test<true>(s0, sc.aabb[idx], dist);
    else obb_test<true>(s0, sc.obb[idx], inverse_q(sc.obbc[idx]), dist);
  }
  const vec3 o = O + d * dist;  // :61
  const vec3 off = o - d * kEps;

  // 2. the T loss rays (:67-85). P quads per ray (P = 16 / rays in the chunk, at
  // most 4, with an inner root): quad j of a ray traverses the root's children c with c % P == j, so
  // the ray's subtrees run side by side instead of leaving 16 - T quads idle (config 4: the job's
  // waves hold wave slots beside the nearest traversal for their whole length). The subtrees are
  // disjoint, so the ray's kept terms are its quads' lists together, ranked by order code across
  // them and summed serially in reference order as before.
  const BvhRes bres = bvh_res(sc);
  const int leaf0 = sc.bvh_leaf0, qshift = lane & ~3;
  for (int t0 = 0; t0 < T;) {  // (wave-uniform)
    const int P = leaf0 > 0 ? min(4, 16 / min(16, T - t0)) : 1;  // quads per ray
    const int nr = min(T - t0, 16 / P);                                              // rays in this chunk
    const int rq = wq / P, j = wq - rq * P, wq0 = rq * P;                            // ray, part, its first quad
    const int t = t0 + rq;
    const bool valid = rq < nr;
    const Seg s = make_seg(off, normalize(load3(sc.targets, valid ? t : 0) - off));
    const float om = fabsf(s.o.x) + fabsf(s.o.y) + fabsf(s.o.z);
    const bool force = force_all(s, om);
    int g = valid && sc.bvh_levels > 0 ? 0 : -1, sp = 0, n = 0;
    while (__any(g >= 0)) {
      while (g >= 0 && g < leaf0) {  // (quad-uniform) descend in index order, every entered child
        const int c0 = 4 * g + 1;
        const CullRec r = load_node(bres, c0 + qd);
        float tn;
        const bool h = node_entry(s, r, om, tn);
        // (an empty node's entry is +inf: cull_stored); at the root, this quad's share of the children
        const bool enter = (force | (h & (tn < INFINITY))) & (g != 0 || qd % P == j);
        const uint32_t eb = (uint32_t)(__builtin_amdgcn_ballot_w64(enter) >> qshift) & 0xFu;
        if (eb) {
          const int first = __builtin_ctz(eb);
          const uint32_t rest = eb & (eb - 1u);
          if (enter && qd != first) my[sp + __popc(rest & ((1u << qd) - 1u))] = (uint32_t)(c0 + qd);
          sp += __popc(rest);
          g = c0 + first;
        } else {
          g = sp > 0 ? (int)my[--sp] : -1;
        }
      }
      if (g >= leaf0) {
        int cc;
        const float term = leaf_loss_term<OBB>(sc, s, bres, (g - leaf0) * kBvhLeaf + qd, t, cc);
        const uint32_t nz = (uint32_t)(__builtin_amdgcn_ballot_w64(term != 0.0f) >> qshift) & 0xFu;
        const int at = n + __popc(nz & ((1u << qd) - 1u));
        if (term != 0.0f && at < kLossCap) { s_code[wq][at] = (uint32_t)cc; s_term[wq][at] = term; }
        n += __popc(nz);
        g = sp > 0 ? (int)my[--sp] : -1;
      }
    }
    // the ray's lists: the P quads' counts (every lane takes part in the shuffles)
    int nk[4], ntot = 0;
    bool fits = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      nk[k] = __shfl(n, 4 * min(wq0 + k, 15));
      if (k < P) { ntot += nk[k]; fits = fits && nk[k] <= kLossCap; }
    }
    // rank the kept terms by order code across the ray's lists (the lanes of its quads share the
    // entries), then sum them serially in that order in the ray's first lane
    // (lanes read each other's LDS entries: order the leaf loop's writes before the ranking and the
    // ranks' scatter before the sum, as kd_wave_kernel does)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    float* const srt = &s_sorted[0][0] + wq0 * kLossCap;  // the ray's P x kLossCap sorted entries
    if (valid && fits) {
      for (int i = qd; i < n; i += 4) {
        const uint32_t ci = s_code[wq][i];
        int rank = 0;
        for (int k = 0; k < P; ++k)
          for (int jj = 0; jj < nk[k]; ++jj) rank += s_code[wq0 + k][jj] < ci ? 1 : 0;
        srt[rank] = s_term[wq][i];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (valid && fits && j == 0) {
      float sum = 0.0f;
      for (int i = 0; i < ntot; ++i) sum += srt[i];
      if (qd == 0) ppr[slot * T + t] = (float)fp.R * fp.perm_strength - sum;  // :260
    }
    for (unsigned long long ov = __builtin_amdgcn_ballot_w64(qd == 0 && j == 0 && valid && !fits); ov; ov &= ov - 1ull) {  // (wave-uniform)
      const int src = __builtin_ctzll(ov), tt = t0 + (src >> 2) / P;
      const Seg so = make_seg(off, normalize(load3(sc.targets, tt) - off));
      const float sum = loss_sum_wave(sc, so, tt);
      if (lane == 0) ppr[slot * T + tt] = (float)fp.R * fp.perm_strength - sum;
    }
    t0 += nr;
  }
}

#ifdef ART_DIAG
// This source's share of the diagnostic histograms (its first-hit casts' ray steps), for art_diag_dump_impl.
bool diag_fetch_permeate(unsigned long long (*h)[64]) {
  return hipMemcpyFromSymbol(h, HIP_SYMBOL(g_diag), sizeof(unsigned long long) * 4 * 64) == hipSuccess;
}
#endif

void launch_permeate(const DevScene& sc, const FrameParams& fp, const FanLayout& L, const float* origins, uint8_t* block,
                     const int2* slot_batch, hipStream_t st) {
  if (fp.S == 0) return;
  if (sc.no > 0)
    hipLaunchKernelGGL((permeate_bvh_kernel<true>), dim3(fp.TC, fp.S), dim3(64), 0, st, sc, fp, L, origins, block, slot_batch);
  else
    hipLaunchKernelGGL((permeate_bvh_kernel<false>), dim3(fp.TC, fp.S), dim3(64), 0, st, sc, fp, L, origins, block, slot_batch);
}

}  // namespace art
