// art_trace_path.hpp — path_kernel: one bounce of the job except the nearest-hit search.
#pragma once
#include "art_trace_rays.hpp"

namespace art {

// ------------------------------------------------------------------------------------------
// Path kernel: everything of one bounce of AudioRaytracerJobBatched.Execute (:61-215) except the
// nearest-hit search (nearest_first_kernel's hits). 8 independent waves per workgroup, one 64-ray
// group each (grid-stride); the waves reserve their pair positions with one atomic per region for
// the whole workgroup (one per wave: same-line atomics serialize). MULTI (H > 1): one launch per
// bounce; the ray state (o, life | d, hits, alive) carries over in `state`, and the rays still
// alive are appended to the next bounce's live list.
// ------------------------------------------------------------------------------------------
constexpr int kPathWaves = 8;

template <bool HITS, bool MULTI>
__global__ __launch_bounds__(64 * kPathWaves) __attribute__((amdgpu_waves_per_eu(4))) void path_kernel(
    DevScene sc, FrameParams fp, FanLayout L, const float* __restrict__ origins, uint8_t* __restrict__ block,
    const int* __restrict__ ray_order, VisPairs vp, uint32_t* __restrict__ pair_count,
    const int2* __restrict__ pre_hits, float4* __restrict__ state, int step, int emit_echo) {
  constexpr int K = kPathWaves;
  __shared__ uint32_t s_agg[2][K][2];
  __shared__ uint32_t s_aggb[2][2];
  __shared__ uint32_t s_live[2][K], s_liveb[2];
  int agg_round = 0;  // block-uniform reservation round (the LDS buffers alternate by its parity)
  __builtin_amdgcn_s_setprio(3);  // on the critical path; in multi-hit frames the echo traversal runs beside it
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nrb = (fp.R + 63) >> 6;  // 64-ray groups per fan
  const int ngroups = fp.S * nrb;
  const int T = fp.T, H = MULTI ? fp.H : 1;
  const unsigned long long lt = (1ull << lane) - 1ull;
  // one reservation for the workgroup: returns this wave's base in each of the two regions
  auto reserve = [&](uint32_t n0, uint32_t n1, uint32_t* counter, uint32_t& b0, uint32_t& b1) {
    const int par = agg_round++ & 1;
    if (lane == 0) { s_agg[par][w][0] = n0; s_agg[par][w][1] = n1; }
    __syncthreads();
    if (threadIdx.x < 2) {
      uint32_t t = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) t += s_agg[par][k][threadIdx.x];
      s_aggb[par][threadIdx.x] = t ? atomicAdd(&counter[threadIdx.x], t) : 0u;
      if (MULTI && threadIdx.x == 0 && t) atomicAdd(echo_counts(state, ngroups) + step, t);  // bounce step's echoes
    }
    __syncthreads();
    b0 = s_aggb[par][0];
    b1 = s_aggb[par][1];
    for (int k = 0; k < w; ++k) { b0 += s_agg[par][k][0]; b1 += s_agg[par][k][1]; }
  };
  for (int g = (int)blockIdx.x * K + w;; g += (int)gridDim.x * K) {
    if (g - w >= ngroups) break;  // block-uniform: a wave past the end takes part with no rays
    const bool gvalid = g < ngroups;
    const int fan = gvalid ? g / nrb : 0;
    const int slot = gvalid ? (g - fan * nrb) * 64 + lane : fp.R;
    const bool valid = slot < fp.R;
    const int ray = valid ? ray_order[slot] : 0;
    uint8_t* fb = block + (size_t)fan * L.stride;
    uint16_t* echo = reinterpret_cast<uint16_t*>(fb + L.echo_off);
    art_half3* hpo = reinterpret_cast<art_half3*>(fb + L.hit_points_off);
    uint32_t* hid = reinterpret_cast<uint32_t*>(fb + L.hit_ids_off);
    const bool single_slot = fp.TC == 1;
    const int my_slot = (int)(((long long)((ray / fp.bs) * fp.bs) * fp.TC) / fp.R);  // batchId (:63-64)

    // Reset (:72-80) with sequential-batch semantics (TC > 1 only; at TC == 1 every slot is written
    // once below): frozen bit k = a later batch resets this ray's slot k.
    uint32_t frozen = 0;
    if (valid) {
      const int my_batch = ray / fp.bs;
      const art_half3 z = {0, 0, 0};
      for (int k = 0; k < H; ++k) {
        const int j = ray * H + k;
        bool any_reset;
        const int keep = batch_slot_state(fp, j, my_batch, any_reset);
        if (!keep) frozen |= 1u << k;
        if (!single_slot && (!keep || any_reset) && step == 0) {
          echo[j] = 0;
          if (HITS) { hpo[j] = z; hid[j] = ART_HIT_NONE; }
        }
      }
    }

    const vec3 O = load3(origins, fan);
    vec3 o = O;
    vec3 d = load_dir(sc.dirs, valid ? ray : 0);
    float life = fp.max_life;
    int hits = 0;
    bool alive = valid;
    const size_t sidx = (size_t)g * 64 + lane;  // ray slot of the state / hit arrays
    if (MULTI && step > 0 && valid) {
      const float4 a = state[2 * sidx], b = state[2 * sidx + 1];
      o = mk3(a.x, a.y, a.z);
      life = a.w;
      d = mk3(b.x, b.y, b.z);
      hits = __float_as_int(b.w) & 0xff;
      alive = ((__float_as_int(b.w) >> 8) & 1) != 0;
    }
    const bool alive0 = alive;

    // this bounce's nearest hit (nearest_first_kernel)
    const Seg s = make_seg(o, d);
    const int2 ph = gvalid ? pre_hits[sidx] : make_int2(__float_as_int(FLT_MAX), kNoHit);
    const int bc = ph.y;
    const bool hit = alive && bc != kNoHit;
    alive = hit;  // a miss ends the ray (:200-207)
    int type = kNone, idx = 0;
    float dist = __int_as_float(ph.x);
    if (hit) {
      winner_of(sc, s, bc, type, idx, dist);
      o = o + d * dist;  // :111
      life -= dist;      // :112
      hits += 1;         // :113
    }
    const int k = hits - 1;
    const bool live_slot = hit && !((frozen >> k) & 1u);
    if (HITS && live_slot) {  // :118, :197
      art_half3 p;
      p.x = f32tof16(o.x); p.y = f32tof16(o.y); p.z = f32tof16(o.z);
      hpo[ray * H + k] = p;
      hid[ray * H + k] = ART_HIT_ID(type, idx);  // ShootRayCast's (hitColliderType, collider) :225-280
    }

    // the echo ray to the fan origin (:124-145), emitted into a live slot only (:118), and the hit
    // record the T muffle rays start from (:150-173); one reservation for the workgroup
    const vec3 off = o - d * kEps;                 // :124, :158
    const float dist0 = distance(O, o);            // :130 (un-offset hit point)
    {
      const unsigned long long me = __builtin_amdgcn_ballot_w64(live_slot), mr = __builtin_amdgcn_ballot_w64(hit);
      exec_add(fp.exec, kExecEchoPairs, (unsigned long long)__popcll(me));
      uint32_t eb, rb;
      reserve(emit_echo ? (uint32_t)__popcll(me) : 0u, (uint32_t)__popcll(mr), pair_count, eb, rb);
      if (emit_echo && live_slot) {
        const uint32_t at = eb + (uint32_t)__popcll(me & lt);
        const vec3 qdir = normalize(O - off);
        vp.seg[2 * (size_t)at] = make_float4(off.x, off.y, off.z, dist0);
        vp.seg[2 * (size_t)at + 1] = make_float4(qdir.x, qdir.y, qdir.z, __int_as_float(kNoOwner));
        vp.out[at] = make_uint2((uint32_t)(((size_t)fan * L.stride + L.echo_off) / 2) + (uint32_t)(ray * H + k),
                                f32tof16(dist0 * echo_of(sc, type, idx)));  // :142-144
      }
      if (hit) {
        const uint32_t at = rb + (uint32_t)__popcll(mr & lt);
        vp.hrec[at] = make_float4(off.x, off.y, off.z, __uint_as_float((uint32_t)(((size_t)fan * fp.TC + my_slot) * T)));
      }
    }
    // a blocked echo leaves the reset value (:76); the echo traversal overwrites the visible ones
    // (or, tracing from the hits (!emit_echo), writes both itself)
    if (emit_echo && live_slot && single_slot) echo[ray * H + k] = 0;

    // termination / reflection — :179-193, ReflectRay :456-532
    if (!MULTI) {
      alive = false;  // hits >= H == 1 after the first hit; a miss has already ended the ray
    } else if (hit) {
      if (hits >= H || life <= 0.0f) {
        alive = false;
      } else {
        alive = reflect_at_hit(sc, fp, type, idx, o, d, life);
      }
    }
    if (MULTI) {
      if (valid) {  // the next launch's ray state (a ray that stopped records alive = 0)
        state[2 * sidx] = make_float4(o.x, o.y, o.z, life);
        state[2 * sidx + 1] = make_float4(d.x, d.y, d.z, __int_as_float(hits | (alive ? 256 : 0)));
      }
      // the rays still alive: the next bounce's traversal list (one reservation per workgroup)
      uint32_t* live = live_list(state, ngroups);
      uint32_t* live_n = live + (size_t)ngroups * 64;
      const bool app = valid && alive && step + 1 < fp.H;
      const unsigned long long m = __builtin_amdgcn_ballot_w64(app);
      const int par = agg_round++ & 1;
      if (lane == 0) s_live[par][w] = (uint32_t)__popcll(m);
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int kk = 0; kk < K; ++kk) t += s_live[par][kk];
        s_liveb[par] = t ? atomicAdd(&live_n[step + 1], t) : 0u;
      }
      __syncthreads();
      uint32_t base = s_liveb[par];
      for (int kk = 0; kk < w; ++kk) base += s_live[par][kk];
      if (app) live[base + (uint32_t)__popcll(m & lt)] = (uint32_t)sidx;
    }
    if (valid && (!MULTI || (alive0 && !alive))) {  // in the launch where the ray stops
      if (single_slot) {  // slots past the last hit keep the reset value 0 (:72-80)
        const art_half3 z = {0, 0, 0};
        for (int kk = hits; kk < H; ++kk) {
          echo[ray * H + kk] = 0;
          if (HITS) { hpo[ray * H + kk] = z; hid[ray * H + kk] = ART_HIT_NONE; }
        }
      }
      if (HITS) fb[L.hit_counts_off + ray] = (uint8_t)hits;  // :204, :212
    }
  }
}

}  // namespace art
