// art_trace.hip — the throughput raytrace stage (AudioRaytracerJobBatched.Execute,
// Jobs/AudioRaytracerJobBatched.cs:61-215) on gfx950.
//
// One frame of S fans x R rays is, per bounce k = 0 .. H-1:
//   nearest_first_kernel  nearest hit of every live ray segment (ShootRayCast :225-280) by a
//                         quad-per-ray traversal of the collider BVH (art_bvh.hip);
//   path_kernel           the exact re-evaluation of the winner, the hit point, the echo pair
//                         (:121-145) and the hit record of the muffle rays (:150-173) and, for
//                         multi-hit frames, the reflection / termination (:179-193, ReflectRay
//                         :456-532) and the ray state of the next bounce;
//   vis_kernel            (side stream) the bounce's echo rays (CanRaySeePoint :365-397) by quad
//                         BVH any-hit traversal; a visible echo is stored at once;
// then, once for the frame:
//   muffle_kernel         every hit's muffle rays (CanRaySeeAudioTarget :405-449) against the
//                         target's direction-cell candidate lists (art_cells.hip), visible rays
//                         counted into the muffle accumulators.
// Every output equals the reference's bit for bit: the broad phases are exact, the
// nearest hit is the (distance, reference order) minimum, any-hit verdicts are ORs.
// The kernels: art_trace_{nearest,path,echo,muffle}.hpp (echo_muffle_kernel in the last), over
// art_trace_rays.hpp and art_quad.hpp; here: the pair buffer, the launch plan, the launches. Permeation: art_permeate.hip.

// Build switches (everything else is a constant: the settled A/B questions are in DESIGN.md §4).
//   ART_DIAG / ART_WAVE_TIMES  diagnostic builds (tools/diag_*.sh; tools/wt_*.sh, tools/wave_times.py)
//   ART_MEASURE_PARTS  measurement builds, wrong outputs: 1 = no muffle rays in echo_muffle_kernel, 2 = no echo rays
//   ART_REPLAY_DEAL    1: a wave's replayed leaf tests are dealt over its quads; 0: each quad tests its own record
#ifndef ART_MEASURE_PARTS
#define ART_MEASURE_PARTS 0
#endif
#ifndef ART_REPLAY_DEAL
#define ART_REPLAY_DEAL 1
#endif

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "art_trace_echo.hpp"
#include "art_trace_muffle.hpp"
#include "art_trace_nearest.hpp"
#include "art_trace_path.hpp"

namespace art {

// Pair buffer: echo segments | echo outputs | hit records | first-segment hits | ray state + live
// list (multi-hit).
struct PairBufs {
  VisPairs vp;
  int2* pre;        // [groups * 64] nearest hits of the current bounce
  uint16_t* elog;   // [groups * 64][16] leaf records of the bounce-0 cast (one-hit frames with one batch slot: EchoLog)
  float4* state;    // [groups * 64][2] ray state between the bounce launches (multi-hit frames)
  size_t total;
};

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t echo_cap_of(const FrameParams& fp) { return ((size_t)fp.S * fp.R * fp.H + 63) & ~(size_t)63; }

static PairBufs pair_bufs(void* base, const FrameParams& fp) {
  PairBufs b{};
  const size_t slots = (size_t)fp.S * ((fp.R + 63) / 64) * 64;
  // (multi-hit frames: room for the fixed per-bounce slots of the folded path, H * slots records)
  // (and for the one-hit fused plan's records at fixed slots: `slots` of them, past S * R when R % 64 != 0)
  const size_t ecap = std::max(echo_cap_of(fp), slots * fp.H), hcap = std::max((size_t)fp.S * fp.R * fp.H, slots * fp.H);
  uint8_t* p = static_cast<uint8_t*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) { uint8_t* q = p ? p + off : nullptr; off += align256(bytes); return q; };
  b.vp.seg = reinterpret_cast<float4*>(take(ecap * 32));
  b.vp.out = reinterpret_cast<uint2*>(take(ecap * 8));
  b.vp.hrec = reinterpret_cast<float4*>(take(hcap * 16));
  b.vp.echo_cap = (uint32_t)ecap;
  b.pre = reinterpret_cast<int2*>(take(slots * sizeof(int2)));
  if (fp.H == 1 && fp.TC == 1) b.elog = reinterpret_cast<uint16_t*>(take(slots * 32));
  if (fp.H > 1) b.state = reinterpret_cast<float4*>(take(slots * (2 * sizeof(float4) + 4) + 2 * kLiveCounters * 4));
  b.total = off;
  return b;
}

size_t fast_pair_bytes(const FrameParams& fp) { return pair_bufs(nullptr, fp).total; }

// Fans per launch_raytrace_fast call: echo pairs and hit records (R*H per fan each) stay below
// 2^31 (u32 indices), the muffle accumulator index (fan * TC + slot) * T + t fits 32 bits, and a
// fan's echo halves stay addressable with a 32-bit half offset into the block
// (fan * stride / 2 < 2^32).
int fast_fans_per_launch(int R, int H, int T, int TC, uint32_t stride) {
  const unsigned long long per_fan = (unsigned long long)R * H + 64;
  const unsigned long long by_pairs = ((1ull << 31) - 64) / per_fan;
  const unsigned long long by_dest = ((1ull << 32) - 1) / ((unsigned long long)(TC > 0 ? TC : 1) * (T > 0 ? T : 1));
  const unsigned long long by_block = ((1ull << 33) - 1) / (stride ? stride : 1) - 1;
  unsigned long long n = std::min(std::min(std::min(by_pairs, by_dest), by_block), (unsigned long long)(1 << 24));
  if (const char* e = getenv("ART_FAST_CHUNK_FANS")) {  // test hook: force small chunks
    const long long v = atoll(e);
    if (v > 0) n = std::min(n, (unsigned long long)v);
  }
  return (int)std::max(1ull, n);
}

// An event pair around one launch (marks may be null); a launch past the pairs is counted as dropped.
template <class F>
static void marked(KernelMarks* marks, int kind, hipStream_t s, F&& launch) {
  const bool m = marks && marks->used < marks->cap;
  if (marks && !m) marks->dropped++;
  if (m) { marks->kind[marks->used] = kind; (void)hipEventRecord(marks->ev[2 * marks->used], s); }
  launch();
  if (m) { (void)hipEventRecord(marks->ev[2 * marks->used + 1], s); marks->used++; }
}

// f(std::bool_constant<a>{}, std::bool_constant<b>{}): a launch written once as a generic lambda, four instantiations.
template <class F>
static void with_flags(bool a, bool b, F&& f) {
  if (a) { if (b) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
  else { if (b) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}

static int device_cus() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
  return n > 0 ? n : 256;
}

// What one launch_raytrace_fast call launches: the plan's decisions and its grid numbers (no launches here).
struct TracePlan {
  bool split, multi, hm, fused, fold, per_bounce, tab, logp, obb, ex;
  unsigned groups, path_blocks;  // 64-ray groups; path_kernel workgroups
  unsigned echo_batches;         // vis_kernel workgroups when it runs over the emitted pairs
  unsigned mblocks, mt;          // muffle ray blocks x targets over the grid (the targets past mt are looped)
  // the plan taken (art_debug_last_plan): the branch of the launch chain, then the switches on top
  uint32_t bits() const {
    return (per_bounce ? (fold ? ART_PLAN_FOLD : ART_PLAN_PER_BOUNCE) : fused ? ART_PLAN_FUSED : hm ? ART_PLAN_HM
            : split ? ART_PLAN_SPLIT : 0u) |
           (tab ? ART_PLAN_TAB : 0u) | (obb ? ART_PLAN_OBB : 0u) | (ex ? ART_PLAN_EX : 0u);
  }
};

static TracePlan trace_plan(const DevScene& sc, const FrameParams& fp, const FanLayout& L, const PairBufs& pb, bool side_stream) {
  TracePlan p{};
  p.groups = (unsigned)((size_t)fp.S * ((fp.R + 63) / 64));
  p.obb = sc.no > 0;  // OBB-free scenes run instantiations without the OBB tests
  p.ex = fp.exec != nullptr;
  p.path_blocks = (p.groups + kPathWaves - 1) / kPathWaves;
  p.multi = fp.H > 1;
  p.echo_batches = pb.vp.echo_cap / 64;  // (one workgroup each)
  p.split = side_stream;
  static const int cus = device_cus();
  // One-hit frames with one batch slot and hit outputs trace the echo rays straight from the nearest
  // hits (HM) when the frame's echo traversal fits the chip in one round of waves (4 per 64-ray group, 8 per
  // SIMD): a larger one would hold every wave slot and starve the path kernel beside it (config 4:
  // path 30 -> 977 us).
  p.hm = p.split && !p.multi && fp.TC == 1 && L.has_hits && p.groups <= (unsigned)cus * 8u;
  // One-hit frames with one batch slot and no hit outputs (the fused plan): no path kernel at all. The
  // cast's epilogue stores each ray slot's hit record and echo half (fold_path<true>: the misses'
  // reset too), and the echo traversal and the muffle rays start from the records as one launch on
  // st (echo_muffle_kernel), at any frame size (no path kernel is left to starve; config 4 1.684 ->
  // 1.660 ms/step)
  p.fused = p.split && !p.multi && fp.TC == 1 && !L.has_hits;
  // Multi-hit frames with one batch slot and no hit outputs fold the path kernel into the nearest
  // kernel (nearest_first_kernel<..., FOLD>): records at fixed per-bounce slots, no live list
  p.fold = p.split && p.multi && fp.TC == 1 && !L.has_hits;
  p.per_bounce = p.split && p.multi && pb.state;  // each bounce's echo traversal on the side stream (per-bounce echo counts)
  const size_t hcap = (size_t)fp.S * fp.R * fp.H;
  p.mblocks = (ART_MEASURE_PARTS == 1 && p.fused) ? 0u : p.fused ? (p.groups + 3) / 4
                  : (unsigned)(((p.fold ? (size_t)p.groups * 64 * fp.H : hcap) + 255) / 256);  // ray slots / hit records
  p.mt = (unsigned)std::min(fp.T, 64);
  // bounce 0 with the shared-origin node table (nearest_first_kernel<..., TAB>) when a fan's 64-ray
  // groups come in fours, the BVH fits the table and the scene has OBBs. Measured (round 6, A/B of
  // per-kernel HIP-event times): config 3 (4096 OBBs) nearest 68.4 -> 63.3 us, config 5 even; in
  // OBB-free scenes the 1024-lane workgroups and the table build cost more than the table saves
  // (config 2 nearest 50.8 -> 53.6 us), so they keep the 256-lane kernel.
  p.tab = sc.no > 0 && ((fp.R + 63) / 64) % 4 == 0 && sc.bvh_levels > 0 && (long long)sc.bvh_leaf0 * 4 + 1 <= kTabNodes;
  // The fused plan's bounce-0 cast logs the leaves it tests and the echo waves replay them (EchoLog;
  // not the counting instantiations; leaf ids are 16-bit: up to 65536 leaves). OBB-free scenes only,
  // by measurement: with OBBs the wider node margins cost the cast more than the echo
  // waves save (config 3 0.1526 -> 0.1547 ms/step, config 4 1.019 -> 1.102).
  p.logp = p.fused && !p.ex && !p.obb && !p.tab && pb.elog && sc.bvh_levels > 0 && 3ll * sc.bvh_leaf0 + 1 <= 65536;
  return p;
}

uint32_t launch_raytrace_fast(const DevScene& sc, const FrameParams& fp, const FanLayout& L, const float* origins,
                              uint8_t* block, uint32_t* muffle_acc, const int* ray_order, void* pair_buf, uint32_t* pair_count,
                              hipStream_t st, const SideStream& echo, KernelMarks* marks, bool first_chunk) {
  if (fp.S == 0) return 0;
  PairBufs pb = pair_bufs(pair_buf, fp);
  const TracePlan p = trace_plan(sc, fp, L, pb, echo.st != nullptr);
  const unsigned groups = p.groups;
  const uint32_t nacc = (uint32_t)((size_t)fp.S * fp.TC * fp.T);  // this chunk's muffle accumulators
  uint32_t* ecnt = pb.state ? echo_counts(pb.state, (int)groups) : nullptr;  // per-bounce echo counts
  // (the fused plan's records sit at the folded path's fixed slots, bounce 0 only)
  pb.vp.fixed = p.fold || p.fused ? groups * 64u : 0u;
  EchoFromHits eh;
  eh.fp = fp; eh.L = L; eh.origins = origins; eh.ray_order = ray_order; eh.pre = pb.pre;
  EchoLog el;
  el.rec = p.logp ? pb.elog : nullptr;
  el.count = pair_count ? reinterpret_cast<unsigned long long*>(pair_count + 4) : nullptr;  // (after the 4 pair counters)
  el.keep_count = first_chunk ? 0 : 1;

  // The launches, each once (EX, OBB, ...: std::bool_constant values). Bounce k's cast; TAB: 4 groups of a fan per workgroup.
  auto nearest = [&](int k, auto EX, auto OBB, auto FOLD, auto TAB, auto LOG) {
    hipLaunchKernelGGL((nearest_first_kernel<EX.value, OBB.value, FOLD.value, TAB.value, LOG.value>),
                       dim3(TAB.value ? groups / 4 : groups), dim3(TAB.value ? 1024 : 256), 0, st, sc, fp, origins, ray_order,
                       pb.pre, pb.state, k, muffle_acc, k == 0 ? nacc : 0u, k == 0 ? pair_count : nullptr, L, block, pb.vp, el);
  };
  auto path = [&](hipStream_t s, int k) {
    with_flags(L.has_hits, p.multi, [&](auto HITS, auto MULTI) {
      hipLaunchKernelGGL((path_kernel<HITS.value, MULTI.value>), dim3(p.path_blocks), dim3(64 * kPathWaves), 0, s, sc, fp, L,
                         origins, block, ray_order, pb.vp, pair_count, pb.pre, pb.state, k, (int)!p.hm);
    });
  };
  // The echo traversal of `blocks` 64-pair batches (bounce >= 0: those that bounce emitted); HM: from the hits.
  auto vis = [&](hipStream_t s, unsigned blocks, int bounce, auto HM) {
    with_flags(p.ex, p.obb, [&](auto EX, auto OBB) {
      hipLaunchKernelGGL((vis_kernel<EX.value, OBB.value, HM.value>), dim3(blocks), dim3(256), 0, s, sc, pb.vp, pair_count,
                         EX.value ? fp.exec : nullptr, ecnt, bounce, block, eh);
    });
  };
  // (the standalone muffle kernel never runs the fused plan's records: HM = false)
  auto muffle = [&](hipStream_t s) {
    with_flags(p.ex, p.obb, [&](auto EX, auto OBB) {
      hipLaunchKernelGGL((muffle_kernel<EX.value, OBB.value, false>), dim3(p.mblocks, p.mt), dim3(256), 0, s, sc, fp, pb.vp,
                         pair_count, muffle_acc, eh);
    });
  };
  auto echo_muffle = [&] {
    with_flags(p.ex, p.obb, [&](auto EX, auto OBB) {
      hipLaunchKernelGGL((echo_muffle_kernel<EX.value, OBB.value>), dim3(4 * (groups + p.mblocks * p.mt)), dim3(64), 0, st, sc, fp,
                         pb.vp, pair_count, EX.value ? fp.exec : nullptr, block, eh, muffle_acc, groups, p.mblocks, (int)p.mt, el);
    });
  };

  // Stream plan. Multi-hit frames: per bounce nearest → path on st, that bounce's echo traversal
  // on the side stream right after its path kernel (beside the next bounces' nearest traversals,
  // whose tails leave CUs idle), the muffle kernel after the last bounce on st. One-hit frames
  // with one batch slot and hit outputs (HM): nearest → echo traversal from the hits on st, path → muffle on the
  // side stream (the path kernel leaves the critical path); without hit outputs (fused): nearest →
  // echo_muffle_kernel on st. Other one-hit frames: nearest → path →
  // echo traversal on st, the muffle kernel on the side stream (the longer kernel stays on st: a
  // fork costs ~10 us before the side stream starts). Without a side stream everything runs on st.
  for (int k = 0; k < (p.multi ? fp.H : 1); ++k) {
    marked(marks, kMarkNearest, st, [&] {
      if (p.logp && k == 0) {
        nearest(k, std::false_type{}, std::false_type{}, std::false_type{}, std::false_type{}, std::true_type{});
      } else {
        with_flags(p.ex, p.obb, [&](auto EX, auto OBB) {
          with_flags(p.fold, p.tab && k == 0, [&](auto FOLD, auto TAB) { nearest(k, EX, OBB, FOLD, TAB, std::false_type{}); });
        });
      }
    });
    hipStream_t pst = st;
    if (p.hm) {
      (void)hipEventRecord(echo.fork, st);
      (void)hipStreamWaitEvent(echo.st, echo.fork, 0);
      pst = echo.st;
    }
    if (!p.fused && !p.fold) path(pst, k);
    if (p.per_bounce) {  // this bounce's echoes (at most one per ray slot: `groups` batches)
      (void)hipEventRecord(echo.fork, st);
      (void)hipStreamWaitEvent(echo.st, echo.fork, 0);
      marked(marks, kMarkEcho, echo.st, [&] { vis(echo.st, groups, k, std::false_type{}); });
    }
  }
  if (p.per_bounce) {
    marked(marks, kMarkMuffle, st, [&] { muffle(st); });  // the bounces' echoes are already on the side stream
  } else if (p.fused) {
    marked(marks, kMarkEchoMuffle, st, echo_muffle);
  } else if (p.hm) {
    marked(marks, kMarkMuffle, echo.st, [&] { muffle(echo.st); });  // after the path kernel there
    marked(marks, kMarkEcho, st, [&] { vis(st, groups, -1, std::true_type{}); });  // one 64-ray group per workgroup
  } else if (p.split) {
    (void)hipEventRecord(echo.fork, st);
    (void)hipStreamWaitEvent(echo.st, echo.fork, 0);
    marked(marks, kMarkMuffle, echo.st, [&] { muffle(echo.st); });
    marked(marks, kMarkEcho, st, [&] { vis(st, p.echo_batches, -1, std::false_type{}); });
  } else {
    marked(marks, kMarkEcho, st, [&] { vis(st, p.echo_batches, -1, std::false_type{}); });
    marked(marks, kMarkMuffle, st, [&] { muffle(st); });
  }
  if (p.split && !p.fused) {
    (void)hipEventRecord(echo.join, echo.st);
    (void)hipStreamWaitEvent(st, echo.join, 0);
  }
  return p.bits();
}

#ifdef ART_DIAG
bool diag_fetch_permeate(unsigned long long (*h)[64]);  // art_permeate.hip
extern "C" void art_diag_dump_impl() {
  unsigned long long h[4][64], hp[4][64];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_diag), sizeof h) != hipSuccess || !diag_fetch_permeate(hp)) return;
  for (int k = 0; k < 4; ++k)
    for (int b = 0; b < 64; ++b) h[k][b] += hp[k][b];
  const char* names[4] = {"nearest wave cycles", "echo wave cycles", "nearest ray steps", "echo ray steps"};
  for (int k = 0; k < 4; ++k) {
    fprintf(stderr, "[diag] %s (log2 bucket: count)", names[k]);
    for (int b = 0; b < 64; ++b)
      if (h[k][b]) fprintf(stderr, " %d:%llu", b, h[k][b]);
    fprintf(stderr, "\n");
  }
}
#endif
#ifdef ART_WAVE_TIMES
extern "C" void art_wave_times_dump_impl() {
  const char* path = getenv("ART_WAVE_TIMES_OUT");
  if (!path || hipDeviceSynchronize() != hipSuccess) return;
  static unsigned long long t[kWtCap][2];
  static uint32_t id[kWtCap][3];
  const unsigned n = 0;  // (header word kept for the reader)
  if (hipMemcpyFromSymbol(t, HIP_SYMBOL(g_wt), sizeof t) != hipSuccess ||
      hipMemcpyFromSymbol(id, HIP_SYMBOL(g_wt_id), sizeof id) != hipSuccess)
    return;
  FILE* f = fopen(path, "wb");
  if (!f) return;
  const unsigned cap = kWtCap;
  int dev = 0, khz = 0;  // wall-clock rate
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) khz = 0;
  fwrite(&n, sizeof n, 1, f);
  fwrite(&cap, sizeof cap, 1, f);
  fwrite(&khz, sizeof khz, 1, f);
  fwrite(t, sizeof t, 1, f);
  fwrite(id, sizeof id, 1, f);
  fclose(f);
}
#endif
}  // namespace art
