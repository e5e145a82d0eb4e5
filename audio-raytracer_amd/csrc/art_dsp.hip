// art_dsp.hip — per-sample spatializer DSP (include/art_dsp.h; SURVEY.md §8 f rank 1).
//
// AudioSpatializer.OnAudioFilterRead (Audio/AudioTarget/AudioSpatializer.cs:70-87) runs four
// passes over an interleaved stereo buffer: MuffleDSP (MuffleDSP.cs:13-32), ReverbDSP
// (ReverbDSP.cs:10-24), BinauralDSP (BinauralDSP.cs:15-82) and the volume multiplier. Every
// per-sample value of a pass depends only on the same sample's value after the previous pass and
// on the pass's own filter state, so the passes fuse into one loop over samples with identical
// results. The quantities the C# recomputes per sample (curve lookups, cutoffs, filter alphas)
// are constant over a buffer and are computed once on the host with the same float operations
// (art_dsp_source_params_get), or on the device from a frame's result blocks (the audio tick,
// dsp_tick_params_kernel; art_dsp_math.hpp holds the shared sequence); the GPU runs the recurrences, one lane per source, both channels
// interleaved (two independent chains per lane).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/art_dsp.h"
#include "art_dsp_math.hpp"
#include "art_internal.hpp"

#pragma clang fp contract(off)

namespace art {
namespace {

constexpr int kDspBlock = 256;

// One lane per source; both channels. data: this source's interleaved frames.
__global__ __launch_bounds__(kDspBlock) void dsp_kernel(float* __restrict__ data, const long long* __restrict__ offsets,
                                                        const int* __restrict__ frames_of, int frames_all,
                                                        const art_dsp_source_params* __restrict__ params,
                                                        art_dsp_state* __restrict__ state, int count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= count) return;
  const art_dsp_source_params p = params[s];
  if (p.flags & 4) return;  // not stereo: left as is (AudioSpatializer.cs:72)
  const int frames = frames_of ? frames_of[s] : frames_all;
  float* d = data + (offsets ? offsets[s] : (long long)s * frames_all * 2);
  art_dsp_state st = state[s];
  const bool muffle = (p.flags & 1) != 0, lp = (p.flags & 2) != 0;
  float pmL = st.previous_muffle.left, pmR = st.previous_muffle.right;
  float plL = st.previous_lp.left, plR = st.previous_lp.right;
  float phL = st.previous_hp.left, phR = st.previous_hp.right;
  float piL = st.previous_input.left, piR = st.previous_input.right;
  auto sample = [&](float& l, float& r) {
    if (muffle) {  // MuffleDSP.LowPass :43-44
      pmL += p.muffle_alpha * (l - pmL); l = pmL;
      pmR += p.muffle_alpha * (r - pmR); r = pmR;
    }
    l = l * p.dry_boost;  // ReverbDSP :21-22
    r = r * p.dry_boost;
    l = l * p.gain_left;  // BinauralDSP :59-60
    r = r * p.gain_right;
    if (lp) {  // LowPass :92-93
      plL += p.filter_alpha * (l - plL); l = plL;
      plR += p.filter_alpha * (r - plR); r = plR;
    } else {   // HighPass :102-105
      const float oL = p.filter_alpha * (phL + l - piL);
      piL = l; phL = oL; l = oL;
      const float oR = p.filter_alpha * (phR + r - piR);
      piR = r; phR = oR; r = oR;
    }
    l = l * p.volume;  // AudioSpatializer.cs:84-85
    r = r * p.volume;
  };
  int i = 0;
  if ((reinterpret_cast<uintptr_t>(d) & 15) == 0) {
    float4* d4 = reinterpret_cast<float4*>(d);
    for (; i + 2 <= frames; i += 2) {
      float4 v = d4[i >> 1];
      sample(v.x, v.y);
      sample(v.z, v.w);
      d4[i >> 1] = v;
    }
  }
  for (; i < frames; ++i) {
    float l = d[2 * i], r = d[2 * i + 1];
    sample(l, r);
    d[2 * i] = l;
    d[2 * i + 1] = r;
  }
  st.previous_muffle.left = pmL; st.previous_muffle.right = pmR;
  st.previous_lp.left = plL; st.previous_lp.right = plR;
  st.previous_hp.left = phL; st.previous_hp.right = phR;
  st.previous_input.left = piL; st.previous_input.right = piR;
  state[s] = st;
}

// ---- tiled kernel: one lane per (source, channel), tiles transposed through LDS -------------
//
// The recurrences are serial over frames, so a lane owns one channel chain. The buffers are
// [source][frame][L,R]: a wave reads a tile of kTF frames of its kTS sources with coalesced 8-B
// loads (one instruction covers 256 contiguous bytes of two sources), transposes it through LDS,
// runs the chains out of LDS, and writes the tile back the same way. The next tile's loads are in
// flight while the current one is processed.
#ifndef ART_DSP_TF
#define ART_DSP_TF 64
#endif
constexpr int kTS = 32;              // sources per wave (lane = 2 * source + channel)
constexpr int kTF = ART_DSP_TF;      // frames per tile (64; 32 measured slower on large batches)
constexpr int kSPI = 64 / kTF;       // sources covered by one load instruction
static_assert(kTF == 32 || kTF == 64, "tile width");
constexpr int kRow = 2 * kTF + 2;    // floats per LDS row: bank (2 s + c + 2 n) mod 32 is distinct per half-wave
constexpr int kLoads = kTS * kTF / 64;  // float2 loads per lane per tile

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// Chain and step<M> (the per-sample operation sequence of one channel): art_dsp_math.hpp.

// n frames of one channel's chain from LDS row `in` to LDS row `out` (the same row in
// dsp_tiled_kernel; a shared dry row and the source's own wet row in dsp_mix_kernel).
template <int M>
__device__ __forceinline__ void run_tile(const float* in, float* out, int n, const art_dsp_source_params& p,
                                         float gain, bool mf, bool lp, Chain& c) {
  if (n == kTF) {
    float x[kTF];
#pragma unroll
    for (int k = 0; k < kTF; ++k) x[k] = in[2 * k];
#pragma unroll
    for (int k = 0; k < kTF; ++k) x[k] = step<M>(x[k], p, gain, mf, lp, c);
#pragma unroll
    for (int k = 0; k < kTF; ++k) out[2 * k] = x[k];
  } else {
    for (int k = 0; k < n; ++k) out[2 * k] = step<M>(in[2 * k], p, gain, mf, lp, c);
  }
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(64) void dsp_tiled_kernel(float* __restrict__ data, const long long* __restrict__ offsets,
                                                       const int* __restrict__ frames_of, int frames_all,
                                                       const art_dsp_source_params* __restrict__ params,
                                                       art_dsp_state* __restrict__ state, int count,
                                                       uint32_t nbytes) {
  __shared__ float tile[kTS * kRow];
  const int lane = threadIdx.x;
  const int s0 = blockIdx.x * kTS;
  const int sl = lane >> 1, ch = lane & 1;
  const int s = s0 + sl;
  art_dsp_source_params p{};
  int my_frames = 0;
  Chain c{};
  if (s < count) {
    p = params[s];
    if (!(p.flags & 4)) {
      my_frames = frames_of ? frames_of[s] : frames_all;
      const float* sv = reinterpret_cast<const float*>(state + s);
      c.pm = sv[0 + ch]; c.pl = sv[2 + ch]; c.ph = sv[4 + ch]; c.pi = sv[6 + ch];
    }
  }
  const bool mf = (p.flags & 1) != 0, lp = (p.flags & 2) != 0;
  const float gain = ch ? p.gain_right : p.gain_left;
  const int cls = my_frames > 0 ? (p.flags & 3) : -1;
  const int fmax = wave_max_i(my_frames);
  if (fmax == 0) return;
  const uint64_t b0 = __ballot(cls == 0), b1 = __ballot(cls == 1), b2 = __ballot(cls == 2), b3 = __ballot(cls == 3);
  const bool generic = (b0 != 0) + (b1 != 0) + (b2 != 0) + (b3 != 0) >= 3;

  // loader view: item i of this lane is frame lane % kTF of local source kSPI * i + lane / kTF.
  // Buffer loads/stores with the hardware range check: an item past its source's frames gets the
  // offset nbytes (loads 0, store dropped), so the transfers are branch-free and the wait for the
  // next tile's loads does not also wait for this tile's stores.
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(data, 0, (int)nbytes, 0x00020000);
  const int lf = lane & (kTF - 1);
  // per-source frames and byte offset come from the source's channel-0 lane (no dependent loads)
  const long long my_off = my_frames > 0 ? (offsets ? offsets[s] : (long long)s * frames_all * 2) : 0;
  const int my_ob = (int)(uint32_t)(my_off * 4);
  uint32_t obase[kLoads];
  int lfr[kLoads];
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    const int src_lane = 2 * (kSPI * i + lane / kTF);
    lfr[i] = __shfl(my_frames, src_lane, 64);
    obase[i] = (uint32_t)__shfl(my_ob, src_lane, 64);
  }
  u32x2 pre[kLoads];
  auto voff = [&](int i, int t) -> uint32_t {
    const int f = t * kTF + lf;
    return f < lfr[i] ? obase[i] + (uint32_t)f * 8u : nbytes;
  };
  auto load = [&](int t) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i) pre[i] = __builtin_amdgcn_raw_buffer_load_b64(rs, voff(i, t), 0, 0);
  };
  const int ntiles = (fmax + kTF - 1) / kTF;
  float* row = tile + sl * kRow + ch;
  load(0);
  // 16 out-of-range stores (dropped by the range check): the loop is then entered with the same
  // memory-op order as its back edge (loads, then stores), so the wait for the prefetched tile at
  // the loop head leaves the previous tile's stores in flight (vmcnt(16), not vmcnt(0))
#pragma unroll
  for (int i = 0; i < kLoads; ++i) __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, rs, nbytes + 16u * i, 0, 0);
  for (int t = 0; t < ntiles; ++t) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i)
      *reinterpret_cast<u32x2*>(tile + (kSPI * i + lane / kTF) * kRow + 2 * lf) = pre[i];
    __syncthreads();
    load(t + 1);  // past the last tile every offset is out of range: loads 0, no branch
    const int n = min(max(my_frames - t * kTF, 0), kTF);
    if (generic) {
      run_tile<4>(row, row, n, p, gain, mf, lp, c);
    } else {
      if (b0 && cls == 0) run_tile<0>(row, row, n, p, gain, mf, lp, c);
      if (b1 && cls == 1) run_tile<1>(row, row, n, p, gain, mf, lp, c);
      if (b2 && cls == 2) run_tile<2>(row, row, n, p, gain, mf, lp, c);
      if (b3 && cls == 3) run_tile<3>(row, row, n, p, gain, mf, lp, c);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const u32x2 v = *reinterpret_cast<const u32x2*>(tile + (kSPI * i + lane / kTF) * kRow + 2 * lf);
      __builtin_amdgcn_raw_buffer_store_b64(v, rs, voff(i, t), 0, 0);
    }
    __syncthreads();
  }
  if (my_frames > 0) {
    float* sv = reinterpret_cast<float*>(state + s);
    sv[0 + ch] = c.pm; sv[2 + ch] = c.pl; sv[4 + ch] = c.ph; sv[6 + ch] = c.pi;
  }
}

// ---- listener mix: one dry buffer per target in, one mix per fan out -------------------------
//
// dsp_tiled_kernel's skeleton with shared input and summed output. Source s = f * T + t reads the
// dry row of target t (float[T][frames][2], shared by every fan) and fan f's listener hears
//   mix[f] = ((y[f,0] + y[f,1]) + ...) + y[f,T-1]     fp32, one add per target, ascending t,
// starting from y[f,0] itself. A wave carries G = 32 / T whole fans (T <= 32; the 32 - G T left-over
// source slots idle) or one fan in rounds of 32 targets (T > 32). Per tile of kTF frames:
//   load   the round's dry rows, one 8-B-per-lane buffer load of kTF frames each, into LDS;
//   chain  lane (slot, channel) runs its chain from dry row t (lanes of different fans read the same
//          address: a broadcast) into its own padded wet row;
//   mix    lane k takes frame k as a float2 and sums each fan's rows serially in target order (8-B
//          LDS reads at unit lane stride), then one coalesced 8-B-per-lane store per fan.
// Round r > 0 of a fan reads the mix back as the accumulator and continues the same serial chain
// with targets 32 r .., so the bits are the definition's at any T. Only this wave wrote those bytes:
// no atomics, no wait for another workgroup, nothing that depends on scheduling.
__global__ __launch_bounds__(64) void dsp_mix_kernel(const float* __restrict__ dry,
                                                     const art_dsp_source_params* __restrict__ params,
                                                     art_dsp_state* __restrict__ state, float* mix, int F, int T,
                                                     int frames, uint32_t dry_bytes, uint32_t mix_bytes) {
  __shared__ float lds[2 * kTS * kRow];
  float* const dtile = lds;               // dry rows of the round (kTS rows)
  float* const wtile = lds + kTS * kRow;  // one wet row per source slot
  const int lane = threadIdx.x;
  const int sl = lane >> 1, ch = lane & 1;
  const int rowsT = min(T, kTS);  // targets per fan and round
  const int G = kTS / rowsT;      // fans per wave (1 when T > 32)
  const int g = sl / rowsT, tl = sl - g * rowsT;
  const int f0 = blockIdx.x * G;
  const int gcount = min(G, F - f0);  // fans of this wave (the last wave may be partial)
  const int rounds = (T + kTS - 1) / kTS;
  const int ntiles = (frames + kTF - 1) / kTF;
  // buffer loads/stores with the hardware range check (as in dsp_tiled_kernel): an item past
  // `frames` or past the round's rows gets the offset *_bytes: loads 0, store dropped
  const __amdgpu_buffer_rsrc_t rd =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dry), 0, (int)dry_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(mix, 0, (int)mix_bytes, 0x00020000);
  const int lf = lane & (kTF - 1);
  const float* const in = dtile + tl * kRow + ch;
  float* const out = wtile + sl * kRow + ch;

  for (int r = 0; r < rounds; ++r) {
    const int t0 = r * kTS;
    const int nrows = min(T - t0, kTS);  // dry rows of the round = rows per fan in the mix pass
    const bool active = g < gcount && tl < nrows;
    const size_t s = (size_t)(f0 + g) * T + t0 + tl;
    art_dsp_source_params p{};
    Chain c{};
    bool pass = false, run = false;
    if (active) {
      p = params[s];
      pass = (p.flags & 4) != 0;  // not stereo: the dry frames as they are, the state kept (AudioSpatializer.cs:72)
      run = !pass;
      if (run) {
        const float* sv = reinterpret_cast<const float*>(state + s);
        c.pm = sv[0 + ch]; c.pl = sv[2 + ch]; c.ph = sv[4 + ch]; c.pi = sv[6 + ch];
      }
    }
    const bool mf = (p.flags & 1) != 0, lp = (p.flags & 2) != 0;
    const float gain = ch ? p.gain_right : p.gain_left;
    const int cls = run ? (p.flags & 3) : -1;
    const uint64_t b0 = __ballot(cls == 0), b1 = __ballot(cls == 1), b2 = __ballot(cls == 2), b3 = __ballot(cls == 3);
    const bool generic = (b0 != 0) + (b1 != 0) + (b2 != 0) + (b3 != 0) >= 3;
    const bool any_pass = __ballot(pass) != 0;
    // a round reads what this wave's earlier rounds stored: those stores have completed
    if (r > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // loader view: item i of this lane is frame lane % kTF of dry row kSPI * i + lane / kTF
    u32x2 pre[kLoads];
    auto load = [&](int tile) {
      const int fr = tile * kTF + lf;
#pragma unroll
      for (int i = 0; i < kLoads; ++i) {
        const int row = kSPI * i + lane / kTF;
        const uint32_t off =
            (row < nrows && fr < frames) ? ((uint32_t)(t0 + row) * (uint32_t)frames + (uint32_t)fr) * 8u : dry_bytes;
        pre[i] = __builtin_amdgcn_raw_buffer_load_b64(rd, off, 0, 0);
      }
    };
    load(0);
    for (int tile = 0; tile < ntiles; ++tile) {
#pragma unroll
      for (int i = 0; i < kLoads; ++i)
        *reinterpret_cast<u32x2*>(dtile + (kSPI * i + lane / kTF) * kRow + 2 * lf) = pre[i];
      __syncthreads();  // also: the previous tile's mix pass has read the wet rows
      load(tile + 1);   // past the last tile every offset is out of range: loads 0, no branch
      const int n = min(frames - tile * kTF, kTF);
      if (any_pass && pass)
        for (int k = 0; k < n; ++k) out[2 * k] = in[2 * k];
      const int nr = run ? n : 0;
      if (generic) {
        run_tile<4>(in, out, nr, p, gain, mf, lp, c);
      } else {
        if (b0 && cls == 0) run_tile<0>(in, out, nr, p, gain, mf, lp, c);
        if (b1 && cls == 1) run_tile<1>(in, out, nr, p, gain, mf, lp, c);
        if (b2 && cls == 2) run_tile<2>(in, out, nr, p, gain, mf, lp, c);
        if (b3 && cls == 3) run_tile<3>(in, out, nr, p, gain, mf, lp, c);
      }
      __syncthreads();
      if (lane < kTF && rounds == 1) {  // mix pass: lane = frame of the tile, both channels
        // T <= 32: all 32 rows' reads in flight at once, then the wave's fans one after the other
        // (every branch is wave-uniform); rows past the wave's last fan are read and not used
        const int fr = tile * kTF + lane;
        float2 y[kTS];
#pragma unroll
        for (int i = 0; i < kTS; ++i) y[i] = *reinterpret_cast<const float2*>(wtile + i * kRow + 2 * lane);
        const int used = gcount * nrows;
        float2 acc = y[0];
        int k = 0, gg = 0;
#pragma unroll
        for (int i = 0; i < kTS; ++i) {
          if (i < used) {
            if (k == 0) {
              acc = y[i];  // the sum starts from y[f,0] itself
            } else {
              acc.x = acc.x + y[i].x;
              acc.y = acc.y + y[i].y;
            }
            if (++k == nrows) {
              const uint32_t off =
                  fr < frames ? ((uint32_t)(f0 + gg) * (uint32_t)frames + (uint32_t)fr) * 8u : mix_bytes;
              __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, acc), rm, off, 0, 0);
              k = 0;
              ++gg;
            }
          }
        }
      } else if (lane < kTF) {  // T > 32: one fan, round r's rows added to what the earlier rounds stored
        const int fr = tile * kTF + lane;
        for (int gg = 0; gg < gcount; ++gg) {
          const float* w = wtile + gg * rowsT * kRow + 2 * lane;
          const uint32_t off =
              fr < frames ? ((uint32_t)(f0 + gg) * (uint32_t)frames + (uint32_t)fr) * 8u : mix_bytes;
          float2 acc;
          int k = 0;
          if (r == 0) {
            acc = *reinterpret_cast<const float2*>(w);  // the sum starts from y[f,0] itself
            k = 1;
          } else {  // this lane's own store of the previous round (same lane, same address). Cast whole:
                    // with v.x / v.y taken apart the compiler emitted a 4-B load copied into both channels
            const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rm, off, 0, 0);
            acc = __builtin_bit_cast(float2, v);
          }
          for (; k < nrows; ++k) {
            const float2 y = *reinterpret_cast<const float2*>(w + k * kRow);
            acc.x = acc.x + y.x;
            acc.y = acc.y + y.y;
          }
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, acc), rm, off, 0, 0);
        }
      }
    }
    if (run) {
      float* sv = reinterpret_cast<float*>(state + s);
      sv[0 + ch] = c.pm; sv[2 + ch] = c.pl; sv[4 + ch] = c.ph; sv[6 + ch] = c.pi;
    }
  }
}

// One source's chain over `frames` interleaved stereo frames, dry -> wet, from and to its state.
template <int M>
void host_chain(const art_dsp_source_params& p, art_dsp_state& st, const float* dry, int frames, float* wet) {
  float* sv = reinterpret_cast<float*>(&st);
  for (int ch = 0; ch < 2; ++ch) {
    Chain c{sv[0 + ch], sv[2 + ch], sv[4 + ch], sv[6 + ch]};
    const float gain = ch ? p.gain_right : p.gain_left;
    for (int i = 0; i < frames; ++i) wet[2 * i + ch] = step<M>(dry[2 * i + ch], p, gain, false, false, c);
    sv[0 + ch] = c.pm; sv[2 + ch] = c.pl; sv[4 + ch] = c.ph; sv[6 + ch] = c.pi;
  }
}

}  // namespace

// The listener mix's definition (art_dsp_mix_host), literally: each source's chain, then one fp32
// add per target in ascending t, starting from y[f,0] itself.
void dsp_mix_host(const art_dsp_source_params* params, art_dsp_state* state, const float* dry, int fan_count, int T,
                  int frames, float* mix) {
  std::vector<float> wet((size_t)frames * 2);
  for (int f = 0; f < fan_count; ++f) {
    float* m = mix + (size_t)f * frames * 2;
    for (int t = 0; t < T; ++t) {
      const size_t s = (size_t)f * T + t;
      const art_dsp_source_params& p = params[s];
      const float* d = dry + (size_t)t * frames * 2;
      const float* y = wet.data();
      if (p.flags & 4) {
        y = d;  // not stereo: the dry frames as they are, the state kept (AudioSpatializer.cs:72)
      } else {
        switch (p.flags & 3) {
          case 0: host_chain<0>(p, state[s], d, frames, wet.data()); break;
          case 1: host_chain<1>(p, state[s], d, frames, wet.data()); break;
          case 2: host_chain<2>(p, state[s], d, frames, wet.data()); break;
          default: host_chain<3>(p, state[s], d, frames, wet.data()); break;
        }
      }
      if (t == 0) {
        std::memcpy(m, y, (size_t)frames * 8);
      } else {
        for (int i = 0; i < 2 * frames; ++i) m[i] = m[i] + y[i];
      }
    }
  }
}

int launch_dsp_mix(const float* dry, const art_dsp_source_params* params, art_dsp_state* state, int fan_count, int T,
                   int frames, float* mix, hipStream_t st) {
  if (fan_count <= 0 || T <= 0 || frames <= 0) return ART_DSP_KERNEL_NONE;
  const int G = T <= kTS ? kTS / T : 1;
  hipLaunchKernelGGL(dsp_mix_kernel, dim3((fan_count + G - 1) / G), dim3(64), 0, st, dry, params, state, mix, fan_count,
                     T, frames, (uint32_t)((unsigned long long)T * frames * 8ull),
                     (uint32_t)((unsigned long long)fan_count * frames * 8ull));
  return ART_DSP_KERNEL_MIX;
}


// Per-buffer scalars of one OnAudioFilterRead call (art_dsp_math.hpp has the operation sequence).
int dsp_source_params(const art_spatializer_settings& st, const art_audio_source& src, int sample_rate,
                      art_dsp_source_params& p) {
  std::memset(&p, 0, sizeof p);
  if (src.channels != 2) { p.flags = 4; return ART_OK; }
  if (!curve_ok(st.reverb_volume_curve) || (src.muffle_strength > 0.0f && !curve_ok(st.muffle_curve)))
    return ART_E_INVALID;
  DspSourceInputs in;
  in.muffle_strength = src.muffle_strength;
  in.reverb_volume = src.reverb_volume;
  in.local_dir = mk3(src.local_dir[0], src.local_dir[1], src.local_dir[2]);
  in.listener_distance = src.listener_distance;
  in.volume_multiplier = src.volume_multiplier;
  p = dsp_source_scalars(st, in, (float)sample_rate);
  return ART_OK;
}

// One source of the audio tick: the OnLateUpdate step on the frame's settings record, then the
// per-buffer scalars. rec: the 24-B AudioTargetRTSettings record as six floats.
ART_HD art_dsp_source_params tick_source(const art_spatializer_settings& st, float sr, const float rec[6],
                                         const art_listener& l, vec3 target, float volume) {
  DspSourceInputs in;
  in.muffle_strength = rec[0];
  in.reverb_volume = rec[2];
  listener_local(l, mk3(rec[3], rec[4], rec[5]), target, in.local_dir, in.listener_distance);
  in.volume_multiplier = volume;
  return dsp_source_scalars(st, in, sr);
}

int dsp_tick_params_host(const art_spatializer_settings& st, int sample_rate, const art_listener* listeners,
                         const art_fan* fans, int fan_count, const float* targets, int T, const float* volume,
                         art_dsp_source_params* out) {
  if (!curve_ok(st.reverb_volume_curve) || !curve_ok(st.muffle_curve)) return ART_E_INVALID;
  for (int f = 0; f < fan_count; ++f) {
    if (!fans[f].settings) return ART_E_INVALID;
    for (int t = 0; t < T; ++t) {
      float rec[6];
      std::memcpy(rec, &fans[f].settings[t], sizeof rec);
      const size_t s = (size_t)f * T + t;
      out[s] = tick_source(st, (float)sample_rate, rec, listeners[f], mk3(targets[3 * t], targets[3 * t + 1], targets[3 * t + 2]),
                           volume ? volume[s] : 1.0f);
    }
  }
  return ART_OK;
}

// Settings per target: what dsp_tick_params_host writes for a source when it is given
// settings[cls[t]] as its single settings. Everything is checked before anything is written.
int dsp_tick_params_classes_host(const art_spatializer_settings* settings, int class_count, int sample_rate,
                                 const art_listener* listeners, const art_fan* fans, int fan_count, const float* targets,
                                 int T, const uint8_t* cls, const float* volume, art_dsp_source_params* out) {
  if (class_count < 1 || class_count > kMaxSettingsClasses) return ART_E_INVALID;
  for (int k = 0; k < class_count; ++k)
    if (!curve_ok(settings[k].reverb_volume_curve) || !curve_ok(settings[k].muffle_curve)) return ART_E_INVALID;
  if (cls)
    for (int t = 0; t < T; ++t)
      if (cls[t] >= class_count) return ART_E_INVALID;
  for (int f = 0; f < fan_count; ++f)
    if (!fans[f].settings) return ART_E_INVALID;
  for (int f = 0; f < fan_count; ++f) {
    for (int t = 0; t < T; ++t) {
      float rec[6];
      std::memcpy(rec, &fans[f].settings[t], sizeof rec);
      const size_t s = (size_t)f * T + t;
      out[s] = tick_source(settings[cls ? cls[t] : 0], (float)sample_rate, rec, listeners[f],
                           mk3(targets[3 * t], targets[3 * t + 1], targets[3 * t + 2]), volume ? volume[s] : 1.0f);
    }
  }
  return ART_OK;
}

namespace {

// The audio tick's parameter step, one lane per source s = f * T + t: the settings record of the
// frame's result block, the fan's listener, the bound scene's target position and the bound curves
// in, one art_dsp_source_params record out. The block is only read; the settings are assumed
// aligned to 4 bytes only (8-B loads when the record's address allows, the layout's 16-B strides
// always do).
__global__ __launch_bounds__(kDspBlock) void dsp_tick_params_kernel(DspTickArgs a) {
  const int s = blockIdx.x * kDspBlock + threadIdx.x;
  if (s >= a.count) return;
  const int f = s / a.T, t = s - f * a.T;
  const uint8_t* rp = a.block + (size_t)f * a.stride + a.settings_off + (size_t)t * sizeof(art_target_settings);
  float rec[6];
  if ((reinterpret_cast<uintptr_t>(rp) & 7) == 0) {
    const float2* r2 = reinterpret_cast<const float2*>(rp);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float2 v = r2[k];
      rec[2 * k] = v.x;
      rec[2 * k + 1] = v.y;
    }
  } else {
    const float* r1 = reinterpret_cast<const float*>(rp);
#pragma unroll
    for (int k = 0; k < 6; ++k) rec[k] = r1[k];
  }
  const art_listener l = a.listeners[f];
  const vec3 target = mk3(a.targets[3 * t], a.targets[3 * t + 1], a.targets[3 * t + 2]);
  a.out[s] = tick_source(a.st, a.sr, rec, l, target, a.volume ? a.volume[s] : 1.0f);
}

// The 24-B settings record at rp as six floats (aligned to 4 bytes only, as in dsp_tick_params_kernel).
__device__ __forceinline__ void load_settings_record(const uint8_t* rp, float rec[6]) {
  if ((reinterpret_cast<uintptr_t>(rp) & 7) == 0) {
    const float2* r2 = reinterpret_cast<const float2*>(rp);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float2 v = r2[k];
      rec[2 * k] = v.x;
      rec[2 * k + 1] = v.y;
    }
  } else {
    const float* r1 = reinterpret_cast<const float*>(rp);
#pragma unroll
    for (int k = 0; k < 6; ++k) rec[k] = r1[k];
  }
}

// The parameter step with settings per target: one lane per source s = f * T + t, exactly as in
// dsp_tick_params_kernel, but each lane gathers the record of its target's class from the bound table
// (a.cls, the class map, lies in the argument block: stream-ordered with the launch). Measured against
// one wave per (target, 64 fans) with the class's record in SGPRs: DESIGN.md 3a.
__global__ __launch_bounds__(kDspBlock) void dsp_tick_params_classes_kernel(DspTickClassArgs a) {
  const long long s64 = (long long)blockIdx.x * kDspBlock + threadIdx.x;
  if (s64 >= (long long)a.fan_count * a.T) return;
  const int s = (int)s64;
  const int f = s / a.T, t = s - f * a.T;
  float rec[6];
  load_settings_record(a.block + (size_t)f * a.stride + a.settings_off + (size_t)t * sizeof(art_target_settings), rec);
  const art_listener l = a.listeners[f];
  const vec3 target = mk3(a.targets[3 * t], a.targets[3 * t + 1], a.targets[3 * t + 2]);
  const art_spatializer_settings st = a.table[a.cls[t]];
  a.out[s] = tick_source(st, a.sr, rec, l, target, a.volume ? a.volume[s] : 1.0f);
}

}  // namespace

void launch_dsp_tick_params(const DspTickArgs& a, hipStream_t st) {
  if (a.count <= 0) return;
  hipLaunchKernelGGL(dsp_tick_params_kernel, dim3((a.count + kDspBlock - 1) / kDspBlock), dim3(kDspBlock), 0, st, a);
}

void launch_dsp_tick_params_classes(const DspTickClassArgs& a, hipStream_t st) {
  if (a.fan_count <= 0 || a.T <= 0) return;
  const long long count = (long long)a.fan_count * a.T;  // <= 2^31 - 1 (the caller's check)
  hipLaunchKernelGGL(dsp_tick_params_classes_kernel, dim3((unsigned)((count + kDspBlock - 1) / kDspBlock)), dim3(kDspBlock), 0,
                     st, a);
}

// Sources follow the targets: the contract of art_dsp_sources_follow_host, literally.
void dsp_sources_follow_host(const int32_t* target_src, int T_new, int T_old, const int32_t* fan_src, int F_new, int F_old,
                             const art_dsp_state* state_old, const float* volume_old, art_dsp_state* state_new,
                             float* volume_new, float new_volume) {
  for (int f = 0; f < F_new; ++f) {
    const int fo = fan_src ? fan_src[f] : f;
    for (int t = 0; t < T_new; ++t) {
      const size_t s = (size_t)f * T_new + t;
      const int to = target_src[t];
      if (fo >= 0 && fo < F_old && to >= 0 && to < T_old) {
        const size_t so = (size_t)fo * T_old + to;
        std::memcpy(&state_new[s], &state_old[so], sizeof(art_dsp_state));
        if (volume_new) volume_new[s] = volume_old ? volume_old[so] : new_volume;
      } else {
        std::memset(&state_new[s], 0, sizeof(art_dsp_state));
        if (volume_new) volume_new[s] = new_volume;
      }
    }
  }
}

namespace {

constexpr int kFollowBlock = 256;

// Two lanes per source s = f * T_new + t, each moves one 16-B half of the 32-B state (the lanes of a
// wave read and write adjacent halves: full lines for an identity map, 32-B pieces for any other);
// the even lane writes the volume. A pure gather: the old arrays are only read, and only at a source
// whose fan and target index lie inside them. Arrays are assumed aligned to 4 bytes only: 16-B
// accesses when both state arrays allow them (a.wide), four 4-B ones otherwise. The target map is
// read from the argument block.
__global__ __launch_bounds__(kFollowBlock) void dsp_sources_follow_kernel(DspFollowArgs a) {
  const uint32_t i = blockIdx.x * (uint32_t)kFollowBlock + threadIdx.x;  // < 2^32: count <= 2^31 - 1
  const uint32_t s = i >> 1, h = i & 1u;
  if (s >= a.count) return;
  const uint32_t f = s / (uint32_t)a.T_new, t = s - f * (uint32_t)a.T_new;
  const int fo = a.fan_src ? a.fan_src[f] : (int)f;
  const int to = a.target_src[t];
  const bool old = fo >= 0 && fo < a.F_old && to >= 0 && to < a.T_old;
  const size_t so = old ? (size_t)fo * (size_t)a.T_old + (size_t)to : 0;
  const uint8_t* src = a.state_old + so * sizeof(art_dsp_state) + h * 16u;
  uint8_t* dst = a.state_new + (size_t)s * sizeof(art_dsp_state) + h * 16u;
  if (a.wide) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (old) v = *reinterpret_cast<const uint4*>(src);
    *reinterpret_cast<uint4*>(dst) = v;
  } else {
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (old) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = reinterpret_cast<const uint32_t*>(src)[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) reinterpret_cast<uint32_t*>(dst)[k] = v[k];
  }
  if (h == 0u && a.volume_new) a.volume_new[s] = (old && a.volume_old) ? a.volume_old[so] : a.new_volume;
}

}  // namespace

void launch_dsp_sources_follow(const DspFollowArgs& a, hipStream_t st) {
  if (a.count == 0u) return;
  const unsigned long long lanes = 2ull * a.count;
  hipLaunchKernelGGL(dsp_sources_follow_kernel, dim3((unsigned)((lanes + kFollowBlock - 1) / kFollowBlock)),
                     dim3(kFollowBlock), 0, st, a);
}

// Returns the kernel it launched (ART_DSP_KERNEL_*, art_debug_last_dsp_kernel).
int launch_dsp(float* data, unsigned long long data_bytes, const long long* offsets, const int* frames_of,
               int frames_all, const art_dsp_source_params* params, art_dsp_state* state, int count, hipStream_t st) {
  if (count <= 0) return ART_DSP_KERNEL_NONE;
  static const int mode = [] {  // ART_DSP_KERNEL=lane: one lane per source, direct loads (A/B only)
    const char* e = std::getenv("ART_DSP_KERNEL");
    return e && !std::strcmp(e, "lane") ? 1 : 0;
  }();
  // the tiled kernel's 8-B buffer ops need an 8-B aligned base (every source offset is an even
  // float count) and 32-bit byte offsets
  const bool aligned = (reinterpret_cast<uintptr_t>(data) & 7) == 0;
  if (mode == 0 && aligned && data_bytes < 0x7fffffffULL) {
    hipLaunchKernelGGL(dsp_tiled_kernel, dim3((count + kTS - 1) / kTS), dim3(64), 0, st, data, offsets, frames_of,
                       frames_all, params, state, count, (uint32_t)data_bytes);
    return ART_DSP_KERNEL_TILED;
  }
  hipLaunchKernelGGL(dsp_kernel, dim3((count + kDspBlock - 1) / kDspBlock), dim3(kDspBlock), 0, st, data, offsets,
                     frames_of, frames_all, params, state, count);
  return ART_DSP_KERNEL_LANE;
}

}  // namespace art
