// art_dsp_math.hpp — the spatializer's per-buffer scalars (include/art_dsp.h), shared by the host
// entry points (art_dsp_source_params_get, art_dsp_process, art_dsp_tick_params_host) and the device
// tick (dsp_tick_params_kernel, art_dsp.hip), so both evaluate the reference's fp32 operation
// sequences from one source; and the per-sample chain of one channel (Chain,
// step<M>), shared by dsp_tiled_kernel, dsp_mix_kernel and the listener mix's host twin.
#pragma once

#include <math.h>

#include "../../include/art_dsp.h"
#include "unity_math.hpp"

#pragma clang fp contract(off)

namespace art {

ART_HD float uclamp(float x, float a, float b) { return umax(a, umin(b, x)); }
constexpr float kToDegrees = 57.29578f;      // math.degrees
constexpr float kToRadians = 0.0174532924f;  // math.radians
constexpr float kDoublePi = 2.0f * 3.14159265f;  // MuffleDSP.cs:35 / BinauralDSP.cs:84

// NativeSampledAnimationCurve.Evaluate (NativeSampledAnimationCurve.cs:64-89)
ART_HD float curve_eval(const art_curve& c, float time) {
  const float percent = time / c.length;
  const int n = c.sample_count;
  const float cp = umax(0.0f, umin((float)(n - 1), percent * (float)(n - 1)));
  const int fi = (int)floorf(cp), ci = (int)ceilf(cp);
  return ulerp(c.baked[fi], c.baked[ci], cp - (float)fi);
}

ART_HD float lowpass_alpha(float cutoff, float sr) {  // MuffleDSP.cs:40-42, BinauralDSP.cs:89-91
  const float rc = 1.0f / (cutoff * kDoublePi);
  const float dt = 1.0f / sr;
  return dt / (rc + dt);
}
ART_HD float highpass_alpha(float cutoff, float sr) {  // BinauralDSP.cs:99-101
  const float rc = 1.0f / (cutoff * kDoublePi);
  const float dt = 1.0f / sr;
  return rc / (rc + dt);
}

ART_HD bool curve_ok(const art_curve& c) { return c.baked && c.sample_count >= 2; }

// The inputs of one stereo source that change per buffer: the ray tracer's settings of its audio
// target and what AudioSpatializer.OnLateUpdate caches (AudioSpatializer.cs:61-67).
struct DspSourceInputs {
  float muffle_strength, reverb_volume;  // audioTargetSettings
  vec3 local_dir;                        // cachedLocalDir (:64)
  float listener_distance;               // cachedListenerDistance (:66)
  float volume_multiplier;               // volumeMultiplier (:18)
};

// AudioSpatializer.OnLateUpdate (AudioSpatializer.cs:61-67). Transform.InverseTransformDirection is
// engine-native; the contract is the Unity.Mathematics form math.mul(math.inverse(q), v): rotation
// only, as InverseTransformDirection ignores scale (parity-unpinned).
ART_HD void listener_local(const art_listener& l, vec3 perceived_position, vec3 target_position, vec3& local_dir,
                           float& listener_distance) {
  const vec3 lp = mk3(l.position[0], l.position[1], l.position[2]);
  quat q;
  q.x = l.rotation[0]; q.y = l.rotation[1]; q.z = l.rotation[2]; q.w = l.rotation[3];
  const vec3 world = perceived_position - lp;
  local_dir = normalize(qmul(qinverse(q), world));
  listener_distance = distance(target_position, lp);
}

// Per-buffer scalars of one stereo source (everything the C# recomputes per sample is constant over
// the buffer). Both curves must be curve_ok when they are read (the muffle curve only when
// muffle_strength > 0).
ART_HD art_dsp_source_params dsp_source_scalars(const art_spatializer_settings& st, const DspSourceInputs& in, float sr) {
  art_dsp_source_params p{};
  if (in.muffle_strength > 0.0f) {  // MuffleDSP.cs:22-26
    const float muffle = curve_eval(st.muffle_curve, in.muffle_strength);
    const float cutoff = ulerp(st.muffle_cutoff_max, st.muffle_cutoff_min, muffle);
    p.muffle_alpha = lowpass_alpha(cutoff, sr);
    p.flags |= 1;
  }
  {  // ReverbDSP.cs:12-13
    const float t = curve_eval(st.reverb_volume_curve, in.reverb_volume);
    p.dry_boost = ulerp(st.reverb_dry_boost_min, st.reverb_dry_boost_max, t);
  }
  {  // BinauralDSP.cs:17-50, :65, :73
    const vec3 ld = in.local_dir;
    const float dist = in.listener_distance;
    // BinauralDSP.Process runs unbursted on the audio thread (no [BurstCompile] under Audio/), so
    // Unity.Mathematics' atan2 / sin / cos are (float)System.Math.Atan2/Sin/Cos: double precision,
    // rounded once to float (the host libm's double functions here, the device library's in a kernel).
    const float azimuth = (float)atan2((double)ld.x, (double)ld.z) * kToDegrees;
    float eps = st.pan_strength;
    if (st.distance_based_panning) eps *= usaturate(dist / st.max_pan_distance);
    const float pan = (float)sin((double)(azimuth * kToRadians)) * eps;
    const float gl = sqrtf(0.5f * (1.0f - pan));
    const float gr = sqrtf(0.5f * (1.0f + pan));
    const float front = umax(0.0f, (float)cos((double)(azimuth * kToRadians)));
    float rear = ulerp(1.0f - st.rear_attenuation_strength, 1.0f, front);
    if (st.distance_based_rear_attenuation) {
      const float df = usaturate(1.0f - (dist / st.max_rear_attenuation_distance));
      rear = uclamp(rear * df, 1.0f - st.rear_attenuation_strength, 1.0f);
    }
    const float elev = ld.y <= 0.0f ? ulerp(1.0f, st.low_pass_volume, usaturate(-ld.y))
                                    : ulerp(1.0f, st.high_pass_volume, usaturate(ld.y));
    p.gain_left = gl * rear * elev;
    p.gain_right = gr * rear * elev;
    if (ld.y <= 0.0f) {
      const float c = ulerp(st.low_pass_cutoff_min, st.low_pass_cutoff_max, usaturate(-ld.y)) *
                      (1.0f - 0.5f * usaturate(dist / st.max_elevation_effect_distance));
      p.filter_alpha = lowpass_alpha(c, sr);
      p.flags |= 2;
    } else {
      const float c = ulerp(st.high_pass_cutoff_min, st.high_pass_cutoff_max, usaturate(ld.y)) *
                      (1.0f + 0.5f * usaturate(dist / st.max_elevation_effect_distance));
      p.filter_alpha = highpass_alpha(c, sr);
    }
  }
  p.volume = in.volume_multiplier;
  return p;
}

// ---- the per-sample chain of one channel (AudioSpatializer.OnAudioFilterRead's four passes fused) ----
// One definition for dsp_tiled_kernel, dsp_mix_kernel and the host twin of the listener mix
// (art_dsp_mix_host): all evaluate this operation sequence.
struct Chain {
  float pm, pl, ph, pi;  // previousMuffle, previousLP, previousHP, previousInput of this channel
};

// M: bit 0 muffle, bit 1 low pass (fixed for the caller's wave or source); M == 4: per-lane selects
// (exact: every selected value is computed with the same operations as in the fixed variants).
template <int M>
ART_HD float step(float x, const art_dsp_source_params& p, float gain, bool mf, bool lp, Chain& c) {
  if constexpr (M == 4) {
    const float m = c.pm + p.muffle_alpha * (x - c.pm);
    x = mf ? m : x;
    c.pm = mf ? m : c.pm;
  } else if constexpr (M & 1) {
    c.pm = c.pm + p.muffle_alpha * (x - c.pm);  // MuffleDSP.LowPass :43-44
    x = c.pm;
  }
  x = x * p.dry_boost;  // ReverbDSP :21-22
  x = x * gain;         // BinauralDSP :59-60
  if constexpr (M == 4) {
    const float l = c.pl + p.filter_alpha * (x - c.pl);
    const float h = p.filter_alpha * (c.ph + x - c.pi);
    c.pl = lp ? l : c.pl;
    c.ph = lp ? c.ph : h;
    c.pi = lp ? c.pi : x;
    x = lp ? l : h;
  } else if constexpr (M & 2) {
    c.pl = c.pl + p.filter_alpha * (x - c.pl);  // LowPass :92-93
    x = c.pl;
  } else {
    const float h = p.filter_alpha * (c.ph + x - c.pi);  // HighPass :102-105
    c.pi = x;
    c.ph = h;
    x = h;
  }
  return x * p.volume;  // AudioSpatializer.cs:84-85
}

}  // namespace art
