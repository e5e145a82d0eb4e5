// art_dsp_api.cpp — the per-sample spatializer DSP entry points (include/art_dsp.h) over the
// kernels of art_dsp.hip: batching and staging of a host call, the device-resident call.
#include "art_ctx.hpp"

using namespace art;

extern "C" {

ART_API int art_dsp_source_params_get(const art_spatializer_settings* settings, const art_audio_source* source,
                                      int32_t sample_rate, art_dsp_source_params* out) {
  if (!settings || !source || !out || sample_rate <= 0) return ART_E_INVALID;
  return dsp_source_params(*settings, *source, sample_rate, *out);
}

ART_API int art_dsp_process(art_ctx* c, const art_spatializer_settings* settings, art_audio_source* sources,
                            int32_t count, int32_t sample_rate) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  if (!settings || count < 0 || (count > 0 && !sources) || sample_rate <= 0) return fail(c, ART_E_INVALID, "invalid argument");
  if (c->inflight) return fail(c, ART_E_STATE, "a frame is in flight");
  c->last_dsp_kernel = ART_DSP_KERNEL_NONE;
  // host: per-buffer scalars; stereo sources with samples go to the device
  std::vector<int> idx;
  std::vector<art_dsp_source_params> params;
  std::vector<long long> offs;
  std::vector<int> frames;
  long long total = 0;  // floats, each source 16-B aligned
  for (int32_t k = 0; k < count; ++k) {
    const art_audio_source& a = sources[k];
    if (a.frames < 0 || (a.frames > 0 && !a.data) || !a.state) return fail(c, ART_E_INVALID, "invalid source %d", k);
    if (a.channels != 2 || a.frames == 0) continue;  // left as is (AudioSpatializer.cs:72)
    art_dsp_source_params p;
    if (dsp_source_params(*settings, a, sample_rate, p) != ART_OK) return fail(c, ART_E_INVALID, "invalid curve");
    idx.push_back(k);
    params.push_back(p);
    offs.push_back(total);
    frames.push_back(a.frames);
    total += ((long long)a.frames * 2 + 3) & ~3LL;
  }
  const size_t n = idx.size();
  if (n == 0) return ART_OK;
  {  // group sources by filter class (muffle x low/high pass) so a wave's chains run one code path
    std::vector<size_t> ord(n);
    for (size_t j = 0; j < n; ++j) ord[j] = j;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return (params[a].flags & 3) < (params[b].flags & 3); });
    std::vector<int> idx2(n);
    std::vector<art_dsp_source_params> params2(n);
    std::vector<int> frames2(n);
    total = 0;
    for (size_t j = 0; j < n; ++j) {
      idx2[j] = idx[ord[j]];
      params2[j] = params[ord[j]];
      frames2[j] = frames[ord[j]];
      offs[j] = total;
      total += ((long long)frames2[j] * 2 + 3) & ~3LL;
    }
    idx.swap(idx2);
    params.swap(params2);
    frames.swap(frames2);
  }
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_data = 0, o_offs = al(o_data + (size_t)total * 4), o_frames = al(o_offs + n * 8),
               o_params = al(o_frames + n * 4), o_state = al(o_params + n * sizeof(art_dsp_source_params)),
               bytes = al(o_state + n * sizeof(art_dsp_state));
  Device& dv = c->devs[0];
  HIP_TRY(c, hipSetDevice(dv.id));
  if (!c->h_dsp.reserve(bytes) || !dv.dsp.reserve(bytes)) return fail(c, ART_E_NOMEM, "allocation failed");
  uint8_t* h = static_cast<uint8_t*>(c->h_dsp.p);
  for (size_t j = 0; j < n; ++j) {
    const art_audio_source& a = sources[idx[j]];
    std::memcpy(h + o_data + offs[j] * 4, a.data, (size_t)a.frames * 8);
    std::memcpy(h + o_state + j * sizeof(art_dsp_state), a.state, sizeof(art_dsp_state));
  }
  std::memcpy(h + o_offs, offs.data(), n * 8);
  std::memcpy(h + o_frames, frames.data(), n * 4);
  std::memcpy(h + o_params, params.data(), n * sizeof(art_dsp_source_params));
  uint8_t* d = static_cast<uint8_t*>(dv.dsp.p);
  HIP_TRY(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, dv.stream));
  c->last_dsp_kernel = launch_dsp(reinterpret_cast<float*>(d + o_data), (unsigned long long)total * 4,
                                  reinterpret_cast<const long long*>(d + o_offs), reinterpret_cast<const int*>(d + o_frames), 0,
                                  reinterpret_cast<const art_dsp_source_params*>(d + o_params),
                                  reinterpret_cast<art_dsp_state*>(d + o_state), (int)n, dv.stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(h + o_data, d + o_data, (size_t)total * 4, hipMemcpyDeviceToHost, dv.stream));
  HIP_TRY(c, hipMemcpyAsync(h + o_state, d + o_state, n * sizeof(art_dsp_state), hipMemcpyDeviceToHost, dv.stream));
  HIP_TRY(c, hipStreamSynchronize(dv.stream));
  for (size_t j = 0; j < n; ++j) {
    art_audio_source& a = sources[idx[j]];
    std::memcpy(a.data, h + o_data + offs[j] * 4, (size_t)a.frames * 8);
    std::memcpy(a.state, h + o_state + j * sizeof(art_dsp_state), sizeof(art_dsp_state));
  }
  return ART_OK;
}

ART_API int art_dsp_process_device(art_ctx* c, float* d_data, const art_dsp_source_params* d_params,
                                   art_dsp_state* d_state, int32_t count, int32_t frames, void* stream) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  if (count < 0 || frames < 0 || (count > 0 && (!d_data || !d_params || !d_state))) return fail(c, ART_E_INVALID, "invalid argument");
  c->last_dsp_kernel = ART_DSP_KERNEL_NONE;
  if (count == 0 || frames == 0) return ART_OK;
  Device& dv = c->devs[0];
  HIP_TRY(c, hipSetDevice(dv.id));
  c->last_dsp_kernel = launch_dsp(d_data, (unsigned long long)count * (unsigned long long)frames * 8ull, nullptr, nullptr,
                                  frames, d_params, d_state, count, static_cast<hipStream_t>(stream));
  HIP_TRY(c, hipGetLastError());
  return ART_OK;
}

// ---------------------------------------------------------------------------- audio tick
ART_API int art_dsp_tick_params_host(const art_spatializer_settings* settings, int32_t sample_rate,
                                     const art_listener* listeners, const art_fan* fans, int32_t fan_count,
                                     const float* target_positions, int32_t target_count, const float* volume,
                                     art_dsp_source_params* out) {
  if (!settings || sample_rate <= 0 || fan_count < 0 || target_count < 0) return ART_E_INVALID;
  if (fan_count > 0 && (!listeners || !fans || (target_count > 0 && (!target_positions || !out)))) return ART_E_INVALID;
  return dsp_tick_params_host(*settings, sample_rate, listeners, fans, fan_count, target_positions, target_count, volume, out);
}

ART_API int art_dsp_tick_params_classes_host(const art_spatializer_settings* settings, int32_t class_count, int32_t sample_rate,
                                             const art_listener* listeners, const art_fan* fans, int32_t fan_count,
                                             const float* target_positions, int32_t target_count, const uint8_t* target_class,
                                             const float* volume, art_dsp_source_params* out) {
  if (!settings || sample_rate <= 0 || fan_count < 0 || target_count < 0) return ART_E_INVALID;
  if (fan_count > 0 && (!listeners || !fans || (target_count > 0 && (!target_positions || !out)))) return ART_E_INVALID;
  return dsp_tick_params_classes_host(settings, class_count, sample_rate, listeners, fans, fan_count, target_positions,
                                      target_count, target_class, volume, out);
}

// The bind of class_count settings records (art_dsp_settings_bind: one): the table and every class's
// two curves as one packed image, [records | curves], in one copy to devs[0].tick_curves.
static int bind_settings(art_ctx* c, const char* fn, const art_spatializer_settings* settings, int32_t class_count,
                         int32_t sample_rate) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", fn);
  if (!settings || sample_rate <= 0) return fail(c, ART_E_INVALID, "invalid argument");
  if (class_count < 1 || class_count > kMaxSettingsClasses)
    return fail(c, ART_E_INVALID, "%s: class_count %d is outside [1, %d]", fn, class_count, kMaxSettingsClasses);
  size_t floats = 0;
  for (int32_t k = 0; k < class_count; ++k) {
    const art_curve& mc = settings[k].muffle_curve;
    const art_curve& rc = settings[k].reverb_volume_curve;
    if (!mc.baked || mc.sample_count < 2 || !rc.baked || rc.sample_count < 2)
      return fail(c, ART_E_INVALID, "%s: both curves need a baked table of at least 2 samples", fn);
    floats += (size_t)mc.sample_count + (size_t)rc.sample_count;
  }
  if (c->inflight) return fail(c, ART_E_STATE, "a frame is in flight");
  if (c->devs.empty()) return fail(c, ART_E_STATE, "the context has no device");
  Device& dv = c->devs[0];
  HIP_TRY(c, hipSetDevice(dv.id));
  // a tick still running on the caller's stream reads the table and the curves being replaced
  if (int rc2 = dv.fence.wait(c, dv.stream)) return rc2;
  HIP_TRY(c, hipStreamSynchronize(dv.stream));
  c->tick.bound = false;
  const size_t table_bytes = (size_t)class_count * sizeof(art_spatializer_settings);  // a multiple of 8
  const size_t bytes = table_bytes + floats * sizeof(float);
  if (!dv.tick_curves.reserve(bytes)) return fail(c, ART_E_NOMEM, "device allocation failed");
  uint8_t* d = static_cast<uint8_t*>(dv.tick_curves.p);
  std::vector<uint8_t> image(bytes);
  art_spatializer_settings* table = reinterpret_cast<art_spatializer_settings*>(image.data());
  size_t at = table_bytes;
  for (int32_t k = 0; k < class_count; ++k) {
    table[k] = settings[k];
    for (art_curve* cv : {&table[k].muffle_curve, &table[k].reverb_volume_curve}) {
      const size_t n = (size_t)cv->sample_count * sizeof(float);
      std::memcpy(image.data() + at, cv->baked, n);
      cv->baked = reinterpret_cast<float*>(d + at);
      at += n;
    }
  }
  HIP_TRY(c, hipMemcpy(d, image.data(), bytes, hipMemcpyHostToDevice));
  c->tick.st = table[0];
  c->tick.class_count = class_count;
  c->tick.d_table = reinterpret_cast<const art_spatializer_settings*>(d);
  c->tick.sample_rate = sample_rate;
  c->tick.bound = true;
  return ART_OK;
}

ART_API int art_dsp_settings_bind(art_ctx* c, const art_spatializer_settings* settings, int32_t sample_rate) {
  return bind_settings(c, __func__, settings, 1, sample_rate);
}

ART_API int art_dsp_settings_bind_classes(art_ctx* c, const art_spatializer_settings* settings, int32_t class_count,
                                          int32_t sample_rate) {
  return bind_settings(c, __func__, settings, class_count, sample_rate);
}

// ---------------------------------------------------------------------------- the class map
ART_API int art_dsp_target_classes_set(art_ctx* c, const uint8_t* cls, int32_t count) {
  if (!c) return ART_E_INVALID;
  if (count < 0 || count > kMaxTargets || (count > 0 && !cls))
    return fail(c, ART_E_INVALID, "%s: count outside [0, %d] or a NULL map", __func__, kMaxTargets);
  c->tick.target_class.assign(cls, cls + count);
  return ART_OK;
}

ART_API int art_dsp_target_classes_get(art_ctx* c, uint8_t* out, int32_t cap) {
  if (!c || cap < 0 || (cap > 0 && !out)) return ART_E_INVALID;
  const std::vector<uint8_t>& m = c->tick.target_class;
  for (int32_t i = 0; i < cap && (size_t)i < m.size(); ++i) out[i] = m[(size_t)i];
  return (int)m.size();
}

// What the listener mix asks of its buffers (dsp_mix_kernel's 8-B buffer operations with 32-bit byte
// offsets); 0 or an error code, `why` set.
static int mix_limits(const float* d_dry, const float* d_mix, long long fan_count, long long T, long long frames,
                      const char*& why) {
  if ((reinterpret_cast<uintptr_t>(d_dry) | reinterpret_cast<uintptr_t>(d_mix)) & 7) {
    why = "d_dry and d_mix must be 8-byte aligned";
    return ART_E_INVALID;
  }
  if (T * frames * 8 > 0x7fffffffLL || fan_count * frames * 8 > 0x7fffffffLL || fan_count * T > 0x7fffffffLL) {
    why = "T * frames * 8 and fan_count * frames * 8 must stay below 2^31 bytes (split the call)";
    return ART_E_UNSUPPORTED;
  }
  return ART_OK;
}

// The buffers of a listener mix that follows the parameter step (art_dsp_tick_mix_device): checked
// with the other arguments, before anything is enqueued.
struct TickMix { const float* d_dry; const float* d_mix; int32_t frames; };

// The parameter step of the tick on `st`, ordered as a reader of the bound scene; count_out: sources.
static int tick_params(art_ctx* c, const char* fn, const void* d_block, uint32_t out_flags, int32_t fan_count,
                       const art_listener* d_listeners, const float* d_volume, art_dsp_source_params* d_params,
                       bool more_null, hipStream_t st, int& count_out, const TickMix* mix = nullptr) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", fn);
  if (c->inflight) return fail(c, ART_E_STATE, "%s: a frame is in flight (tick after art_complete)", fn);
  if (c->devs.empty() || !c->devs[0].bound) return fail(c, ART_E_STATE, "%s: no scene bound (art_scene_bind)", fn);
  if (!c->tick.bound) return fail(c, ART_E_STATE, "%s: no spatializer settings bound (art_dsp_settings_bind)", fn);
  const Frame& f = c->fr;
  if (!(f.stages & ART_STAGE_REDUCE)) return fail(c, ART_E_INVALID, "%s: the bound frame has no ART_STAGE_REDUCE (no settings section)", fn);
  if (fan_count < 0 || (fan_count > 0 && (!d_block || !d_listeners || !d_params || more_null)))
    return fail(c, ART_E_INVALID, "%s: bad device buffers", fn);
  count_out = 0;
  if (fan_count == 0) return ART_OK;
  Device& dv = c->devs[0];
  if (dv.sc.T != f.T || !dv.sc.targets) return fail(c, ART_E_STATE, "%s: the bound scene's targets are not the frame's", fn);
  if ((long long)fan_count * f.T > 0x7fffffffLL) return fail(c, ART_E_UNSUPPORTED, "%s: more than 2^31 - 1 sources", fn);
  // one class and no map: dsp_tick_params_kernel on that class, as before there were classes
  const std::vector<uint8_t>& cls = c->tick.target_class;
  const bool classes = c->tick.class_count > 1 || !cls.empty();
  if (!cls.empty()) {
    if ((int)cls.size() != f.T)
      return fail(c, ART_E_STATE, "%s: the class map has %d entries, the bound frame %d targets (art_dsp_target_classes_follow)",
                  fn, (int)cls.size(), f.T);
    for (int t = 0; t < f.T; ++t)
      if (cls[(size_t)t] >= c->tick.class_count)
        return fail(c, ART_E_STATE, "%s: target %d names class %d, %d are bound", fn, t, (int)cls[(size_t)t], c->tick.class_count);
  }
  if (mix && mix->frames > 0) {
    const char* why = nullptr;
    if (int rc = mix_limits(mix->d_dry, mix->d_mix, fan_count, f.T, mix->frames, why)) return fail(c, rc, "%s: %s", fn, why);
  }
  HIP_TRY(c, hipSetDevice(dv.id));
  // the bound frame's layout for the requested outputs (as art_launch_device derives it)
  art_frame_desc tmp{};
  tmp.ray_count = f.R; tmp.max_hits_per_ray = f.H; tmp.audio_target_count = f.T; tmp.batch_slots = f.TC;
  tmp.stages = f.stages;
  const FanLayout L = make_layout(&tmp, out_flags);
  DspTickArgs a{};
  a.block = static_cast<const uint8_t*>(d_block);
  a.stride = L.stride;
  a.settings_off = L.settings_off;
  a.T = f.T;
  a.count = fan_count * f.T;
  a.listeners = d_listeners;
  a.targets = dv.sc.targets;
  a.volume = d_volume;
  a.out = d_params;
  a.st = c->tick.st;
  a.sr = (float)c->tick.sample_rate;
  int rc = scene_reader_begin(c, dv, f, st);
  if (rc) return rc;
  if (classes) {
    DspTickClassArgs b{};
    b.block = a.block; b.stride = a.stride; b.settings_off = a.settings_off;
    b.T = f.T; b.fan_count = fan_count;
    b.listeners = a.listeners; b.targets = a.targets; b.volume = a.volume; b.out = a.out;
    b.table = c->tick.d_table;
    b.sr = a.sr;
    if (!cls.empty()) std::memcpy(b.cls, cls.data(), cls.size());  // empty: all class 0
    launch_dsp_tick_params_classes(b, st);
  } else {
    launch_dsp_tick_params(a, st);
  }
  HIP_TRY(c, hipGetLastError());
  count_out = a.count;
  return scene_reader_end(c, dv, st);
}

ART_API int art_dsp_tick_params_device(art_ctx* c, const void* d_block, uint32_t out_flags, int32_t fan_count,
                                       const art_listener* d_listeners, const float* d_volume,
                                       art_dsp_source_params* d_params, void* stream) {
  int count = 0;
  return tick_params(c, __func__, d_block, out_flags, fan_count, d_listeners, d_volume, d_params, false,
                     static_cast<hipStream_t>(stream), count);
}

ART_API int art_dsp_tick_device(art_ctx* c, const void* d_block, uint32_t out_flags, int32_t fan_count,
                                const art_listener* d_listeners, const float* d_volume, float* d_data,
                                art_dsp_state* d_state, int32_t frames, art_dsp_source_params* d_params, void* stream) {
  if (c && !c->cpu && frames < 0) return fail(c, ART_E_INVALID, "%s: frames is negative", __func__);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int count = 0;
  int rc = tick_params(c, __func__, d_block, out_flags, fan_count, d_listeners, d_volume, d_params,
                       frames > 0 && (!d_data || !d_state), st, count);
  if (rc) return rc;
  c->last_dsp_kernel = ART_DSP_KERNEL_NONE;
  if (count == 0 || frames == 0) return ART_OK;
  c->last_dsp_kernel = launch_dsp(d_data, (unsigned long long)count * (unsigned long long)frames * 8ull, nullptr, nullptr,
                                  frames, d_params, d_state, count, st);
  HIP_TRY(c, hipGetLastError());
  return ART_OK;
}

// ---------------------------------------------------------------------------- listener mix
ART_API int art_dsp_mix_device(art_ctx* c, const float* d_dry, const art_dsp_source_params* d_params,
                               art_dsp_state* d_state, int32_t fan_count, int32_t target_count, int32_t frames,
                               float* d_mix, void* stream) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  if (fan_count < 0 || target_count < 0 || frames < 0) return fail(c, ART_E_INVALID, "%s: negative argument", __func__);
  c->last_dsp_kernel = ART_DSP_KERNEL_NONE;
  if (fan_count == 0 || frames == 0) return ART_OK;
  if (target_count < 1) return fail(c, ART_E_INVALID, "%s: target_count must be at least 1", __func__);
  if (!d_dry || !d_params || !d_state || !d_mix) return fail(c, ART_E_INVALID, "%s: bad device buffers", __func__);
  const char* why = nullptr;
  if (int rc = mix_limits(d_dry, d_mix, fan_count, target_count, frames, why)) return fail(c, rc, "%s: %s", __func__, why);
  Device& dv = c->devs[0];
  HIP_TRY(c, hipSetDevice(dv.id));
  c->last_dsp_kernel =
      launch_dsp_mix(d_dry, d_params, d_state, fan_count, target_count, frames, d_mix, static_cast<hipStream_t>(stream));
  HIP_TRY(c, hipGetLastError());
  return ART_OK;
}

ART_API int art_dsp_tick_mix_device(art_ctx* c, const void* d_block, uint32_t out_flags, int32_t fan_count,
                                    const art_listener* d_listeners, const float* d_volume, const float* d_dry,
                                    art_dsp_state* d_state, int32_t frames, art_dsp_source_params* d_params,
                                    float* d_mix, void* stream) {
  if (c && !c->cpu && frames < 0) return fail(c, ART_E_INVALID, "%s: frames is negative", __func__);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int count = 0;
  const TickMix mix{d_dry, d_mix, frames};
  int rc = tick_params(c, __func__, d_block, out_flags, fan_count, d_listeners, d_volume, d_params,
                       frames > 0 && (!d_dry || !d_state || !d_mix), st, count, &mix);
  if (rc) return rc;
  c->last_dsp_kernel = ART_DSP_KERNEL_NONE;
  if (count == 0 || frames == 0) return ART_OK;
  c->last_dsp_kernel = launch_dsp_mix(d_dry, d_params, d_state, fan_count, c->fr.T, frames, d_mix, st);
  HIP_TRY(c, hipGetLastError());
  return ART_OK;
}

ART_API int art_dsp_mix_host(const art_dsp_source_params* params, art_dsp_state* state, const float* dry,
                             int32_t fan_count, int32_t target_count, int32_t frames, float* mix) {
  if (fan_count < 0 || target_count < 0 || frames < 0) return ART_E_INVALID;
  if (fan_count == 0 || frames == 0) return ART_OK;
  if (target_count < 1 || !params || !state || !dry || !mix) return ART_E_INVALID;
  dsp_mix_host(params, state, dry, fan_count, target_count, frames, mix);
  return ART_OK;
}

ART_API int art_debug_last_dsp_kernel(art_ctx* c) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  return c->last_dsp_kernel;
}

// ---------------------------------------------------------------------------- sources follow the targets
// Every entry of a target map lies in [-1, T_old).
static bool follow_map_ok(const int32_t* target_src, int32_t T_new, int32_t T_old) {
  for (int32_t t = 0; t < T_new; ++t)
    if (target_src[t] < -1 || target_src[t] >= T_old) return false;
  return true;
}

ART_API int art_dsp_target_classes_follow(art_ctx* c, const int32_t* target_src, int32_t target_count_new,
                                          int32_t target_count_old, uint8_t new_class) {
  if (!c) return ART_E_INVALID;
  if (target_count_new < 0 || target_count_old < 0) return fail(c, ART_E_INVALID, "%s: negative count", __func__);
  if (!target_src) {  // the store's follow map: the caller's counts must be the store's
    const TargetStore& t = c->targets;
    if (target_count_new != t.synced || target_count_old != t.base_count)
      return fail(c, ART_E_INVALID, "%s: target counts %d <- %d are not the store's (synced %d, follow base %d)", __func__,
                  target_count_new, target_count_old, t.synced, t.base_count);
    target_src = t.follow.data();
  }
  if (target_count_new > kMaxTargets || target_count_old > kMaxTargets)
    return fail(c, ART_E_UNSUPPORTED, "%s: more than %d targets", __func__, kMaxTargets);
  std::vector<uint8_t>& m = c->tick.target_class;
  if (!m.empty() && (int32_t)m.size() != target_count_old)
    return fail(c, ART_E_INVALID, "%s: the class map has %d entries, target_count_old is %d", __func__, (int)m.size(),
                target_count_old);
  if (target_count_new > 0 && !follow_map_ok(target_src, target_count_new, target_count_old))
    return fail(c, ART_E_INVALID, "%s: a target_src entry lies outside [-1, %d)", __func__, target_count_old);
  std::vector<uint8_t> next((size_t)target_count_new);
  for (int32_t t = 0; t < target_count_new; ++t) {
    const int32_t to = target_src[t];
    next[(size_t)t] = to < 0 ? new_class : m.empty() ? (uint8_t)0 : m[(size_t)to];  // an empty map is all zeros
  }
  m.swap(next);
  return ART_OK;
}

ART_API int art_dsp_sources_follow_host(const int32_t* target_src, int32_t target_count_new, int32_t target_count_old,
                                        const int32_t* fan_src, int32_t fan_count_new, int32_t fan_count_old,
                                        const art_dsp_state* state_old, const float* volume_old,
                                        art_dsp_state* state_new, float* volume_new, float new_volume) {
  if (target_count_new < 0 || target_count_old < 0 || fan_count_new < 0 || fan_count_old < 0) return ART_E_INVALID;
  if (fan_count_new == 0 || target_count_new == 0) return ART_OK;  // no source to write
  if (!target_src || !state_new) return ART_E_INVALID;
  if (fan_count_old > 0 && target_count_old > 0 && !state_old) return ART_E_INVALID;
  if (!follow_map_ok(target_src, target_count_new, target_count_old)) return ART_E_INVALID;
  dsp_sources_follow_host(target_src, target_count_new, target_count_old, fan_src, fan_count_new, fan_count_old, state_old,
                          volume_old, state_new, volume_new, new_volume);
  return ART_OK;
}

ART_API int art_dsp_sources_follow_device(art_ctx* c, const int32_t* target_src, int32_t target_count_new,
                                          int32_t target_count_old, const int32_t* d_fan_src, int32_t fan_count_new,
                                          int32_t fan_count_old, const art_dsp_state* d_state_old, const float* d_volume_old,
                                          art_dsp_state* d_state_new, float* d_volume_new, float new_volume, void* stream) {
  if (!c) return ART_E_INVALID;
  if (c->cpu) return fail(c, ART_E_UNSUPPORTED, "%s: the CPU backend (device_mask 0) has the host entry points only", __func__);
  if (target_count_new < 0 || target_count_old < 0 || fan_count_new < 0 || fan_count_old < 0)
    return fail(c, ART_E_INVALID, "%s: negative count", __func__);
  if (!target_src) {  // the store's follow map: the caller's counts must be the store's
    const TargetStore& t = c->targets;
    if (target_count_new != t.synced || target_count_old != t.base_count)
      return fail(c, ART_E_INVALID, "%s: target counts %d <- %d are not the store's (synced %d, follow base %d)", __func__,
                  target_count_new, target_count_old, t.synced, t.base_count);
    target_src = t.follow.data();
  }
  if (target_count_new > kMaxTargets || target_count_old > kMaxTargets)
    return fail(c, ART_E_UNSUPPORTED, "%s: more than %d targets", __func__, kMaxTargets);
  const long long count = (long long)fan_count_new * target_count_new, count_old = (long long)fan_count_old * target_count_old;
  if (count > 0x7fffffffLL) return fail(c, ART_E_UNSUPPORTED, "%s: more than 2^31 - 1 sources", __func__);
  if (count == 0) return ART_OK;
  if (!d_state_new || (count_old > 0 && !d_state_old)) return fail(c, ART_E_INVALID, "%s: bad device buffers", __func__);
  if (!follow_map_ok(target_src, target_count_new, target_count_old))
    return fail(c, ART_E_INVALID, "%s: a target_src entry lies outside [-1, %d)", __func__, target_count_old);
  const uintptr_t so = reinterpret_cast<uintptr_t>(d_state_old), vo = reinterpret_cast<uintptr_t>(d_volume_old),
                  sn = reinterpret_cast<uintptr_t>(d_state_new), vn = reinterpret_cast<uintptr_t>(d_volume_new),
                  fs = reinterpret_cast<uintptr_t>(d_fan_src);
  if ((so | vo | sn | vn | fs) & 3) return fail(c, ART_E_INVALID, "%s: device arrays must be 4-byte aligned", __func__);
  {  // out of place only: no old array may overlap a new one
    struct Range { uintptr_t p; unsigned long long bytes; };
    const Range olds[2] = {{so, (unsigned long long)count_old * sizeof(art_dsp_state)}, {vo, (unsigned long long)count_old * 4ull}};
    const Range news[2] = {{sn, (unsigned long long)count * sizeof(art_dsp_state)}, {vn, (unsigned long long)count * 4ull}};
    for (const Range& o : olds)
      for (const Range& n : news)
        if (o.p && n.p && o.bytes && o.p < n.p + n.bytes && n.p < o.p + o.bytes)
          return fail(c, ART_E_INVALID, "%s: an old and a new array overlap (the call is out of place only)", __func__);
  }
  if (c->devs.empty()) return fail(c, ART_E_STATE, "%s: the context has no device", __func__);
  DspFollowArgs a{};
  a.state_old = reinterpret_cast<const uint8_t*>(d_state_old);
  a.volume_old = d_volume_old;
  a.state_new = reinterpret_cast<uint8_t*>(d_state_new);
  a.volume_new = d_volume_new;
  a.fan_src = d_fan_src;
  a.T_new = target_count_new; a.T_old = target_count_old; a.F_old = fan_count_old;
  a.count = (uint32_t)count;
  a.new_volume = new_volume;
  a.wide = ((so | sn) & 15) == 0 ? 1 : 0;
  for (int32_t t = 0; t < target_count_new; ++t) a.target_src[t] = (int16_t)target_src[t];
  Device& dv = c->devs[0];
  HIP_TRY(c, hipSetDevice(dv.id));
  launch_dsp_sources_follow(a, static_cast<hipStream_t>(stream));
  HIP_TRY(c, hipGetLastError());
  return ART_OK;
}

}  // extern "C"
