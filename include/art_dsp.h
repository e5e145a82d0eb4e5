/*
 * art_dsp.h — per-sample audio DSP of the spatializer (SURVEY.md §8 f rank 1), the direct consumer
 * of the ray tracer's AudioTargetRTSettings.
 *
 * Reference (paths relative to "Assets/C# Scripts/"):
 *   AudioSpatializer.OnAudioFilterRead   Audio/AudioTarget/AudioSpatializer.cs:70-87
 *     muffleDSP.Process                  Audio/AudioTarget/MuffleDSP.cs:13-32, LowPass :38-45
 *     reverbDSP.Process                  Audio/AudioTarget/ReverbDSP.cs:10-24
 *     binauralDSP.Process                Audio/AudioTarget/BinauralDSP.cs:15-82, LowPass :87-94,
 *                                        HighPass :97-106
 *     volume multiplier                  AudioSpatializer.cs:79-86
 *   cached inputs (main thread)          AudioSpatializer.cs:61-67 (local direction, distance)
 *   settings                             DataTypes/AudioSpatializerSettings.cs:4-45
 *   curves                               DataTypes/NativeSampledAnimationCurve.cs:64-89
 *
 * One art_audio_source = one AudioSpatializer's OnAudioFilterRead call: an interleaved buffer
 * processed in place, plus the filter state the C# structs keep between calls. The per-buffer
 * scalars (curve lookups, filter coefficients, binaural gains with atan2/sin/cos) are computed on
 * the host; the per-sample recurrences run on the GPU, one lane per source (both channels).
 *
 * The audio tick (art_dsp_tick_*) is the main-thread link between the two:
 *   AudioTargetManager.UpdateAudioTargetSettings -> AudioSpatializer.UpdateSpatializer
 *     -> OnLateUpdate                    Audio/AudioTarget/AudioSpatializer.cs:55-67
 *        worldDir = PercievedAudioPosition - listener.position
 *        cachedLocalDir = normalize(InverseTransformDirection(worldDir))
 *        cachedListenerDistance = distance(transform.position, listener.position)
 * followed by the per-buffer scalars above. It turns the settings section of a frame's result blocks
 * (art_launch_device, art_device.h) into art_dsp_source_params on the device, on the caller's
 * stream and without a host round trip; art_dsp_tick_params_host is the same computation on the
 * host. InverseTransformDirection is engine-native: the contract is math.mul(math.inverse(q), v)
 * with q the listener's rotation (rotation only).
 */
#ifndef ART_DSP_H
#define ART_DSP_H

#include "art.h"

#ifdef __cplusplus
extern "C" {
#endif

/* StereoFloat (DataTypes/StereoFloat.cs:5-14) */
typedef struct { float left, right; } art_stereo;

/* Filter state of one AudioSpatializer (in/out; zero-initialised like the C# structs). */
typedef struct {
    art_stereo previous_muffle;  /* MuffleDSP.previousMuffle (MuffleDSP.cs:9) */
    art_stereo previous_lp;      /* BinauralDSP.previousLP (BinauralDSP.cs:9) */
    art_stereo previous_hp;      /* BinauralDSP.previousHP (:10) */
    art_stereo previous_input;   /* BinauralDSP.previousInput (:11) */
} art_dsp_state;

/* AudioSpatializerSettings fields the per-sample chain reads (AudioSpatializerSettings.cs:8-45). */
typedef struct {
    float pan_strength;                       /* :8 */
    float rear_attenuation_strength;          /* :12 */
    int32_t distance_based_panning;           /* :15 (bool) */
    float max_pan_distance;                   /* :16 */
    int32_t distance_based_rear_attenuation;  /* :19 (bool) */
    float max_rear_attenuation_distance;      /* :20 */
    float max_elevation_effect_distance;      /* :23 */
    float low_pass_cutoff_min, low_pass_cutoff_max;    /* :26 */
    float low_pass_volume;                    /* :29 */
    float high_pass_cutoff_min, high_pass_cutoff_max;  /* :32 */
    float high_pass_volume;                   /* :35 */
    art_curve muffle_curve;                   /* :38 (baked) */
    float muffle_cutoff_min, muffle_cutoff_max;        /* :39 */
    art_curve reverb_volume_curve;            /* :45 (baked) */
    float reverb_dry_boost_min, reverb_dry_boost_max;  /* :44 */
} art_spatializer_settings;

/* One OnAudioFilterRead call of one AudioSpatializer. */
typedef struct {
    float* data;              /* interleaved samples, frames * channels, processed in place */
    int32_t frames;           /* samples per channel */
    int32_t channels;         /* only 2 is processed (AudioSpatializer.cs:72); others are left as is */
    float muffle_strength;    /* audioTargetSettings.MuffleStrength */
    float reverb_volume;      /* audioTargetSettings.ReverbVolume */
    float local_dir[3];       /* cachedLocalDir (AudioSpatializer.cs:64) */
    float listener_distance;  /* cachedListenerDistance (:66) */
    float volume_multiplier;  /* volumeMultiplier (:18) */
    art_dsp_state* state;     /* in/out */
} art_audio_source;

/* Process count sources (synchronous: buffers and states are updated when this returns). */
ART_API int art_dsp_process(art_ctx* ctx, const art_spatializer_settings* settings, art_audio_source* sources,
                            int32_t count, int32_t sample_rate);

/* Per-buffer scalars of one stereo source, as art_dsp_process derives them on the host. */
typedef struct {
    float muffle_alpha;       /* LowPass alpha of the muffle cutoff (MuffleDSP.cs:40-42) */
    float dry_boost;          /* ReverbDSP.cs:12-13 */
    float gain_left, gain_right;  /* BinauralDSP sampleModification (:48-50) */
    float filter_alpha;       /* low-pass alpha (elevation <= 0) or high-pass alpha (:65-76, :89-101) */
    float volume;             /* volume multiplier */
    int32_t flags;            /* bit 0: muffle active (:22); bit 1: low pass (else high pass) (:63) */
    int32_t reserved;
} art_dsp_source_params;

ART_API int art_dsp_source_params_get(const art_spatializer_settings* settings, const art_audio_source* source,
                                      int32_t sample_rate, art_dsp_source_params* out);

/* Device-resident batch (servers, bench): count stereo sources of `frames` samples each, stored
 * back to back in d_data (float [count][frames][2]); d_params (art_dsp_source_params[count]) and
 * d_state (art_dsp_state[count]) are device arrays. Enqueued on `stream`, not synchronised. */
ART_API int art_dsp_process_device(art_ctx* ctx, float* d_data, const art_dsp_source_params* d_params,
                                   art_dsp_state* d_state, int32_t count, int32_t frames, void* stream);

/* Diagnostics (tests, ABI 3.14): the kernel the context's last per-sample DSP call launched, so a
 * test knows which kernel it compared (art_dsp_process, art_dsp_process_device and art_dsp_tick_device
 * pick the tiled kernel, or the lane kernel when d_data is not 8-byte aligned, the batch reaches
 * 2^31 - 1 bytes, or ART_DSP_KERNEL=lane is set in the environment; the listener mix has one kernel).
 * ART_DSP_KERNEL_NONE before the first call and after a call that had nothing to launch. A host-side
 * decision: it does not synchronise. ART_E_INVALID for a NULL context, ART_E_UNSUPPORTED on the CPU
 * backend. */
#define ART_DSP_KERNEL_NONE  0
#define ART_DSP_KERNEL_TILED 1   /* dsp_tiled_kernel: one lane per (source, channel), tiles through LDS */
#define ART_DSP_KERNEL_LANE  2   /* dsp_kernel: one lane per source, direct loads */
#define ART_DSP_KERNEL_MIX   3   /* dsp_mix_kernel: the listener mix */
ART_API int art_debug_last_dsp_kernel(art_ctx* ctx);

/* ---- audio tick (ABI 3.5): spatializer parameters from a frame's result blocks ---------------- */

/* The AudioListener's transform (one per fan): position, rotation as a quaternion (x, y, z, w). */
typedef struct { float position[3]; float rotation[4]; } art_listener;   /* 28 B; one per fan */

/* Host twin, context-free (works with the CPU backend's frames and in tests): source s = f*T + t,
 * out[f*T + t] from fans[f].settings[t], listeners[f] and target_positions[3*t..] (the bound scene's
 * target positions, the JobBatch snapshot); volume = float[fan_count*T], NULL = 1.0f.
 * Both curves must be valid (baked, sample_count >= 2), else ART_E_INVALID. */
ART_API int art_dsp_tick_params_host(const art_spatializer_settings* settings, int32_t sample_rate,
        const art_listener* listeners, const art_fan* fans, int32_t fan_count,
        const float* target_positions, int32_t target_count,
        const float* volume, art_dsp_source_params* out);

/* Copy the scalars, upload the two baked curves to the context's first device; synchronous.
 * Both curves must be valid, else ART_E_INVALID (the device cannot refuse a single source). */
ART_API int art_dsp_settings_bind(art_ctx* ctx, const art_spatializer_settings* settings, int32_t sample_rate);

/* d_block / out_flags / fan_count as given to art_launch_device; d_listeners = art_listener[fan_count],
 * d_volume = float[fan_count*T] or NULL, d_params = art_dsp_source_params[fan_count*T] (all HBM).
 * Enqueued on `stream`, not synchronised. The block is only read. The tick reads the bound scene's
 * target positions, so it is ordered like a frame: after the last art_targets_sync, after a frame on
 * another stream, and a later sync, bind or schedule orders itself after it.
 * ART_E_STATE without a bound scene or bound settings or while a host frame is in flight;
 * ART_E_INVALID for a bound frame without ART_STAGE_REDUCE (no settings section). */
ART_API int art_dsp_tick_params_device(art_ctx* ctx, const void* d_block, uint32_t out_flags, int32_t fan_count,
        const art_listener* d_listeners, const float* d_volume, art_dsp_source_params* d_params, void* stream);

/* The step above, then the per-sample chain over d_data = float[fan_count*T][frames][2] and
 * d_state[fan_count*T]; d_params is written (callers may read it back). Two launches on `stream`,
 * no host work between them. */
ART_API int art_dsp_tick_device(art_ctx* ctx, const void* d_block, uint32_t out_flags, int32_t fan_count,
        const art_listener* d_listeners, const float* d_volume, float* d_data, art_dsp_state* d_state,
        int32_t frames, art_dsp_source_params* d_params, void* stream);

/* ---- settings per target (ABI 3.15): a table of settings classes and a class map --------------- */

/* Every AudioSpatializer carries its own settings (AudioSpatializer.cs:10-11, baked in Awake :38-39,
 * beside its volumeMultiplier :18). A settings class is one art_spatializer_settings; a context binds a
 * table of K classes (1 <= K <= 256) and each target of the scene names one class through the class
 * map, uint8 class_of[T]. Source s = f*T + t is evaluated with settings[class_of[t]]; the listener
 * step, the target position, the volume, the sample rate (one per table) and the record are as above.
 * The contract, literally:
 *   out[f*T + t] = what art_dsp_tick_params_host writes for that source when it is given
 *                  settings[class_of[t]] as its single settings
 *
 * Host twin, context-free: settings = art_spatializer_settings[class_count]; target_class =
 * uint8[target_count], or NULL = every target is class 0; the other arguments as
 * art_dsp_tick_params_host. ART_E_INVALID, with nothing written, when class_count is outside [1, 256],
 * when any class has a curve that is not valid (both curves of every class, used or not, as for the
 * device bind), or when a map entry is >= class_count. */
ART_API int art_dsp_tick_params_classes_host(const art_spatializer_settings* settings, int32_t class_count,
        int32_t sample_rate, const art_listener* listeners, const art_fan* fans, int32_t fan_count,
        const float* target_positions, int32_t target_count,
        const uint8_t* target_class /* uint8[target_count] or NULL = all class 0 */,
        const float* volume, art_dsp_source_params* out);

/* Copy the class_count records and upload the table and all 2 * class_count curves (each with its own
 * sample_count and length) to the context's first device, as one packed image in one copy. Ordered
 * and synchronous like art_dsp_settings_bind: it waits for a pending reader before it replaces
 * anything. It replaces any earlier bind of either kind; art_dsp_settings_bind is the bind of one
 * class. A bind does not touch the class map. ART_E_INVALID for class_count outside [1, 256] or a
 * curve that is not valid, ART_E_STATE while a frame is in flight, ART_E_UNSUPPORTED on the CPU
 * backend. */
ART_API int art_dsp_settings_bind_classes(art_ctx* ctx, const art_spatializer_settings* settings,
        int32_t class_count, int32_t sample_rate);

/* The class map: host state of the context. count in [0, 256]; 0 is the initial state and means
 * "every target is class 0". Pure host calls: no synchronisation, and they work on the CPU backend
 * (as art_target_follow_map does). _get copies min(cap, count) entries and returns the count.
 * ART_E_INVALID for a NULL context, a count outside [0, 256], cap < 0, or a NULL array with a
 * positive count / cap. Entries are checked against the bound class count by the tick, not here. */
ART_API int art_dsp_target_classes_set(art_ctx* ctx, const uint8_t* cls, int32_t count);
ART_API int art_dsp_target_classes_get(art_ctx* ctx, uint8_t* out, int32_t cap);

/* The tick under classes. art_dsp_tick_params_device, art_dsp_tick_device and
 * art_dsp_tick_mix_device keep their signatures. With one class bound and an empty map they do what
 * they always did (the same kernel, the same arguments). With more classes or a non-empty map they
 * use the table and the map: still one launch for the parameter step, no extra host work, and the
 * map travels in the kernel's argument block (it is read before the call returns and is
 * stream-ordered with the launch: a later art_dsp_target_classes_set does not reach a tick already
 * enqueued). Checked before anything is enqueued:
 *   ART_E_STATE  the map is not empty and its length differs from the bound frame's target count
 *                (the caller's check that it followed a count change);
 *   ART_E_STATE  a map entry is >= the bound class count.
 * A churn that keeps the target count (a remove plus an add) cannot be detected by length: moving
 * the map after target churn is the caller's duty, exactly as for d_state (below). */

/* ---- listener mix (ABI 3.6): one dry buffer per target in, one mix per fan out ------------------ */

/* A server with one listener per fan: the scene's T audio targets are shared by every fan, so there
 * is one dry buffer per target and tick, and a listener hears the sum of its T sources. Sources are
 * numbered s = f*T + t as in the tick. For fan f, frame i, channel c:
 *   y[f,t][i][c] = the per-sample chain (muffle, reverb, binaural, volume, as art_dsp_process_device
 *                  runs it) over dry[t][.][c] with params[s], continuing from state[s]
 *   mix[f][i][c] = (((y[f,0] + y[f,1]) + y[f,2]) + ... + y[f,T-1])[i][c]
 * The adds are fp32, one per target, in ascending t, starting from y[f,0] itself (a -0.0f survives
 * at T = 1), never contracted. state[s] afterwards is what art_dsp_process_device leaves for the
 * same source and input; dry is only read; mix is overwritten. A source whose params carry flag bit
 * 2 (not stereo; the tick never produces it) contributes its dry frames unchanged and keeps its
 * state (AudioSpatializer.cs:72). Unity's mixer is closed: this order is the project's definition
 * (DESIGN.md 3a).
 *
 * d_dry float[T][frames][2], d_params / d_state [fan_count*T], d_mix float[fan_count][frames][2];
 * enqueued on `stream`, not synchronised. ART_OK and no launch for fan_count == 0 or frames == 0;
 * otherwise ART_E_INVALID for target_count < 1, a NULL buffer, or d_dry / d_mix not 8-byte aligned,
 * and ART_E_UNSUPPORTED when target_count*frames*8 or fan_count*frames*8 reaches 2^31 bytes. */
ART_API int art_dsp_mix_device(art_ctx* ctx, const float* d_dry, const art_dsp_source_params* d_params,
        art_dsp_state* d_state, int32_t fan_count, int32_t target_count, int32_t frames,
        float* d_mix, void* stream);

/* art_dsp_tick_params_device, then the above with T = the bound frame's: two launches on
 * `stream`, no host work between them; same ordering rules and errors as art_dsp_tick_device,
 * and art_dsp_mix_device's for d_dry / d_mix (checked before anything is enqueued). */
ART_API int art_dsp_tick_mix_device(art_ctx* ctx, const void* d_block, uint32_t out_flags, int32_t fan_count,
        const art_listener* d_listeners, const float* d_volume, const float* d_dry,
        art_dsp_state* d_state, int32_t frames, art_dsp_source_params* d_params,
        float* d_mix, void* stream);

/* Host twin, context-free (works beside the CPU backend): the contract above, literally. */
ART_API int art_dsp_mix_host(const art_dsp_source_params* params, art_dsp_state* state, const float* dry,
        int32_t fan_count, int32_t target_count, int32_t frames, float* mix);

/* ---- sources follow the targets (ABI 3.13): d_state / d_volume after a target count change ------- */

/* The tick and the mix number sources s = f*T + t. When T changes, or a swap-back moves the last
 * target into a hole, every fan's filter states and volumes sit at the wrong index. These two calls
 * move them to the new numbering, out of place, by a target map (art_target_follow_map,
 * art_colliders.h) and an optional fan map (listeners that join and leave in the same pass).
 *
 * The contract is the host twin, literally. For f < fan_count_new and t < target_count_new:
 *   s  = f * target_count_new + t
 *   fo = fan_src ? fan_src[f] : f
 *   to = target_src[t]
 *   if 0 <= fo < fan_count_old and 0 <= to < target_count_old:
 *     state_new[s]  = the 32 bytes of state_old[fo * target_count_old + to], bit for bit
 *     volume_new[s] = volume_old ? volume_old[fo * target_count_old + to] : new_volume
 *   else (a new source):
 *     state_new[s]  = 32 zero bytes (the zero-initialised C# structs)
 *     volume_new[s] = new_volume
 * A fan index out of range, on either side, means "new listener" (the device cannot refuse it).
 * volume_new NULL: no volumes are written. volume_old NULL with volume_new set: every source gets
 * new_volume. The tick's default for a NULL volume array is 1.0f: that is the usual new_volume.
 * The old arrays are only read; old and new arrays must not overlap.
 *
 * Host twin, context-free: ART_E_INVALID for a negative count; ART_OK with nothing written when
 * fan_count_new == 0 or target_count_new == 0; otherwise ART_E_INVALID for a NULL target_src or
 * state_new, a NULL state_old with fan_count_old * target_count_old > 0, or a target_src entry
 * outside [-1, target_count_old) (checked before anything is written). */
ART_API int art_dsp_sources_follow_host(const int32_t* target_src, int32_t target_count_new, int32_t target_count_old,
        const int32_t* fan_src, int32_t fan_count_new, int32_t fan_count_old,
        const art_dsp_state* state_old, const float* volume_old,
        art_dsp_state* state_new, float* volume_new, float new_volume);

/* The same on the context's first device, one launch enqueued on `stream`: no synchronisation, no
 * event, no host round trip (the target map travels in the kernel's argument block; target_src is
 * read before the call returns). It reads nothing of the scene, so it takes no part in the ordering
 * of frames and syncs: the caller's stream orders it against the ticks that use the arrays. The arrays
 * need 4-byte alignment only (16-byte accesses when both state arrays allow them).
 * target_src NULL = the store's follow map: target_count_new and target_count_old must then equal
 * art_target_synced_count and the follow map's base count, else ART_E_INVALID (the caller's check
 * that its idea of T agrees with the store's). With a host target_src the call needs no store and no
 * bound scene. d_fan_src is a device array int32[fan_count_new], or NULL = identity.
 * ART_E_INVALID for a negative count, a required pointer that is NULL, a misaligned pointer, an old
 * array that overlaps a new one (a range check on the host), or a target_src entry outside
 * [-1, target_count_old). ART_OK and no launch when fan_count_new == 0 or target_count_new == 0.
 * ART_E_UNSUPPORTED when a target count exceeds the frame limit (256), when
 * fan_count_new * target_count_new exceeds 2^31 - 1, or on the CPU backend. */
ART_API int art_dsp_sources_follow_device(art_ctx* ctx,
        const int32_t* target_src /* host, or NULL = the store's follow map */,
        int32_t target_count_new, int32_t target_count_old,
        const int32_t* d_fan_src /* device int32[fan_count_new], or NULL = identity */,
        int32_t fan_count_new, int32_t fan_count_old,
        const art_dsp_state* d_state_old, const float* d_volume_old,
        art_dsp_state* d_state_new, float* d_volume_new, float new_volume, void* stream);

/* The class map (ABI 3.15) follows the targets with the semantics of art_dsp_sources_follow_host for
 * one fan: new[t] = old[target_src[t]] when 0 <= target_src[t] < target_count_old, new_class when it
 * is -1. Host only (works on the CPU backend, no synchronisation). target_src NULL = the store's
 * follow map, with the checks of art_dsp_sources_follow_device: the counts must equal
 * art_target_synced_count and the follow map's base count, else ART_E_INVALID. target_count_old must
 * equal the map's current length unless the map is empty; an empty map is treated as all zeros
 * (and becomes a map of target_count_new entries). ART_E_INVALID also for a negative count or a
 * target_src entry outside [-1, target_count_old); ART_E_UNSUPPORTED for a count above 256. Nothing
 * changes on an error. Call it before art_target_follow_mark, like the move of d_state: the order
 * after target churn is art_targets_sync, art_dsp_target_classes_follow,
 * art_dsp_sources_follow_device, art_target_follow_mark. */
ART_API int art_dsp_target_classes_follow(art_ctx* ctx,
        const int32_t* target_src /* host, or NULL = the store's follow map */,
        int32_t target_count_new, int32_t target_count_old, uint8_t new_class);

#ifdef __cplusplus
}
#endif
#endif /* ART_DSP_H */
