"""Per-sample spatializer DSP (include/art_dsp.h; SURVEY.md §8 f rank 1).

Mirrors AudioSpatializer.OnAudioFilterRead (Audio/AudioTarget/AudioSpatializer.cs:70-87): each
AudioSource holds an interleaved stereo buffer processed in place and the filter state the C#
MuffleDSP / BinauralDSP structs keep between calls. The product path runs on the GPU through
libart.so; there is no CPU fallback.

The audio tick (tick_params_host, bind_settings, tick_params_device, tick_device) is the main-thread
link in front of it (AudioSpatializer.UpdateSpatializer / OnLateUpdate, AudioSpatializer.cs:55-67):
the settings section of a frame's result blocks and each fan's listener become the per-buffer
scalars, on the device and on the caller's stream, or on the host.

The listener mix (mix_device, tick_mix_device, mix_host) is the server form of the chain: one dry
buffer per audio target in, shared by every fan, and one mix per fan out, the fan's T sources summed
in ascending target order (include/art_dsp.h has the contract).

sources_follow_device / sources_follow_host move the per-source filter states and volumes to the new
numbering s = f * T + t after targets were added or removed (TargetStore.follow_map, art/targets.py).

Settings per target (bind_settings_classes, set_target_classes / get_target_classes,
follow_target_classes, tick_params_classes_host): every AudioSpatializer carries its own settings
(AudioSpatializer.cs:10-11), so a context binds a table of settings classes and a class map names each
target's class; the tick entry points then evaluate source f * T + t with classes[map[t]].
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import abi


def _linear_curve(n: int = 50) -> np.ndarray:
    # NativeSampledAnimationCurve.Default (NativeSampledAnimationCurve.cs:92-98) bakes Unity's
    # closed-source AnimationCurve.Evaluate: the baked table is an input; a ramp stands in for it.
    return (np.arange(n, dtype=np.float32) / np.float32(n - 1)).astype(np.float32)


@dataclass
class SpatializerSettings:
    """AudioSpatializerSettings (DataTypes/AudioSpatializerSettings.cs:4-45), Default at :47-73."""
    pan_strength: float = 0.8
    rear_attenuation_strength: float = 0.2
    distance_based_panning: bool = True
    max_pan_distance: float = 5.0
    distance_based_rear_attenuation: bool = True
    max_rear_attenuation_distance: float = 15.0
    max_elevation_effect_distance: float = 12.0
    low_pass_cutoff: tuple = (5000.0, 22000.0)
    low_pass_volume: float = 0.85
    high_pass_cutoff: tuple = (25.0, 150.0)
    high_pass_volume: float = 1.15
    muffle_curve: np.ndarray = field(default_factory=_linear_curve)
    muffle_curve_length: float = 1.0
    muffle_cutoff: tuple = (75.0, 8000.0)
    reverb_volume_curve: np.ndarray = field(default_factory=_linear_curve)
    reverb_volume_curve_length: float = 1.0
    reverb_dry_boost: tuple = (1.0, 3.0)

    def to_c(self) -> abi.art_spatializer_settings:
        self._mc = np.ascontiguousarray(self.muffle_curve, np.float32)
        self._rc = np.ascontiguousarray(self.reverb_volume_curve, np.float32)
        fp = C.POINTER(C.c_float)
        return abi.art_spatializer_settings(
            self.pan_strength, self.rear_attenuation_strength, int(self.distance_based_panning),
            self.max_pan_distance, int(self.distance_based_rear_attenuation), self.max_rear_attenuation_distance,
            self.max_elevation_effect_distance, self.low_pass_cutoff[0], self.low_pass_cutoff[1], self.low_pass_volume,
            self.high_pass_cutoff[0], self.high_pass_cutoff[1], self.high_pass_volume,
            abi.art_curve(self._mc.ctypes.data_as(fp), self._mc.size, self.muffle_curve_length),
            self.muffle_cutoff[0], self.muffle_cutoff[1],
            abi.art_curve(self._rc.ctypes.data_as(fp), self._rc.size, self.reverb_volume_curve_length),
            self.reverb_dry_boost[0], self.reverb_dry_boost[1])


@dataclass
class AudioSource:
    """One AudioSpatializer: its buffer for this OnAudioFilterRead call, the per-buffer inputs and
    the persistent filter state."""
    data: np.ndarray                     # float32 [frames * channels], processed in place
    channels: int = 2
    muffle_strength: float = 0.0         # audioTargetSettings.MuffleStrength
    reverb_volume: float = 0.0           # audioTargetSettings.ReverbVolume
    local_dir: tuple = (0.0, 0.0, 1.0)   # cachedLocalDir (AudioSpatializer.cs:64)
    listener_distance: float = 1.0       # cachedListenerDistance (:66)
    volume_multiplier: float = 1.0       # volumeMultiplier (:18)
    state: np.ndarray = field(default_factory=lambda: np.zeros(1, abi.DSP_STATE))

    def to_c(self) -> abi.art_audio_source:
        assert self.data.dtype == np.float32 and self.data.flags["C_CONTIGUOUS"]
        assert self.state.dtype == abi.DSP_STATE and self.state.flags["C_CONTIGUOUS"]
        return abi.art_audio_source(
            self.data.ctypes.data_as(C.POINTER(C.c_float)), self.data.size // self.channels, self.channels,
            self.muffle_strength, self.reverb_volume, (C.c_float * 3)(*self.local_dir), self.listener_distance,
            self.volume_multiplier, self.state.ctypes.data_as(C.POINTER(abi.art_dsp_state)))

    def copy(self) -> "AudioSource":
        return AudioSource(self.data.copy(), self.channels, self.muffle_strength, self.reverb_volume, self.local_dir,
                           self.listener_distance, self.volume_multiplier, self.state.copy())


def sources_to_c(sources: list[AudioSource]):
    arr = (abi.art_audio_source * max(1, len(sources)))()
    for i, s in enumerate(sources):
        arr[i] = s.to_c()
    return arr


def process(ctx, settings: SpatializerSettings, sources: list[AudioSource], sample_rate: int = 48000):
    """AudioSpatializer.OnAudioFilterRead for every source, on the GPU (art_dsp_process)."""
    st = settings.to_c()
    arr = sources_to_c(sources)
    rc = ctx.lib.art_dsp_process(ctx.ptr, C.byref(st), arr, len(sources), sample_rate)
    if rc:
        ctx._raise(rc)


def source_params(settings: SpatializerSettings, source: AudioSource, sample_rate: int = 48000) -> np.ndarray:
    """The per-buffer scalars art_dsp_process derives on the host (for the device-resident API)."""
    st = settings.to_c()
    src = source.to_c()
    out = np.zeros(1, abi.DSP_SOURCE_PARAMS)
    rc = abi.load_library().art_dsp_source_params_get(C.byref(st), C.byref(src), sample_rate,
                                                      out.ctypes.data_as(C.POINTER(abi.art_dsp_source_params)))
    if rc:
        raise ValueError(f"art_dsp_source_params_get: {rc}")
    return out


def process_device(ctx, d_data, d_params, d_state, count: int, frames: int, stream: int | None = None):
    """art_dsp_process_device on `stream` (not synchronised): d_data float [count][frames][2], processed
    in place; buffers are torch tensors or raw device pointers (d_data needs 4-byte alignment only)."""
    rc = ctx.lib.art_dsp_process_device(ctx.ptr, _dptr(d_data), _dptr(d_params), _dptr(d_state), count, frames, stream)
    if rc:
        ctx._raise(rc)


def debug_last_dsp_kernel(ctx) -> int:
    """art_debug_last_dsp_kernel: the abi.ART_DSP_KERNEL_* the context's last per-sample DSP call launched."""
    rc = ctx.lib.art_debug_last_dsp_kernel(ctx.ptr)
    if rc < 0:
        ctx._raise(rc)
    return rc


@dataclass
class Listener:
    """The AudioListener's transform: position and rotation (quaternion x, y, z, w)."""
    position: tuple = (0.0, 0.0, 0.0)
    rotation: tuple = (0.0, 0.0, 0.0, 1.0)


def listeners_array(listeners) -> np.ndarray:
    """Listener objects (or an abi.LISTENER array) as one abi.LISTENER array, one record per fan."""
    if isinstance(listeners, np.ndarray):
        assert listeners.dtype == abi.LISTENER
        return np.ascontiguousarray(listeners)
    out = np.zeros(len(listeners), abi.LISTENER)
    for i, l in enumerate(listeners):
        out[i]["position"] = l.position
        out[i]["rotation"] = l.rotation
    return out


def tick_params_host(settings: SpatializerSettings, listeners, fan_settings: np.ndarray, target_positions: np.ndarray,
                     volume: np.ndarray | None = None, sample_rate: int = 48000) -> np.ndarray:
    """art_dsp_tick_params_host: the spatializer parameters of every (fan, target) source from the
    fans' settings (abi.SETTINGS [fan_count, T], a frame's FanOutputs.settings), one listener per
    fan and the scene's target positions; returns DSP_SOURCE_PARAMS [fan_count * T]."""
    fs = np.ascontiguousarray(fan_settings)
    assert fs.dtype == abi.SETTINGS and fs.ndim == 2
    S, T = fs.shape
    ls = listeners_array(listeners)
    assert ls.size == S
    tp = np.ascontiguousarray(target_positions, np.float32).reshape(-1, 3)
    assert tp.shape[0] == T
    fans = (abi.art_fan * max(S, 1))()
    for i in range(S):
        fans[i].settings = fs[i].ctypes.data
    vol = None
    if volume is not None:
        vol = np.ascontiguousarray(volume, np.float32).reshape(-1)
        assert vol.size == S * T
    out = np.zeros(S * T, abi.DSP_SOURCE_PARAMS)
    st = settings.to_c()
    rc = abi.load_library().art_dsp_tick_params_host(C.byref(st), sample_rate, ls.ctypes.data, fans, S, tp.ctypes.data, T,
                                                     vol.ctypes.data if vol is not None else None, out.ctypes.data)
    if rc:
        raise ValueError(f"art_dsp_tick_params_host: {abi.ERROR_NAMES.get(rc, rc)}")
    return out


def _dptr(x) -> int | None:
    """A device buffer as the C ABI takes it: a torch tensor's data pointer, or a raw pointer / None."""
    if x is None or isinstance(x, int):
        return x
    assert x.is_contiguous()
    return x.data_ptr()


def bind_settings(ctx, settings: SpatializerSettings, sample_rate: int = 48000):
    """art_dsp_settings_bind: the spatializer settings of the later ticks (curves uploaded once)."""
    st = settings.to_c()
    rc = ctx.lib.art_dsp_settings_bind(ctx.ptr, C.byref(st), sample_rate)
    if rc:
        ctx._raise(rc)


def settings_table(classes):
    """SpatializerSettings objects as one art_spatializer_settings array (which keeps the curves alive)."""
    arr = (abi.art_spatializer_settings * max(1, len(classes)))()
    arr._curves = []
    for k, s in enumerate(classes):
        arr[k] = s.to_c()
        arr._curves.append((s._mc, s._rc))
    return arr


def tick_params_classes_host(classes, listeners, fan_settings: np.ndarray, target_positions: np.ndarray,
                             target_class=None, volume: np.ndarray | None = None, sample_rate: int = 48000) -> np.ndarray:
    """art_dsp_tick_params_classes_host: tick_params_host with one SpatializerSettings per class and
    target_class (uint8 [T], None = every target is class 0) naming each target's class."""
    fs = np.ascontiguousarray(fan_settings)
    assert fs.dtype == abi.SETTINGS and fs.ndim == 2
    S, T = fs.shape
    ls = listeners_array(listeners)
    assert ls.size == S
    tp = np.ascontiguousarray(target_positions, np.float32).reshape(-1, 3)
    assert tp.shape[0] == T
    fans = (abi.art_fan * max(S, 1))()
    for i in range(S):
        fans[i].settings = fs[i].ctypes.data
    cls = None
    if target_class is not None:
        cls = np.ascontiguousarray(target_class, np.uint8).reshape(-1)
        assert cls.size == T
    vol = None
    if volume is not None:
        vol = np.ascontiguousarray(volume, np.float32).reshape(-1)
        assert vol.size == S * T
    out = np.zeros(S * T, abi.DSP_SOURCE_PARAMS)
    table = settings_table(classes)
    rc = abi.load_library().art_dsp_tick_params_classes_host(
        table, len(classes), sample_rate, ls.ctypes.data, fans, S, tp.ctypes.data, T,
        cls.ctypes.data if cls is not None else None, vol.ctypes.data if vol is not None else None, out.ctypes.data)
    if rc:
        raise ValueError(f"art_dsp_tick_params_classes_host: {abi.ERROR_NAMES.get(rc, rc)}")
    return out


def bind_settings_classes(ctx, classes, sample_rate: int = 48000):
    """art_dsp_settings_bind_classes: one SpatializerSettings per class (table and curves uploaded once);
    the later ticks evaluate target t with classes[class map[t]] (set_target_classes)."""
    table = settings_table(classes)
    rc = ctx.lib.art_dsp_settings_bind_classes(ctx.ptr, table, len(classes), sample_rate)
    if rc:
        ctx._raise(rc)


def set_target_classes(ctx, target_class):
    """art_dsp_target_classes_set: the class of every target (uint8 [T]); empty = every target is class 0."""
    cls = np.ascontiguousarray(target_class, np.uint8).reshape(-1)
    rc = ctx.lib.art_dsp_target_classes_set(ctx.ptr, cls.ctypes.data if cls.size else None, cls.size)
    if rc:
        ctx._raise(rc)


def get_target_classes(ctx) -> np.ndarray:
    """art_dsp_target_classes_get: the class map, uint8 [count]."""
    out = np.zeros(256, np.uint8)
    n = ctx.lib.art_dsp_target_classes_get(ctx.ptr, out.ctypes.data, out.size)
    if n < 0:
        ctx._raise(n)
    return out[:n].copy()


def follow_target_classes(ctx, target_src, target_count_new: int, target_count_old: int, new_class: int = 0):
    """art_dsp_target_classes_follow: the class map moved to the new target numbering, new targets in
    new_class. target_src is a host int32 array, or None = the store's follow map. Before follow_mark."""
    ts = None
    if target_src is not None:
        ts = np.ascontiguousarray(target_src, np.int32).reshape(-1)
        assert ts.size == target_count_new
    rc = ctx.lib.art_dsp_target_classes_follow(ctx.ptr, None if ts is None else ts.ctypes.data, target_count_new,
                                               target_count_old, new_class)
    if rc:
        ctx._raise(rc)


def tick_params_device(ctx, d_block, fan_count: int, d_listeners, d_params, d_volume=None, out_flags: int = 0,
                       stream: int | None = None):
    """art_dsp_tick_params_device on `stream` (not synchronised); buffers are torch tensors or raw
    device pointers."""
    rc = ctx.lib.art_dsp_tick_params_device(ctx.ptr, _dptr(d_block), out_flags, fan_count, _dptr(d_listeners),
                                            _dptr(d_volume), _dptr(d_params), stream)
    if rc:
        ctx._raise(rc)


def tick_device(ctx, d_block, fan_count: int, d_listeners, d_data, d_state, frames: int, d_params, d_volume=None,
                out_flags: int = 0, stream: int | None = None):
    """art_dsp_tick_device on `stream` (not synchronised): the parameter step, then the per-sample
    chain over d_data (float [fan_count * T][frames][2]) and d_state."""
    rc = ctx.lib.art_dsp_tick_device(ctx.ptr, _dptr(d_block), out_flags, fan_count, _dptr(d_listeners), _dptr(d_volume),
                                     _dptr(d_data), _dptr(d_state), frames, _dptr(d_params), stream)
    if rc:
        ctx._raise(rc)


def mix_device(ctx, d_dry, d_params, d_state, fan_count: int, target_count: int, frames: int, d_mix,
               stream: int | None = None):
    """art_dsp_mix_device on `stream` (not synchronised): d_dry float [T][frames][2] (only read),
    d_params / d_state [fan_count * T], d_mix float [fan_count][frames][2] (overwritten)."""
    rc = ctx.lib.art_dsp_mix_device(ctx.ptr, _dptr(d_dry), _dptr(d_params), _dptr(d_state), fan_count, target_count, frames,
                                    _dptr(d_mix), stream)
    if rc:
        ctx._raise(rc)


def tick_mix_device(ctx, d_block, fan_count: int, d_listeners, d_dry, d_state, frames: int, d_params, d_mix, d_volume=None,
                    out_flags: int = 0, stream: int | None = None):
    """art_dsp_tick_mix_device on `stream` (not synchronised): the parameter step, then the listener
    mix over d_dry (float [T][frames][2]) into d_mix (float [fan_count][frames][2])."""
    rc = ctx.lib.art_dsp_tick_mix_device(ctx.ptr, _dptr(d_block), out_flags, fan_count, _dptr(d_listeners), _dptr(d_volume),
                                         _dptr(d_dry), _dptr(d_state), frames, _dptr(d_params), _dptr(d_mix), stream)
    if rc:
        ctx._raise(rc)


def sources_follow_host(target_src, target_count_old: int, fan_count_new: int, fan_count_old: int, state_old: np.ndarray,
                        volume_old: np.ndarray | None = None, fan_src=None, new_volume: float = 1.0,
                        want_volume: bool = True):
    """art_dsp_sources_follow_host: the states (abi.DSP_STATE [fan_count_old * T_old]) and volumes moved
    to the numbering s = f * T_new + t by target_src (int32 [T_new]) and fan_src (int32 [fan_count_new]
    or None = identity). Returns (state_new, volume_new); volume_new is None when want_volume is False."""
    ts = np.ascontiguousarray(target_src, np.int32).reshape(-1)
    T_new = ts.size
    fs = None if fan_src is None else np.ascontiguousarray(fan_src, np.int32).reshape(-1)
    assert fs is None or fs.size == fan_count_new
    n_old = fan_count_old * target_count_old
    assert state_old.dtype == abi.DSP_STATE and state_old.size == n_old and state_old.flags["C_CONTIGUOUS"]
    vo = None
    if volume_old is not None:
        vo = np.ascontiguousarray(volume_old, np.float32).reshape(-1)
        assert vo.size == n_old
    state_new = np.zeros(fan_count_new * T_new, abi.DSP_STATE)
    volume_new = np.zeros(fan_count_new * T_new, np.float32) if want_volume else None
    rc = abi.load_library().art_dsp_sources_follow_host(
        ts.ctypes.data, T_new, target_count_old, None if fs is None else fs.ctypes.data, fan_count_new, fan_count_old,
        state_old.ctypes.data, None if vo is None else vo.ctypes.data, state_new.ctypes.data,
        None if volume_new is None else volume_new.ctypes.data, new_volume)
    if rc:
        raise ValueError(f"art_dsp_sources_follow_host: {abi.ERROR_NAMES.get(rc, rc)}")
    return state_new, volume_new


def sources_follow_device(ctx, target_src, target_count_new: int, target_count_old: int, fan_count_new: int,
                          fan_count_old: int, d_state_old, d_state_new, d_volume_old=None, d_volume_new=None,
                          d_fan_src=None, new_volume: float = 1.0, stream: int | None = None):
    """art_dsp_sources_follow_device on `stream` (not synchronised), out of place. target_src is a host
    int32 array, or None = the store's follow map (the counts must then be the store's synced count and
    the map's base count); the other buffers are torch tensors or raw device pointers."""
    ts = None
    if target_src is not None:
        ts = np.ascontiguousarray(target_src, np.int32).reshape(-1)
        assert ts.size == target_count_new
    rc = ctx.lib.art_dsp_sources_follow_device(ctx.ptr, None if ts is None else ts.ctypes.data, target_count_new,
                                               target_count_old, _dptr(d_fan_src), fan_count_new, fan_count_old,
                                               _dptr(d_state_old), _dptr(d_volume_old), _dptr(d_state_new),
                                               _dptr(d_volume_new), new_volume, stream)
    if rc:
        ctx._raise(rc)


def mix_host(params: np.ndarray, state: np.ndarray, dry: np.ndarray, fan_count: int, target_count: int) -> np.ndarray:
    """art_dsp_mix_host: params (abi.DSP_SOURCE_PARAMS [fan_count * T]), state (abi.DSP_STATE
    [fan_count * T], updated in place), dry (float32 [T, frames * 2], only read); returns the mix,
    float32 [fan_count, frames * 2]."""
    n = fan_count * target_count
    assert params.dtype == abi.DSP_SOURCE_PARAMS and params.size == n and params.flags["C_CONTIGUOUS"]
    assert state.dtype == abi.DSP_STATE and state.size == n and state.flags["C_CONTIGUOUS"]
    d = np.ascontiguousarray(dry, np.float32).reshape(target_count, -1)
    frames = d.shape[1] // 2
    assert d.shape[1] == 2 * frames
    mix = np.zeros((fan_count, 2 * frames), np.float32)
    rc = abi.load_library().art_dsp_mix_host(params.ctypes.data, state.ctypes.data, d.ctypes.data, fan_count, target_count,
                                             frames, mix.ctypes.data)
    if rc:
        raise ValueError(f"art_dsp_mix_host: {abi.ERROR_NAMES.get(rc, rc)}")
    return mix
