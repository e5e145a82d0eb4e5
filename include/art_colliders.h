/*
 * art_colliders.h — the device-resident scene store, both halves: the collider lists (SURVEY.md
 * §8 f rank 2, the collider upload path on the near side of the ray tracer) and the audio-target
 * positions (the second half of this file).
 *
 * Reference (paths relative to "Assets/C# Scripts/"):
 *   NativeJobBatch<T>                       DataTypes/NativeJobBatch.cs:8-56
 *     Add                                   :27-30   (NextBatch.Add)
 *     RemoveAtSwapBack                      :31-34
 *     this[index] set                       :14-18   (an in-place update of NextBatch)
 *     UpdateJobBatch                        :36-50   (memcpy NextBatch -> JobBatch, every frame)
 *   AudioColliderManager.AddColiderToSystem Audio/AudioColliderManager.cs:42-62 (id = NextBatch.Length:
 *                                           Colliders/AudioOBBCollider.cs:18-22, AudioAABBCollider.cs:14-17,
 *                                           AudioSphereCollider.cs:14-17)
 *   AudioColliderManager.SwapRemove         Audio/AudioColliderManager.cs:90-105 (invalid ids skipped)
 *   AudioColliderManager.UpdateColiderInSystem :107-110 (collider[id] = GetBakedColliderStruct(),
 *                                           AudioOBBCollider.cs:23-26)
 *   AudioColliderManager.UpdateJobBatch     :115-122 (called once per frame, AudioRayTracer.cs:155)
 *
 * The reference copies every collider into the job snapshot each frame, and a GPU port of that
 * would upload every collider every frame. Here the context keeps the three collider lists
 * resident in HBM as decoded SoA records. The host side keeps the NextBatch mirror: add / set /
 * remove-at-swap-back touch only the mirror and mark records dirty. art_colliders_sync is
 * UpdateJobBatch: it uploads only the dirty records (one H2D copy) and decodes them on the device
 * (one kernel). With ART_CTX_RESIDENT_COLLIDERS set, art_schedule and art_scene_bind take the
 * colliders from the last sync (the JobBatch snapshot) instead of the desc's arrays.
 *
 * Baking a collider struct from its transform (GetBakedColliderStruct, AudioOBBCollider.cs:31-66)
 * stays with the caller: it uses the engine's transform and quaternion math, and its result (the
 * 20/26/16-byte struct) is the contract.
 *
 * The target half mirrors AudioTargetManager over NativeJobBatch<float3>:
 *   AudioTargetManager.AddAudioTargetToSystem      Audio/AudioTargetManager.cs:49-57 (the position is
 *                                                  appended, AudioTarget/AudioTargetRT.cs:40-44)
 *   AudioTargetManager.RemoveAudioTargetFromSystem :59-96 (the last position moves into the hole, :73, :95)
 *   AudioTargetManager.UpdateColiderInSystem       :97-100 -> AudioTargetRT.UpdateToAudioSystem
 *                                                  (AudioTarget/AudioTargetRT.cs:45-48), called for a target
 *                                                  that is not static and moved (:8-10, :53-62)
 *   AudioTargetManager.UpdateJobBatch              :105-110 (once per frame)
 * The context keeps the NextBatch mirror of the positions with dirty marks. art_targets_sync is
 * UpdateJobBatch: K moved targets cost an upload of K positions and, on a bound device scene, the
 * rebuild of those K targets' muffle cell lists; the BVH, the other targets' lists and the frame
 * layout stay. With ART_CTX_RESIDENT_TARGETS set, art_schedule and art_scene_bind take the
 * positions and the target count from the last target sync.
 */
#ifndef ART_COLLIDERS_H
#define ART_COLLIDERS_H

#include "art.h"

#ifdef __cplusplus
extern "C" {
#endif

/* collider kinds */
#define ART_KIND_SPHERE 0  /* art_sphere (16 B) */
#define ART_KIND_AABB   1  /* art_aabb (20 B) */
#define ART_KIND_OBB    2  /* art_obb (26 B) */

/* art_set_flags bit: frames read the resident store (desc collider arrays must be NULL / 0). */
#define ART_CTX_RESIDENT_COLLIDERS 0x20u

/* NativeJobBatch.Add: appends rec (a struct of the kind) to the kind's list; *out_id = its index
 * (the C# AudioColliderId). */
ART_API int art_collider_add(art_ctx* ctx, int32_t kind, const void* rec, int32_t* out_id);

/* NativeJobBatch[id] = rec (UpdateColiderInSystem). ART_E_INVALID if id is out of range. */
ART_API int art_collider_set(art_ctx* ctx, int32_t kind, int32_t id, const void* rec);

/* n updates of one kind in one call (ids[j] <- recs[j], recs packed back to back); all ids are
 * checked before anything changes. */
ART_API int art_collider_set_many(art_ctx* ctx, int32_t kind, const int32_t* ids, const void* recs, int32_t n);

/* RemoveAtSwapBack(id): the last record moves to id. Like AudioColliderManager.SwapRemove
 * (:92-93), an id out of range is skipped (returns ART_OK, nothing changes). */
ART_API int art_collider_remove_swapback(art_ctx* ctx, int32_t kind, int32_t id);

/* NativeJobBatch[id] get (the mirror, i.e. NextBatch, including unsynced changes). */
ART_API int art_collider_get(art_ctx* ctx, int32_t kind, int32_t id, void* rec);

/* NextBatch.Length of the kind (>= 0), or a negative error code. */
ART_API int art_collider_count(art_ctx* ctx, int32_t kind);

/* Drop every collider of every kind (the lists become empty; the next sync publishes that). */
ART_API int art_colliders_clear(art_ctx* ctx);

/* UpdateJobBatch for the three kinds: publish the mirror to every device of the context.
 * Stream-ordered, not synchronous: the dirty records' upload and decode are enqueued on the
 * context's stream ahead of the next frame (art_launch_device on another stream waits for them).
 * ART_E_STATE while a frame is in flight (the reference syncs after Complete). A count change
 * (add, remove, clear) unbinds a bound resident scene (the BVH's buffers are sized by the counts:
 * the next art_scene_bind / art_schedule builds them again) unless the scene was bound with a
 * reserved capacity (art_colliders_reserve, below) and every kind stays within it. */
ART_API int art_colliders_sync(art_ctx* ctx);

/* What the last art_colliders_sync moved. */
typedef struct {
    int32_t dirty_records;   /* records uploaded and decoded */
    int32_t full_prep;       /* 1 if a count changed, so every record's bounds were rebuilt on the device */
    int32_t reallocated;     /* 1 if the device capacity grew (every record uploaded) */
    int32_t cells_rebuilt;   /* 1 if the muffle direction-cell lists were rebuilt (a record left its motion slack) */
    uint64_t bytes_uploaded; /* H2D bytes of the sync (indices + records) */
} art_collider_sync_stats;

ART_API int art_colliders_last_sync(art_ctx* ctx, art_collider_sync_stats* out);

/* ------------------------------------------ colliders that appear and disappear (ABI 3.10) */

/* Room for up to `spheres`, `aabbs` and `obbs` colliders of each kind in scenes bound from now on
 * with ART_CTX_RESIDENT_COLLIDERS: a later art_colliders_sync that changes a count and keeps every
 * kind within its capacity keeps such a scene bound. The sync stays stream-ordered like a move and
 * allocates nothing (the store's lists, the BVH's buffers and the muffle cell lists are sized by the
 * capacity; the update image of up to min(total capacity, 2^16) records is allocated at the bind).
 * On the device the BVH's leaf order is sorted again in the scene's buffers, every node box is
 * recomputed and the cell lists are rebuilt: results are those of a fresh bind. With
 * ART_BVH_RESORT_DEN=d in the environment (scenes of up to 2^16 colliders) the sort runs only once
 * the adds and removes since the last one exceed 1/d of the colliders (0: never; the default is 1:
 * at every count change, the measured optimum, DESIGN.md §3b "Colliders that appear and
 * disappear"); in between, the labels (kind, index) that vanished leave their leaf positions to
 * the labels that appeared (RemoveAtSwapBack shortens a list from its end, so labels change only at
 * the tails; a survivor swapped into a hole is a changed record at an existing label) and the tail
 * of the leaf order is packed: any leaf order gives an exact BVH, only its tightness suffers.
 * A scene bound with more colliders of a kind than reserved is sized by its own count, and that
 * count is the kind's capacity. 0, 0, 0 (the default) = a count change unbinds, as before. Does not
 * touch a scene that is already bound. Reserve before the store's first sync: a store whose device
 * lists have to grow past their allocation unbinds once more.
 * Whether a scene has muffle cell lists, and their room, is decided from the capacity (and the
 * target capacity): a scene has lists for every count it can take, or for none.
 * ART_E_INVALID for a negative capacity, ART_E_UNSUPPORTED above the collider limit (2^24) in total,
 * ART_E_STATE while a frame is in flight.
 * Nothing new stays with the caller: the fan layout does not depend on the collider counts. */
ART_API int art_colliders_reserve(art_ctx* ctx, int32_t spheres, int32_t aabbs, int32_t obbs);
ART_API int art_collider_capacity(art_ctx* ctx, int32_t kind);   /* reserved capacity of the kind, or < 0 */

/* What the last art_colliders_sync did to the lists and to a bound scene (the CPU backend, which
 * keeps no device scene, reports kept_bound 0 and the counts). */
typedef struct {
    int32_t kept_bound;     /* 1: the bound scene followed the count change */
    int32_t added, removed; /* labels that appeared / vanished, all kinds */
    int32_t relabelled;     /* leaf positions whose reference was rewritten by the relabel kernel (read
                               back from device 0: art_colliders_last_resize waits for that sync) */
    int32_t bvh_rebuilt;    /* 1: the full kd build ran in place (the default; churn threshold, large scene, from/to empty) */
    int32_t levels_changed; /* 1: the tree's level count changed */
    int32_t cells_rebuilt;
    uint64_t bytes_uploaded;
} art_collider_resize_stats;
ART_API int art_colliders_last_resize(art_ctx* ctx, art_collider_resize_stats* out);

/* ------------------------------------------------------------------ audio targets (ABI 3.4) */

/* art_set_flags bit: frames read the resident target positions (desc.audio_target_positions must
 * be NULL and desc.audio_target_count 0). Combines freely with ART_CTX_RESIDENT_COLLIDERS.
 * art_fan_layout_get takes no context: pass it a copy of the desc with audio_target_count set to
 * art_target_synced_count (its positions pointer any non-NULL value; it is not read). */
#define ART_CTX_RESIDENT_TARGETS 0x800u

/* AddAudioTargetToSystem (:49-57): appends pos; *out_id = its index in the list. */
ART_API int art_target_add(art_ctx* ctx, const float pos[3], int32_t* out_id);

/* UpdateToAudioSystem (AudioTargetRT.cs:45-48): positions[id] = pos. ART_E_INVALID if id is out of
 * range. A set to the same 12 bytes marks nothing dirty. */
ART_API int art_target_set(art_ctx* ctx, int32_t id, const float pos[3]);

/* n updates in one call (ids[j] <- positions[3j..3j+2]); all ids are checked before anything
 * changes. */
ART_API int art_target_set_many(art_ctx* ctx, const int32_t* ids, const float* positions, int32_t n);

/* RemoveAudioTargetFromSystem (:59-96): the last position moves to id. An id out of range is
 * skipped (returns ART_OK, nothing changes), as art_collider_remove_swapback does. The colliders
 * owned by the swapped target keep their audio_target_id: re-numbering them (the reference's id
 * pool, :75-86, and the colliders' own updates) stays with the caller, through art_collider_set,
 * unless ART_CTX_TARGET_OWNERS_FOLLOW (below) is set. */
ART_API int art_target_remove_swapback(art_ctx* ctx, int32_t id);

/* art_set_flags bit (ABI 3.13): art_target_remove_swapback(id) with a valid id that is not the last
 * index also does what the reference does by itself: swapped.Id.Value = removeIndex
 * (Audio/AudioTargetManager.cs:86) drives AudioCollider.UpdateAudioTargetId
 * (Audio/Colliders/AudioCollider.cs:32,46-50), which rewrites AudioTargetId and pushes the collider
 * through UpdateColiderInSystem. Every record of the collider mirror, of all three kinds, whose
 * audio_target_id is the last index gets audio_target_id = id, exactly as art_collider_set would write
 * it: marked dirty, uploaded by the next art_colliders_sync, counted in the owner histogram there.
 * Records that name the removed id itself are left alone: in the reference they belong to the removed
 * GameObject and leave through their own OnDisable (the caller removes them, art_collider_remove_swapback).
 * A remove then dirties both stores; art_targets_sync and art_colliders_sync may follow in either
 * order, and the frame after both is that of a fresh bind. Without the flag nothing changes. */
#define ART_CTX_TARGET_OWNERS_FOLLOW 0x1000u

/* Records re-numbered by the most recent art_target_remove_swapback, per kind: spheres, AABBs, OBBs
 * (all 0 without the flag, for id == last and for an id out of range). */
ART_API int art_target_last_remove_owners(art_ctx* ctx, int32_t out[3]);

/* positions[id] of the mirror (NextBatch, including unsynced changes). */
ART_API int art_target_get(art_ctx* ctx, int32_t id, float pos[3]);

/* NextBatch.Length (>= 0), or a negative error code. */
ART_API int art_target_count(art_ctx* ctx);

/* The target count of the last art_targets_sync (what resident-target frames use), or a negative
 * error code. */
ART_API int art_target_synced_count(art_ctx* ctx);

/* Drop every target (the next sync publishes the empty list). */
ART_API int art_targets_clear(art_ctx* ctx);

/* UpdateJobBatch (:105-110): publish the mirror to every device of the context. Stream-ordered
 * exactly like art_colliders_sync (the same stream choice and fences). ART_E_STATE while a frame is
 * in flight. A count change (add, remove, clear) unbinds a bound resident-target scene: T is part
 * of the frame layout, so the next art_scene_bind / art_schedule builds everything again — unless
 * the scene was bound with a reserved capacity (art_targets_reserve, below) and the count stays
 * within it. */
ART_API int art_targets_sync(art_ctx* ctx);

/* What the last art_targets_sync moved. */
typedef struct {
    int32_t dirty_targets;      /* positions that changed since the last sync and are still in the list */
    int32_t count_changed;      /* 1 if the list's length changed (the first sync included) */
    int32_t lists_rebuilt;      /* targets whose muffle cell lists were rebuilt on their own */
    int32_t lists_full_rebuild; /* 1 if every target's lists were rebuilt (the entry arena compacted) */
    uint64_t bytes_uploaded;    /* H2D bytes of the sync (indices + positions) */
} art_target_sync_stats;

ART_API int art_targets_last_sync(art_ctx* ctx, art_target_sync_stats* out);

/* Diagnostics (synchronizes device 0): entries in use and capacity of the bound scene's muffle
 * cell-list arena, and the targets currently without lists because theirs did not fit. */
ART_API int art_debug_cells_arena(art_ctx* ctx, uint64_t* used, uint64_t* cap, uint32_t* dropped_targets);

/* ------------------------------------------- targets that appear and disappear (ABI 3.7) */

/* Room for up to `capacity` targets in scenes bound from now on with ART_CTX_RESIDENT_TARGETS:
 * a later art_targets_sync whose count stays in [1, capacity] keeps such a scene bound (it adds,
 * removes and re-indexes the targets on the device, stream-ordered like a move, and allocates
 * nothing). A scene bound with more targets than `capacity` is sized by its own count, and that
 * count is its capacity. 0 (the default) = a count change unbinds, as above. Does not touch a
 * scene that is already bound.
 * ART_E_INVALID for capacity < 0, ART_E_UNSUPPORTED above the target limit (256),
 * ART_E_STATE while a frame is in flight.
 *
 * What stays with the caller after a count change that kept the scene bound:
 *  - the fan-block stride follows the synced count: re-query art_fan_layout_get with
 *    art_target_synced_count (as after a rebind) and size d_block for it;
 *  - without ART_CTX_TARGET_OWNERS_FOLLOW: re-numbering the audio_target_id of the colliders a
 *    swapped target owns (art_collider_set), as art_target_remove_swapback says.
 * The tick's and the mix's source numbering s = f * T + t changes with T and with every swap-back:
 * art_dsp_sources_follow_device (art_dsp.h) moves d_state and d_volume to the new numbering on the
 * device, from the follow map below. */
ART_API int art_targets_reserve(art_ctx* ctx, int32_t capacity);
ART_API int art_target_capacity(art_ctx* ctx);          /* the reserved capacity, or < 0 */

/* What the last art_targets_sync did to the list and to a bound scene's lists. */
typedef struct {
    int32_t kept_bound;     /* 1: the bound scene followed the count change; 0: it was unbound (or none was bound) */
    int32_t added;          /* synced targets that did not exist at the previous sync */
    int32_t removed;        /* previously synced targets that no longer exist */
    int32_t lists_moved;    /* surviving targets whose index changed and whose lists were moved, not rebuilt */
    int32_t lists_rebuilt;  /* targets whose lists were built on their own (new, re-indexed-but-owned, or moved in space) */
    int32_t lists_full_rebuild;
    uint64_t bytes_uploaded;
} art_target_resize_stats;
ART_API int art_targets_last_resize(art_ctx* ctx, art_target_resize_stats* out);

/* Diagnostics (tests; host only, works on the CPU backend): for each synced index i < cap, the synced
 * index the same target held before the last art_targets_sync, or -1 if it is new.
 * Returns the synced count. */
ART_API int art_debug_target_sync_map(art_ctx* ctx, int32_t* src, int32_t cap);

/* ------------------------------------------- per-source data follows the targets (ABI 3.13) */

/* The follow map: the maps of every committed art_targets_sync since the last art_target_follow_mark,
 * composed. src[i] is the index that the target now at synced index i held in the base list (the
 * synced list at the mark), or -1 if it was not in it. Before the first mark the base list is empty
 * (base_count 0), so every target is new. A caller that keeps arrays per source (the tick's d_state and
 * d_volume, art_dsp_sources_follow_device) or per target moves each of them by this map, then marks;
 * any number of syncs may lie between two marks.
 * Returns the synced count; writes min(cap, count) entries; *base_count (may be NULL) = the base
 * list's length. Host only, no synchronisation, works on the CPU backend. ART_E_INVALID for a NULL
 * context, cap < 0 or a NULL src with cap > 0. */
ART_API int art_target_follow_map(art_ctx* ctx, int32_t* src, int32_t cap, int32_t* base_count);

/* The base list becomes the synced list: follow = identity, base_count = synced count. */
ART_API int art_target_follow_mark(art_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* ART_COLLIDERS_H */
