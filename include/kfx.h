/*
 * kfx.h — C-ABI drop-in boundary of the MI355X-native KinectFusion hot path.
 *
 * The reference exposes the hot path only as the C++ class `kf::kinectfusion`
 * (kfusion/include/kinectfusion.h:31-73) whose methods take OpenCV types.  There
 * is no FFI in the reference; this header is the plain-C seam a binding (ctypes,
 * cgo, JNI, or the header-only C++ adapter in
 * slam-kinectfusion_amd/adapter/kinectfusion.h) calls.  Every entry point below
 * names the reference interface it replaces.
 *
 * Conventions
 *   - All host buffers belong to the caller and are copied; the context owns all
 *     device memory.  No torch / HIP types cross this boundary.
 *   - Images are row-major, tightly packed (no pitch): depth f32 or u16 in
 *     millimetres (depth_sensor.cpp:191 converts PNG u16 mm -> f32 mm), colour
 *     BGR8 interleaved (cv::Mat CV_8UC3), vertex/normal maps float3 AoS.
 *   - Poses are kfx_pose {R row-major 3x3, t}; a cv::Affine3f maps 1:1.
 *   - Every function returns an int status (KFX_OK = 0).  The reference prints
 *     CUDA errors and continues (safe_call.hpp:8-14); here they are returned.
 */
#ifndef KFX_H
#define KFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KFX_ABI_VERSION 2 /* 2: kfx_synchronize/kfx_pipeline report earlier frames; u8 weight uploads */
#define KFX_MAX_LEVELS 4

/* status codes */
#define KFX_OK 0
#define KFX_TRACKING_LOST 1 /* kinectfusion.cpp:97-101: "tracking fail!" -> reset() */
#define KFX_ERR_ARG (-1)
#define KFX_ERR_HIP (-2)
#define KFX_ERR_OOM (-3)
#define KFX_ERR_STATE (-4)
#define KFX_ERR_NO_DEVICE (-5)
#define KFX_ERR_COMM (-6)

#define KFX_COMM_ID_BYTES 128

/* kf::Intrinsics (types.hpp:13-29).  `c` (types.hpp:17) is unused on the path. */
typedef struct kfx_intrinsics {
  int width, height;
  float fx, fy, cx, cy;
} kfx_intrinsics;

/* cv::Affine3f as used on the path: rotation row-major R[3*i+j] = R(i,j). */
typedef struct kfx_pose {
  float R[9];
  float t[3];
} kfx_pose;

/* kf::kinectfuison_params (kinectfusion.h:9-30); defaults kinectfusion.cpp:167-190. */
typedef struct kfx_params {
  int pyramid_height;            /* 3 */
  float dfilter_dist;            /* 5 m depth truncation (image_process.cu:15) */
  int bfilter_kernel_size;       /* 5 */
  float bfilter_spatial_sigma;   /* 10 (pixels) */
  float bfilter_color_sigma;     /* 10 (mm) */
  float icp_dist_threshold;      /* 0.015 m */
  float icp_angle_threshold;     /* 30 degrees; stored as sinf(deg2rad) (icp_registration.cpp:5) */
  int icp_iter_count[KFX_MAX_LEVELS]; /* indexed by level: {4,5,10} */
  float volu_range[3];           /* metres, 3 */
  int volu_dims[3];              /* 512 */
  float volu_trun_dist;          /* 2.1 * range / dims */
  kfx_pose volu_pose;            /* translate(-L/2, -L/2, 0.5) */
  int tsdf_max_weight;           /* 64; the kernel uses MAX_WEIGHT (device_utils.cuh:5) */
  float min_pose_move;           /* unused by the reference path */
} kfx_params;

typedef struct kfx_ctx kfx_ctx;

/* ---- library ------------------------------------------------------------ */
int kfx_abi_version(void);
const char *kfx_last_error(void);
/* kinectfuison_params::default_params (kinectfusion.cpp:167-190). */
int kfx_default_params(kfx_params *out);

/* ---- kf::kinectfusion ---------------------------------------------------- */
/* kinectfusion::kinectfusion(intr, params) (kinectfusion.cpp:9-27).  device =
 * HIP ordinal.  Allocates frames, the TSDF volume and ICP workspaces, then
 * reset()s. */
int kfx_create(const kfx_intrinsics *intr, const kfx_params *params, int device,
               kfx_ctx **out);
/* kinectfusion::release() + ~kinectfusion() (kinectfusion.cpp:28-31,191-195). */
int kfx_destroy(kfx_ctx *ctx);
/* kinectfusion::reset() (kinectfusion.cpp:133-141): frame_count=1, frames and
 * volume zeroed (the reference's partial reset, SURVEY A5, is made total),
 * pose_record = [I]. */
int kfx_reset(kfx_ctx *ctx);

/* kinectfusion::pipeline(cmap, dmap) (kinectfusion.cpp:78-127).  Host images;
 * blocks until the frame is done.  Returns KFX_OK, or KFX_TRACKING_LOST when ICP
 * failed and the reference's reset() semantics were applied (frame dropped). */
int kfx_pipeline(kfx_ctx *ctx, const uint8_t *bgr, const float *depth_mm);
int kfx_pipeline_u16(kfx_ctx *ctx, const uint8_t *bgr, const uint16_t *depth_mm);

/* Device-resident input: frames uploaded once with kfx_stage_frames are
 * processed without PCIe traffic and without a host sync (tracking state lives
 * on the device).  kfx_synchronize waits for queued frames
 * and reports them: KFX_TRACKING_LOST if any frame completed since the last
 * status check (kfx_pipeline, kfx_synchronize) was dropped by a tracking
 * failure (reset() applied, kinectfusion.cpp:97-101), KFX_ERR_HIP if the ICP
 * barrier watchdog fired, else KFX_OK. */
int kfx_stage_frames(kfx_ctx *ctx, int n_frames, const uint8_t *bgr,
                     const float *depth_mm);
int kfx_pipeline_staged(kfx_ctx *ctx, int frame_index);
int kfx_synchronize(kfx_ctx *ctx);
/* Pipelined host input (kinectfusion::pipeline, kinectfusion.cpp:48-52, without
 * the per-frame host sync): the frame is copied into a pinned 4-slot ring and
 * uploaded on a copy stream while earlier frames run, then queued like a
 * staged frame; the call returns without waiting for the GPU (it blocks only
 * when the ring slot's previous upload is still in flight).  The caller's
 * buffers are free on return.  Tracking status: kfx_synchronize. */
int kfx_pipeline_async(kfx_ctx *ctx, const uint8_t *bgr, const float *depth_mm);
int kfx_pipeline_async_u16(kfx_ctx *ctx, const uint8_t *bgr, const uint16_t *depth_mm);
/* Zero-copy host input: page-lock a caller buffer (hipHostRegister).  A frame
 * whose depth and colour both lie in registered buffers is uploaded by
 * kfx_pipeline_async straight from them, with no host copy and no host wait;
 * such a buffer is then read asynchronously and must stay unchanged until
 * kfx_synchronize returns (or kfx_unregister_host_buffer, which waits for
 * pending uploads).  kfx_destroy unregisters what is left. */
int kfx_register_host_buffer(kfx_ctx *ctx, void *ptr, size_t bytes);
int kfx_unregister_host_buffer(kfx_ctx *ctx, void *ptr);
/* Captured hipGraphs for the per-frame launch sequence: 0 eager launches;
 * 1 (default) single-stream frames replay one graph per input, overlapped
 * staged / async frames replay their pyrDown + preprocess as a graph and
 * launch ICP, integrate and raycast eagerly; 2 as 1, and overlapped frames
 * also replay ICP + integrate + raycast as a second graph (measured slower,
 * DESIGN.md §3).  Z-slab contexts capture the same graphs, their RCCL
 * collectives (slab combine, sharded-ICP all-reduces) as graph nodes; if RCCL
 * refuses stream capture those frames launch eagerly instead.  Frames of an
 * in-process group (kfx_pipeline_group) launch eagerly when overlapped.
 * Results are identical in every mode. */
int kfx_set_graph_mode(kfx_ctx *ctx, int enabled);
/* The mode in effect: as set, lowered where a capture was refused (RCCL
 * refusing capture: 2 -> 1 for overlapped frames, 1 -> 0 for single-stream
 * frames of a communicator context). */
int kfx_get_graph_mode(kfx_ctx *ctx, int *mode);
/* Why graph mode 2 was lowered to 1 on this context (the RCCL / capture error
 * text), or "" (valid until the context is destroyed). */
const char *kfx_get_graph_note(kfx_ctx *ctx);
/* Overlap each staged frame's preprocess with the previous frame's tracking on
 * a second stream, over double-buffered frame maps (default on; staged frames
 * then launch eagerly instead of through graphs).  Results are identical. */
int kfx_set_frame_overlap(kfx_ctx *ctx, int enabled);
/* Sampled kernel timing inside a run of pipelined frames: every `every`-th
 * frame (from now, up to max_samples frames) is bracketed by HIP events on
 * the stream its kernels run on (such a frame launches eagerly instead of
 * through its graph); kfx_get_kernel_timing returns the mean ms of ICP,
 * integrate and raycast over the samples taken and starts a new sample set.
 * every = 0 turns sampling off. */
int kfx_set_kernel_timing(kfx_ctx *ctx, int every, int max_samples);
int kfx_get_kernel_timing(kfx_ctx *ctx, float out_ms[3], int *n_samples);
/* The same samples split further: ICP, integrate, local raycast (+ resize on a
 * single volume) and the slab combine (RCCL MIN/MAX all-reduces + expand +
 * resize; 0 on a single volume).  out_ms[2] + out_ms[3] is
 * kfx_get_kernel_timing's raycast figure.  Starts a new sample set too. */
int kfx_get_kernel_timing_ex(kfx_ctx *ctx, float out_ms[4], int *n_samples);
/* Run all ICP iterations of a frame as one persistent launch (default on; used
 * only when its grid fits co-resident on the device, else one launch per
 * iteration).  enabled: 0 = one launch per iteration, 1 = persistent (plain
 * launch), 2 = persistent through a cooperative launch (co-residency
 * guaranteed by the runtime, ~15 us slower per frame).  A context whose grid
 * barrier watchdog fires (the frame reports KFX_ERR_HIP and is dropped with a
 * volume reset) switches to mode 2 by itself.  Returns 1 if the persistent
 * kernel is usable on this context, 0 if not, <0 on error.  Results are
 * identical in every mode. */
int kfx_set_icp_persistent(kfx_ctx *ctx, int enabled);
/* Test hook: the next tracked frame's persistent-ICP barrier never completes
 * (its watchdog fires after 0.2 s). */
int kfx_debug_force_icp_stall(kfx_ctx *ctx);
/* Test hook: on != 0 routes integrate and raycast through the 64-bit-index
 * kernels (the path a volume of >= 2^31 stored voxels takes, A9:
 * device_utils.cuh:31, tsdf_volume.cpp:24) at any volume size, so the oracle
 * can pin them at sizes it runs.  Results are identical either way. */
int kfx_debug_force_index64(kfx_ctx *ctx, int on);
/* Debug hooks of integrate's settled-brick skip (added under
 * ABI version 2, nothing else changed).  kfx_debug_count_settled: on != 0
 * makes every integrate launch count the bricks its waves skip (off by
 * default).  kfx_debug_get_settled: out[0] = bricks whose settled byte is set
 * now, out[1] = bricks skipped by the last integrate launch (0 while the
 * count is off).  Results are identical with the count on or off. */
int kfx_debug_count_settled(kfx_ctx *ctx, int on);
int kfx_debug_get_settled(kfx_ctx *ctx, uint64_t out[2]);
/* Debug count of integrate's hidden-brick skip (added under ABI
 * version 2, nothing else changed), armed by kfx_debug_count_settled: out[0] =
 * bricks the last integrate launch stepped over as hidden behind every surface
 * they project onto, out[1] = those among them that hang over an end of their
 * tile's interval (both 0 while the count is off). */
int kfx_debug_get_hidden(kfx_ctx *ctx, uint64_t out[2]);
/* Debug switch of integrate's per-frame tile kernel (added
 * under ABI version 2, nothing else changed).  On (the default where the
 * context keeps a tile table: a whole volume, not 1024..2047 slices deep, with
 * more than one z-chunk per column tile) a small kernel in front of the
 * integrate launch prepares what the integrate waves need once per tile; on == 0 makes every
 * wave compute it for itself again, as contexts without a table always do.
 * Captured graphs are dropped on a change.  Returns 1 if the tile kernel is in
 * use after the call, 0 if not, <0 on error.  Results are identical either
 * way. */
int kfx_debug_int_tiles(kfx_ctx *ctx, int on);
/* Debug hooks of the ICP reduction (added under ABI version 2,
 * nothing else changed).  kfx_debug_get_icp_sums: the 27 int64 fixed-point
 * sums (kfx_stage_icp_accumulate's layout) of the last ICP iteration that ran
 * on this context, whichever kernel ran it; waits for the stream, changes
 * nothing.  kfx_debug_cap_icp_blocks: cap > 0 plans the persistent ICP as if
 * at most `cap` blocks were co-resident on the device (a grid below the real
 * limit is co-resident all the more), cap = 0 restores the device's own
 * figure; captured graphs are dropped.  cap < 0 changes nothing and only
 * reports.  Returns 1 if the persistent kernel is
 * usable under the cap, 0 if not (one launch per iteration then), <0 on
 * error.  plan (may be NULL) receives the plan in effect: [0] 1 if the
 * strided kernel form was chosen, [1] blocks of the grid, [2] levels, [3] the
 * persistent launch in use (0 none, 1 plain, 2 cooperative), then per level l
 * [4+3l] the contiguous pixel span per block (0: whole pixel groups; in the
 * strided form groups b, b + blocks, ...), [5+3l] pixel groups (or spans),
 * [6+3l] pixels per lane.  Results are identical under any cap. */
#define KFX_ICP_PLAN_WORDS 16
int kfx_debug_get_icp_sums(kfx_ctx *ctx, int64_t out[27]);
int kfx_debug_cap_icp_blocks(kfx_ctx *ctx, int cap, int32_t plan[KFX_ICP_PLAN_WORDS]);
/* Debug hook of the ICP step (added under ABI version 2, nothing
 * else changed): the six doubles (rotation vector, translation) of the last
 * ICP iteration that solved on this context, whichever kernel ran it; waits
 * for the stream, changes nothing.  Defined after a track that returned
 * KFX_OK and ran at least one iteration.
 * With it, off the frame path: kfx_stage_icp on a slab context of world 1 with
 * kfx_set_icp_allreduce on and no communicator runs the sharded loop (the
 * per-iteration sums of rank 0 of 1, then the stand-alone solve kernel, no
 * collective), and kfx_debug_cap_icp_blocks reports 3 in plan[3] for such a
 * context.  Every other context behaves as before. */
int kfx_debug_get_icp_step(kfx_ctx *ctx, double x[6]);
/* Debug hooks of the extraction (added under ABI version 2,
 * nothing else changed).  The extraction sweeps (count, emit and pool pass of
 * kfx_extract_points / kfx_extract_mesh and their _attr forms) give every wave
 * K consecutive units (column tile x 8-slice chunk) of one chunk; K is 1 below
 * 131072 units and grows to 64 with the volume.  kfx_debug_extract_units:
 * units in {1, 2, 4, 8, 16, 32, 64} forces that K in every sweep of this
 * context, so a small volume takes the paths of a large one; 0 restores the
 * automatic rule; anything else returns KFX_ERR_ARG and changes nothing.
 * Returns the K the next extraction of this context's whole (or slab's) volume
 * uses.  Results are identical for every K.
 * kfx_debug_scan: the exclusive scan the extraction and the eviction turn
 * their per-unit counts into offsets with, on its own: uploads counts[n], runs
 * the scan on the context's stream with the extraction's workspaces and
 * downloads offsets[n] (offsets[i] = counts[0] + ... + counts[i-1], 64-bit)
 * and *total (the sum of all counts).  KFX_ERR_ARG on a null pointer, n < 1 or
 * n > 2^28. */
int kfx_debug_extract_units(kfx_ctx *ctx, int units);
int kfx_debug_scan(kfx_ctx *ctx, const uint32_t *counts, int64_t n, uint64_t *offsets, uint64_t *total);
/* Measurement hook (tools/slab_record.py): device time of the sharded ICP's
 * per-rank launches for band `rank` of `world` (kfx_set_icp_allreduce's
 * k_icp_acc over the band's rows of every level + the k_icp_solve, 19
 * iterations at the default parameters) on the current frame maps, without
 * the all-reduces, which the caller prices separately; *ms = the mean of
 * `reps` runs.  The tracking state is saved before and restored after, so the
 * context's frames are unaffected. */
int kfx_debug_icp_band_ms(kfx_ctx *ctx, int rank, int world, int reps, float *ms);
/* Slab contexts (SURVEY.md §8e alternative): instead of every rank running
 * the whole ICP (default), rank r accumulates the 27 products over its band
 * of each level's rows and the exact int64 partials are all-reduced (SUM)
 * per iteration (19 collectives per frame), then every rank solves the same
 * system — poses identical to the replicated mode. */
int kfx_set_icp_allreduce(kfx_ctx *ctx, int enabled);
/* Profiling seam (trace builds, -DKFX_ICP_TRACE via tools/variants.sh; the
 * product library returns 0: the stamps' code costs ICP ~3 us per frame):
 * per ICP iteration of the last persistent-ICP frame, five s_memrealtime
 * stamps (100 MHz): block 0 start, block 0 arrived, block 0 released from the
 * barrier, block 0 solved, last block arrived.  Returns the number of
 * iterations written (<= max_iters). */
int kfx_get_icp_trace(kfx_ctx *ctx, uint64_t *out, int max_iters);

/* kinectfusion::getCurCameraPose() (kinectfusion.cpp:128-132). */
int kfx_get_cur_camera_pose(kfx_ctx *ctx, kfx_pose *out);
/* kinectfusion::frame_count (kinectfusion.h:58). */
int kfx_get_frame_count(kfx_ctx *ctx, int *out);
/* kinectfusion::pose_record (kinectfusion.h:59).  Writes min(cap, n) poses. */
int kfx_get_pose_record(kfx_ctx *ctx, kfx_pose *out, int cap, int *n);
/* main.cpp:95-98: pose_record as `Matx44f operator<<` text ("%.8g"). */
int kfx_write_poses_txt(kfx_ctx *ctx, const char *path);

/* ---- frame / volume access (Frame, TSDFVolume::Data) --------------------- */
#define KFX_FRAME_CUR 0  /* cframe: measured maps of the current frame */
#define KFX_FRAME_PREV 1 /* pframe: raycast (model) maps used as ICP target */
/* Download one pyramid level of a frame.  Any pointer may be NULL.  dmap is
 * metres (after bilateral + truncation), vmap/nmap float3 AoS. */
int kfx_get_frame_maps(kfx_ctx *ctx, int which, int level, float *dmap,
                       float *vmap, float *nmap);
/* Upload maps (test seam for ICP / resize). */
int kfx_set_frame_maps(kfx_ctx *ctx, int which, int level, const float *vmap,
                       const float *nmap);
/* TSDFVolume::Data() (tsdf_volume.cpp:4): export the volume as the
 * reference's 8-byte x-fastest records {int16 tsdf, int16 weight, u8 c0,c1,c2,
 * u8 pad=0} (device_types.hpp:51-56).  dst holds X*Y*Z*8 bytes. */
int kfx_download_tsdf(kfx_ctx *ctx, void *dst_records);
/* Import records in the same format (test seam; no reference counterpart).
 * Weights are stored as u8 on the device (the reference's never exceed
 * MAX_WEIGHT = 64): a record weight outside 0..255 fails with KFX_ERR_ARG. */
int kfx_upload_tsdf(kfx_ctx *ctx, const void *src_records);
/* SoA export: tsdf int16[N], weight int16[N], colour u8x4[N] (any may be NULL). */
int kfx_download_volume_soa(kfx_ctx *ctx, int16_t *tsdf, int16_t *weight,
                            uint8_t *rgba);

/* ---- stage entry points (kf::device seam, device_types.hpp:113-128) ------ */
/* imageProcess (kinectfusion.cpp:48-76): upload, pyrDown, bilateral,
 * depthTruncation, getVertexmap, getNormalmap into the CUR frame. */
int kfx_stage_preprocess(kfx_ctx *ctx, const uint8_t *bgr, const float *depth_mm);
/* rigidICP (rigid_icp.cu:135-169) one iteration at `level`: CUR vs PREV maps
 * under `pose`; returns the 27 sums (i<=j upper triangle with b, in the
 * reference's shift order) as int64 fixed point (value * 2^32). */
int kfx_stage_icp_accumulate(kfx_ctx *ctx, int level, const kfx_pose *pose,
                             int64_t sums[27]);
/* ICPRegistration::rigidTransform (icp_registration.cpp:16-46) on CUR vs PREV
 * maps: the whole coarse-to-fine loop.  Returns KFX_OK or KFX_TRACKING_LOST. */
int kfx_stage_icp(kfx_ctx *ctx, kfx_pose *cam_pose_out);
/* device::integrate (tsdf_volume.cu:103-111) of the CUR frame level-0 depth and
 * colour with vol2cam; optional counts of updated / colour-updated voxels. */
int kfx_stage_integrate(kfx_ctx *ctx, const kfx_pose *vol2cam,
                        int64_t *n_updated, int64_t *n_colored);
/* device::raycast (tsdf_volume.cu:264-273) into PREV level 0, with cam2vol and
 * Rinv (row-major 3x3), then resizePointsNormals for levels >= 1.  A slab
 * context of world 1 runs the slab kernel and expands its payload into the
 * same maps; one slab of several is refused (KFX_ERR_STATE). */
int kfx_stage_raycast(kfx_ctx *ctx, const kfx_pose *cam2vol, const float Rinv[9]);

/* ---- timing -------------------------------------------------------------- */
/* Per-stage device milliseconds of the last kfx_pipeline* call run in
 * profiled mode (graph off): {preprocess, icp, integrate, raycast, total}. */
int kfx_set_profiling(kfx_ctx *ctx, int enabled);
int kfx_get_stage_ms(kfx_ctx *ctx, float out_ms[5]);
/* Voxel counts of the last processed frame's integrate (the algorithmic-byte
 * inputs of the roofline): voxels whose tsdf/weight were
 * updated and those whose colour was also blended.  Count-only kernel, the
 * volume is not touched. */
int kfx_integrate_counts(kfx_ctx *ctx, int64_t *n_updated, int64_t *n_colored);
/* Work statistics of the same count-only pass: out = {updated, coloured,
 * visited (voxels evaluated inside the per-column candidate z intervals),
 * gathered (visited voxels that project into the image and read a depth),
 * wave batches executed (4 voxels per lane each), 0, 0, 0} (slots 5-7 are
 * reserved; they held the dropped free-space certification's counts). */
int kfx_integrate_stats(kfx_ctx *ctx, int64_t out[8]);
/* Work statistics of the last processed frame's raycast (re-run on the same
 * state, nothing written): out = {rays marched, empty-space skip lookups,
 * samples skipped by them, lookups that found an occupied brick, 14-sample
 * batches marched (per ray), hit candidates whose normal was computed,
 * N_uniq = distinct voxels the reference raycast (tsdf_volume.cu:210-260, no
 * skipping) reads — nearest samples plus the trilinear corners of the normals
 * (0 for slab contexts), and the number of those reads}. */
int kfx_raycast_stats(kfx_ctx *ctx, int64_t out[8]);
/* Voxel records of n selected (x, y) columns over this context's owned slices
 * [own0, own1) (test seam for volumes too large to download whole): cols =
 * n int32 (x, y) pairs; each output holds n * (own1 - own0) entries, column
 * after column, z ascending (rgb: u8 c0, c1, c2, 0 per voxel).  Any output
 * may be null. */
/* Host side of the Z-slab raycast combine (the same code the
 * device combine runs, exposed for multi-process tests without a GPU): after
 * the all-reduce MIN of the keys, clear the payload {Ts, nout} planes (4 x n
 * u32) of the pixels this slab lost; after the all-reduce MAX of the payload
 * bits, rebuild the level-0 vmap/nmap (n float3 each) of a tracked frame at
 * cam2vol / Rinv (tsdf_volume.cu:246-255). */
int kfx_slab_mask_payload(const uint32_t *key_local, const uint32_t *key_min, uint32_t *payload, int64_t n);
int kfx_slab_expand(const uint32_t *payload, const kfx_intrinsics *intr, const kfx_pose *cam2vol,
                    const float Rinv[9], float *vmap, float *nmap);
int kfx_download_columns(kfx_ctx *ctx, const int32_t *cols, int n, int16_t *tsdf, int16_t *weight,
                         uint32_t *rgb);

/* ---- point cloud ------------------------------------------ */
/* Device ms of the last kfx_extract_points / kfx_extract_mesh call, three
 * phases.  A call with a buffer (cap > 0) normally reads the volume ONCE:
 * [0] the pass that counts every wave's items and writes them into an
 * unordered pool, [1] the offset scan, [2] the pool-to-canonical-order copy
 * (kfx_get_extract_passes = 1).  The two-pass path (count only, cap = 0;
 * kfx_set_extract_passes(2); or more items than cap, when the pool cannot hold
 * them all): [0] the count pass, [1] the scan, [2] the emit pass, which reads
 * the volume again (passes = 2; 0 if nothing was emitted). */
int kfx_get_extract_ms(kfx_ctx *ctx, float out_ms[3]);
/* Volume passes of the last extraction: 1 or 2 (see above). */
int kfx_get_extract_passes(kfx_ctx *ctx, int *passes);
/* 1 (default): kfx_extract_points / kfx_extract_mesh with a buffer read the
 * volume once; 2: always the count pass, the offset scan and the emit pass.
 * The output is identical. */
int kfx_set_extract_passes(kfx_ctx *ctx, int passes);
/* TSDFVolume::fetchPointCloud buffer size (tsdf_volume.cpp:67) */
#define KFX_DEFAULT_CLOUD_POINTS 10000000
/* kinectfusion::getRenderMap (kinectfusion.cpp:33-47; kernel_renderPhong /
 * kernel_renderNormals, image_process.cu:137-221): the previous frame's
 * level-0 raycast maps shaded on the device, lit from the last pose's camera
 * position; out = width*height uchar3, pixels without a surface 0. */
#define KFX_RENDER_PHONG 0
#define KFX_RENDER_NORMAL 1
int kfx_render(kfx_ctx *ctx, int type, uint8_t *out);

/* Free-viewpoint render. */
#define KFX_VIEW_PHONG 0   /* kfx_render's Phong, lit from the view camera's position */
#define KFX_VIEW_NORMAL 1  /* kfx_render's normal colours */
#define KFX_VIEW_COLOR 2   /* the fused colour, unshaded (below) */
/* Render the volume as it stands from camera-to-world pose `cam_pose` (the pose
 * record's convention) through `view` (any size, any fx fy cx cy).  out =
 * width*height uchar3, pixels without a surface 0.  vmap / nmap (float3 AoS) and
 * ts (float, metres along the ray, 0 = no hit) may each be NULL.
 * The maps are the reference raycast's (tsdf_volume.cu:210-260) at `view` from
 * cam2vol = volu_pose^-1 * cam_pose, level 0 only.  KFX_VIEW_COLOR blends the
 * colours of the hit's 8 trilinear corners that lie in the volume and were ever
 * coloured, with 8-bit fixed-point weights in integer arithmetic, in the input
 * images' B, G, R order; a hit without such a corner keeps its Phong value.
 * The call runs on the context's stream behind every queued frame and blocks
 * until the image is on the host.  It writes nothing the tracker reads and
 * leaves a pending tracking status to the next kfx_synchronize.
 * KFX_ERR_ARG: a null view, cam_pose or out; a type outside 0..2; width or
 * height below 1 or width*height above 2^26; a non-finite or zero fx or fy; a
 * non-finite cx, cy or pose entry.  KFX_ERR_STATE: a slab context of a world
 * larger than 1. */
int kfx_render_view(kfx_ctx *ctx, const kfx_intrinsics *view, const kfx_pose *cam_pose,
                    int type, uint8_t *out, float *vmap, float *nmap, float *ts);
int kfx_get_view_ms(kfx_ctx *ctx, float *ms);   /* device ms of the last view (HIP events) */
int kfx_write_ppm(const char *path, const uint8_t *bgr, int width, int height); /* binary P6, RGB */

/* Order-free checksum of the (owned part of the) volume: out[0] = sum mod
 * 2^64 of a 64-bit mix of (x-fastest global voxel index, tsdf, weight,
 * colour) over every voxel, out[1] = voxels with weight > 0.  The sums of a
 * volume's Z-slabs equal the single volume's: a full-size property check
 * without downloading the volume. */
int kfx_volume_checksum(kfx_ctx *ctx, uint64_t out[2]);

/* kinectfusion::extracePointcloud (kinectfusion.cpp:142-147) ->
 * TSDFVolume::fetchPointCloud (tsdf_volume.cpp:63-84) -> device::extract_points
 * (FullScan6, tsdf_volume.cu:307-499): zero crossings of the volume along +x,
 * +y, +z, in volume-pose (world) coordinates.  Writes min(cap, total) points
 * (float3) to xyz (NULL with cap 0: count only) and the total to *n_points.
 * The reference's order is nondeterministic (atomics); here it is canonical
 * (slice chunk, 8x8 tile, z, lane, edge), so the first `cap` points
 * are deterministic.  A slab context extracts its owned slices; concatenating
 * slabs in rank order gives the single-volume cloud. */
int kfx_extract_points(kfx_ctx *ctx, float *xyz, int64_t cap, int64_t *n_points);
/* kinectfusion::savePointcloud (kinectfusion.cpp:148-166): ASCII PLY, x y z per
 * line with ostream's default 6 significant digits. */
int kfx_write_ply(const char *path, const float *xyz, int64_t n);
/* extract (cap <= 0: KFX_DEFAULT_CLOUD_POINTS) + kfx_write_ply */
int kfx_save_pointcloud(kfx_ctx *ctx, const char *path, int64_t cap);

/* Marching-cubes mesh of the zero level set (C5 asks for a mesh;
 * the reference has no counterpart).  A cube is 8 neighbouring voxels, all
 * with weight > 0; corners with tsdf < 0 are inside; the triangle table is
 * derived at run time (each face cuts off every run of inside corners, so
 * ambiguous faces resolve the same way from both sides: a crack-free mesh).
 * Edge vertices interpolate voxel centres as the point cloud does, in world
 * coordinates.  Triangles are 9 floats (3 vertices), in the point cloud's
 * canonical order; writes min(cap, total), *n_tris = total.  A slab meshes
 * its owned cubes: slab meshes concatenate to the single volume's. */
int kfx_extract_mesh(kfx_ctx *ctx, float *tri_xyz, int64_t cap_tris, int64_t *n_tris);
/* ASCII PLY of a triangle soup: 3n vertices (%g), n faces "3 i j k". */
int kfx_write_ply_mesh(const char *path, const float *tri_xyz, int64_t n_tris);

/* Attributed extraction (an extension: the reference fuses colour into the
 * volume, tsdf_volume.cu:82-95, and never reads it back).  Item i of an _attr
 * call is item i of the plain call (same canonical order, total, cap prefix
 * and slab concatenation; x, y, z are the plain call's bits), with a unit
 * normal and the fused colour.  A vertex lies on the grid edge from voxel a to
 * b = a + e_axis.
 *   colour (integers): ta = |tsdf_a|, tb = |tsdf_b| (raw int16), ca, cb the
 *     24-bit packed colours, 0 = never coloured.  Both coloured: channel j =
 *     (ca_j*tb + cb_j*ta + ((ta+tb)>>1)) / (ta+tb), a = 255; one coloured: that
 *     colour, a = 255; none: 0,0,0 and a = 0.  b, g, r = the volume's c0, c1,
 *     c2 (the BGR order of the input images).
 *   normal (float32, no contraction): g_k(q) = (hi - lo) / voxel_size[k] with
 *     hi / lo = F at q +/- e_k where that voxel lies in the volume and has
 *     weight != 0, else F(q), and the difference doubled when exactly one of
 *     the two is valid; m = g(a)*|F_b| + g(b)*|F_a|; n = normalize(R_volume m)
 *     (0,0,0 when the length is 0).  The TSDF is positive in front of the
 *     surface: normals point out of it.
 * cap = 0 (or a null buffer with cap 0) counts only; kfx_set_extract_passes,
 * kfx_get_extract_passes and kfx_get_extract_ms apply as to the plain calls. */
typedef struct kfx_vertex {
  float x, y, z;
  float nx, ny, nz;
  uint8_t b, g, r, a;
} kfx_vertex; /* 28 bytes */
int kfx_extract_points_attr(kfx_ctx *ctx, kfx_vertex *out, int64_t cap, int64_t *n_points);
/* 3 kfx_vertex per triangle */
int kfx_extract_mesh_attr(kfx_ctx *ctx, kfx_vertex *out, int64_t cap_tris, int64_t *n_tris);
/* ASCII PLY: "property float x y z nx ny nz", "property uchar red green blue";
 * lines "%g %g %g %g %g %g %d %d %d" (red = r).  The mesh file adds the face
 * element of kfx_write_ply_mesh (faces "3 3i 3i+1 3i+2"). */
int kfx_write_ply_attr(const char *path, const kfx_vertex *v, int64_t n);
int kfx_write_ply_mesh_attr(const char *path, const kfx_vertex *v, int64_t n_tris);
/* extract (cap <= 0: KFX_DEFAULT_CLOUD_POINTS items) + write */
int kfx_save_pointcloud_attr(kfx_ctx *ctx, const char *path, int64_t cap);
int kfx_save_mesh_attr(kfx_ctx *ctx, const char *path, int64_t cap_tris);

/* ---- moving volume ----------------------------------------
 * Added under ABI version 2, nothing else changed.  The TSDF window follows
 * the camera: kfx_shift_volume moves the contents by whole bricks inside
 * device memory and moves the volume pose the other way, so the model stays
 * where it is in the world; kfx_evict_points hands out the surface the shift
 * is about to drop.  A context that never shifts behaves as before.
 *
 * kfx_shift_volume: shift = (sx, sy, sz) voxels along the volume's own axes,
 * each a multiple of 8.  Afterwards voxel (x, y, z) holds what voxel (x + sx,
 * y + sy, z + sz) held, where that index lies inside the volume; every other
 * voxel is empty as after a reset (tsdf 0, weight 0, colour 0).  A component
 * with |s| >= its dimension empties the volume.  The voxel origin becomes
 * o' = o + s and the volume pose R' = R0, t' = t0 + R0 (o' * voxel_size),
 * R0, t0 the pose the context was created with (recomputed from t0 each time:
 * rounding does not accumulate), in float32 without contraction, in this
 * order: d_k = (float)o'_k * vs_k (vs_k = volu_range[k] / (float)volu_dims[k]);
 * row sum (R[3i]*d0 + R[3i+1]*d1) + R[3i+2]*d2; t'_i = t0_i + sum.  Every later
 * call uses the new pose (frames, kfx_render_view, the extractors,
 * kfx_slice_work*).  The call runs on the context's stream behind every queued
 * frame (staged and overlapped ones included) and in front of every later one;
 * captured graphs are dropped and recaptured.  The skip maps of raycast and
 * integrate are rebuilt from the new contents, as after kfx_upload_tsdf.  The
 * previous-frame maps, the pose record (world coordinates), the frame count
 * and a pending tracking status are untouched.  A zero shift does nothing.
 * KFX_ERR_ARG: a null shift or a component that is no multiple of 8 (volume,
 * origin and pose untouched).  KFX_ERR_STATE: a slab context of a world larger
 * than 1 (a z shift across slabs would need an exchange: out of scope).
 * kfx_reset also returns the origin to (0, 0, 0) and the pose to (R0, t0).  A
 * tracking-loss reset happens on the device and cannot: on KFX_TRACKING_LOST
 * call kfx_reset before going on with a context that has shifted.
 *
 * kfx_evict_points: the items of kfx_extract_points_attr whose grid edge a -> b
 * has a or b outside the box the shift would keep (voxel v is kept iff
 * 0 <= v_k - s_k < dims_k for every k), in the same canonical order and with
 * the same 28 bytes (gradient and colour computed on the whole volume as it
 * stands).  Evicted items and the items of the kept box partition the full
 * extraction.  The volume is not changed.  Writes min(cap, total) items, *n =
 * total, cap = 0 counts only; a zero shift gives 0 items.  Same argument
 * checks as kfx_shift_volume; blocks until the items are on the host.
 *
 * kfx_shift_for_pose (host only, no context): the shift that centres the
 * volume on the point ahead_m metres along the camera's +z: c = cam_pose (0, 0,
 * ahead_m), q = volume_pose^-1 c, shift_k = 8 lround(((q_k - range_k/2) / vs_k)
 * / 8), in double.  KFX_ERR_ARG: a null pointer, a non-finite pose entry, a
 * non-finite or negative ahead_m. */
int kfx_shift_volume(kfx_ctx *ctx, const int shift[3]);
int kfx_evict_points(kfx_ctx *ctx, const int shift[3], kfx_vertex *out, int64_t cap, int64_t *n);
int kfx_get_volume_origin(kfx_ctx *ctx, int origin[3]);   /* accumulated shift, voxels */
int kfx_get_volume_pose(kfx_ctx *ctx, kfx_pose *out);     /* the volume pose in effect */
int kfx_get_shift_ms(kfx_ctx *ctx, float out_ms[2]);      /* device ms of the last evict, last shift (HIP events) */
int kfx_shift_for_pose(const kfx_params *p, const kfx_pose *volume_pose, const kfx_pose *cam_pose,
                       float ahead_m, int shift[3]);      /* host only, no context */

/* ---- moving volume: bricks out and back in -----------------
 * Added under ABI version 2, nothing else changed.  kfx_shift_volume is lossy:
 * what leaves the window survives only as kfx_evict_points' surface points.
 * These calls hand out the TSDF itself, brick by brick, and take it back when
 * the window returns.
 *
 * A brick is 8 x 8 x 8 voxels: one 8x8 column tile x 8 slices, c = its index in
 * the window per axis.  b is its world coordinate, b_k = origin_k / 8 + c_k
 * (origin = kfx_get_volume_origin, a multiple of 8), which no shift changes.
 *
 * kfx_evict_bricks: the bricks kfx_shift_volume(shift) would drop (those with a
 * voxel that is not kept) and that are not empty, ascending (b[2], b[1], b[0]).
 * A brick is empty when all its stored bytes are 0: tsdf, weight and colour, as
 * in a reset's voxels.  Writes min(cap, total) bricks, *n = total; cap = 0
 * counts only.  Slices of a short last group (Z no multiple of 8) past Z are 0
 * in the record.  The volume is unchanged; a zero shift gives 0 bricks; a
 * component with |s| >= its dimension drops every brick.  Argument checks,
 * stream ordering and blocking as kfx_evict_points (KFX_ERR_STATE on a slab of
 * a world larger than 1).
 *
 * kfx_restore_bricks: every input brick whose world coordinate lies in the
 * current window is written whole over the brick at c = b - origin / 8 (slices
 * past Z are ignored); the others are skipped.  *n_restored (may be NULL) = the
 * number written.  KFX_ERR_ARG, nothing written: a null `in` with n > 0, n < 0,
 * a reserved field that is not 0, two input bricks with the same coordinate
 * inside the window.  KFX_ERR_STATE as above.  The call runs on the context's
 * stream behind every queued frame (staged and overlapped ones included) and in
 * front of every later one, as kfx_shift_volume.  Pose, origin, previous-frame
 * maps, pose record, frame count and a pending tracking status are untouched;
 * captured graphs are kept (they hold neither contents nor maps).  Afterwards
 * the context behaves as after kfx_upload_tsdf of the resulting records: the
 * occupancy maps gain the marks of every restored brick's negative slices
 * (they are supersets: bits of an overwritten brick may stay), every settled
 * byte is cleared and integrate's gate is opened.  n = 0, or no brick in the
 * window, does no device work and leaves the settled bytes alone.
 *
 * kfx_get_stream_ms: device ms of the last kfx_evict_bricks (count + scan +
 * emit, without the copy to the host) and the last kfx_restore_bricks (memsets
 * + launch, without the upload), from HIP events. */
typedef struct kfx_brick {
  int32_t b[3];        /* world brick coordinate: b_k = origin_k / 8 + c_k (c = brick index in the window) */
  int32_t reserved;    /* 0 */
  int16_t tsdf[512];   /* index 64*dz + 8*dy + dx: the device order of a brick */
  uint8_t weight[512];
  uint8_t rgb[512][4]; /* c0, c1, c2, 0 */
} kfx_brick;           /* 3600 bytes */
#ifdef __cplusplus
static_assert(sizeof(kfx_brick) == 3600, "kfx_brick is 3600 bytes");
#else
_Static_assert(sizeof(kfx_brick) == 3600, "kfx_brick is 3600 bytes");
#endif
int kfx_evict_bricks(kfx_ctx *ctx, const int shift[3], kfx_brick *out, int64_t cap, int64_t *n);
int kfx_restore_bricks(kfx_ctx *ctx, const kfx_brick *in, int64_t n, int64_t *n_restored);
int kfx_get_stream_ms(kfx_ctx *ctx, float out_ms[2]);     /* device ms of the last evict_bricks, last restore_bricks */

/* Host-only brick store (no context, no GPU): where a caller keeps what is
 * outside the window, keyed by world brick coordinate.
 * kfx_brick_store_put: copies n bricks in; a coordinate already held is
 * replaced (the later of two equal coordinates in one call wins).  KFX_ERR_ARG:
 * a null store, n < 0, a null `in` with n > 0.
 * kfx_brick_store_take_window: removes and returns the bricks with
 * origin_k / 8 <= b_k < origin_k / 8 + ceil(dims_k / 8), ascending (b[2], b[1],
 * b[0]); *n = how many there are; if cap < *n nothing is removed or written
 * (size the buffer and call again).  KFX_ERR_ARG: a null store, origin, dims or
 * n, an origin component that is no multiple of 8, a dims component below 1,
 * cap < 0, a null `out` with cap > 0. */
typedef struct kfx_brick_store kfx_brick_store;
int kfx_brick_store_create(kfx_brick_store **out);
int kfx_brick_store_destroy(kfx_brick_store *s);
int kfx_brick_store_put(kfx_brick_store *s, const kfx_brick *in, int64_t n);
int kfx_brick_store_count(const kfx_brick_store *s, int64_t *n);
int kfx_brick_store_take_window(kfx_brick_store *s, const int origin[3], const int dims[3],
                                kfx_brick *out, int64_t cap, int64_t *n);

/* ---- world map: points and mesh from evicted and window bricks
 * Added under ABI version 2, nothing else changed.  The extractors above see
 * the window only; these take the surface from any set of bricks, the window's
 * merged with what the moving volume streamed out.
 *
 * A world is a list of n kfx_brick records, strictly ascending in (b[2], b[1],
 * b[0]) (the order of kfx_evict_bricks, kfx_brick_store_take_window,
 * kfx_brick_store_copy and kfx_world_bricks).  World voxel w = 8 b + d holds
 * the record's values; a voxel of a brick that is not in the list is
 * unobserved (tsdf 0, weight 0, colour 0).  There are no volume faces: a
 * neighbour is valid iff its weight != 0.
 *
 * kfx_world_points_attr / kfx_world_mesh_attr: the items of
 * kfx_extract_points_attr / kfx_extract_mesh_attr as defined above, with three
 * changes.  (1) Every voxel of every listed brick is visited, the +x / +y / +z
 * edges and cubes of a brick's last row, column and slice included; one that
 * reaches into an absent brick yields nothing (weight 0).  (2) Position: V_k =
 * ((float)w_k + 0.5f) * vs_k, vs_k = volu_range[k] / (float)volu_dims[k] of the
 * context, interpolated along the edge as in the window extractors, then p =
 * R0 V + t0 with the pose the context was created with (the one
 * kfx_shift_volume recomputes from), float32 without contraction: a voxel's
 * position does not depend on where the window stood when it left, and equals
 * the window extractors' bit for bit while the origin is (0, 0, 0).  (3) Order:
 * brick (list order), then dz, then lane = 8 dy + dx, then edge axis (points)
 * or triangle (mesh); for a box of bricks this is the dense canonical order.
 * Normal and colour as above with R0 as R_volume.
 * Writes min(cap, total) items, *n = total; cap = 0 counts only; n = 0 gives 0
 * items and does no device work.  KFX_ERR_ARG, nothing written: a null list
 * with n > 0, n < 0, a reserved field that is not 0, a list that does not
 * ascend strictly (duplicates included), a coordinate with |b_k| >= 2^20 (below
 * that (float)w_k is exact).  KFX_ERR_STATE on a slab of a world larger than 1.
 * KFX_ERR_OOM when a device buffer cannot be allocated.  The calls run on the
 * context's stream behind every queued frame and block until the items are on
 * the host; they read only the list (never the volume), write nothing the
 * tracker reads, and keep captured graphs and a pending tracking status.  The
 * device buffers grow on demand, are kept, and are freed in kfx_destroy.
 *
 * kfx_get_world_ms: device ms of the last of the two calls: neighbour table,
 * count + scan, emit (HIP events; neither the upload of the records nor the
 * download of the items).
 *
 * kfx_brick_store_copy: all bricks of the store, ascending, nothing removed;
 * *n = how many; cap < *n writes nothing.  KFX_ERR_ARG as kfx_brick_store_take_window.
 *
 * kfx_world_bricks: the window's non-empty bricks (those kfx_evict_bricks
 * returns for a shift that drops everything) merged with the store's (NULL: no
 * store), ascending; the window's brick wins on an equal coordinate.  *n = how
 * many; cap < *n writes nothing.  Store and volume are unchanged (the last
 * kfx_evict_bricks time of kfx_get_stream_ms is this call's).
 *
 * kfx_save_world_mesh: kfx_world_bricks, kfx_world_mesh_attr (cap_tris <= 0:
 * KFX_DEFAULT_CLOUD_POINTS triangles), kfx_write_ply_mesh_attr. */
int kfx_world_points_attr(kfx_ctx *ctx, const kfx_brick *bricks, int64_t n, kfx_vertex *out, int64_t cap,
                          int64_t *n_points);
int kfx_world_mesh_attr(kfx_ctx *ctx, const kfx_brick *bricks, int64_t n, kfx_vertex *out, int64_t cap_tris,
                        int64_t *n_tris);
int kfx_get_world_ms(kfx_ctx *ctx, float out_ms[3]);
int kfx_brick_store_copy(const kfx_brick_store *s, kfx_brick *out, int64_t cap, int64_t *n);
int kfx_world_bricks(kfx_ctx *ctx, const kfx_brick_store *store, kfx_brick *out, int64_t cap, int64_t *n);
int kfx_save_world_mesh(kfx_ctx *ctx, const kfx_brick_store *store, const char *path, int64_t cap_tris);

/* ---- indexed mesh: shared vertices and a face list ----------
 * Added under ABI version 2, nothing else changed.  kfx_extract_mesh_attr and
 * kfx_world_mesh_attr hand out three kfx_vertex per triangle; these hand out
 * each surface vertex once and the triangles as indices into that list.
 *
 * A mesh vertex is the grid edge it lies on: the edge from voxel a to b = a +
 * e_axis, owned by a.  Two triangle corners are the same vertex iff they lie on
 * the same edge; vertices are never welded by position (where tsdf_b == 0,
 * several edges give the same 28 bytes and stay distinct).  An edge is used iff
 * (F_a < 0) != (F_b < 0) and at least one of the up to four cubes around it is
 * complete (all 8 weights > 0, inside the volume).
 *   verts: one kfx_vertex per used edge, the 28 bytes kfx_extract_mesh_attr
 *     (the world form: kfx_world_mesh_attr) writes for that edge, ordered by the
 *     owner's canonical position (z / 8, tile, z & 7, lane = 8 (y & 7) + (x & 7),
 *     axis; in a world: brick in list order, dz, lane, axis).
 *   tris: kfx_extract_mesh_attr's triangles in its order, three uint32_t
 *     indices into verts each, corner order kept.
 * So verts[tris] equals the soup call's output byte for byte, and no edge
 * appears twice in verts.
 *
 * *n_verts and *n_tris are always the totals.  Both buffers are written in
 * full iff both pointers are non-null, cap_verts >= *n_verts and cap_tris >=
 * *n_tris; otherwise nothing is written and the call returns KFX_OK (size the
 * buffers and call again, as kfx_brick_store_take_window: a prefix of a face
 * list is of no use).  Null buffers with caps 0 count only.
 * KFX_ERR_ARG: a null n_verts or n_tris, a negative cap, a null buffer with a
 * positive cap; the world form also kfx_world_mesh_attr's list checks.
 * KFX_ERR_STATE: a slab of a world larger than 1 (a seam's vertices would need
 * renumbering across ranks), more than 2^32 - 1 vertices.  KFX_ERR_OOM as
 * above.  Stream behaviour is that of the calls they stand beside: on the
 * context's stream behind every queued frame, blocking until the data is on
 * the host, writing nothing the tracker reads, keeping captured graphs and a
 * pending tracking status; the world form reads only the list.
 *
 * kfx_get_indexed_ms: device ms of the last of the two calls (HIP events of
 * their own; the other kfx_get_*_ms figures and these do not touch each other):
 * [0] the world's neighbour table (0 in the window form), [1] counts + scans,
 * [2] vertex emit, [3] index emit ([2], [3]: 0 when nothing was emitted).
 *
 * kfx_write_ply_mesh_indexed: ASCII PLY with kfx_write_ply_mesh_attr's vertex
 * properties and lines, n_verts vertices, n_tris faces "3 i j k".  KFX_ERR_ARG,
 * no file left behind: an index >= n_verts, a null pointer with a positive
 * count, a negative count.
 * kfx_save_mesh_indexed / kfx_save_world_mesh_indexed: one call to size, one to
 * fill, then the writer; the world saver takes kfx_world_bricks first. */
int kfx_extract_mesh_indexed(kfx_ctx *ctx, kfx_vertex *verts, int64_t cap_verts,
                             uint32_t *tris, int64_t cap_tris,
                             int64_t *n_verts, int64_t *n_tris);
int kfx_world_mesh_indexed(kfx_ctx *ctx, const kfx_brick *bricks, int64_t n,
                           kfx_vertex *verts, int64_t cap_verts, uint32_t *tris, int64_t cap_tris,
                           int64_t *n_verts, int64_t *n_tris);
int kfx_get_indexed_ms(kfx_ctx *ctx, float out_ms[4]);
int kfx_write_ply_mesh_indexed(const char *path, const kfx_vertex *verts, int64_t n_verts,
                               const uint32_t *tris, int64_t n_tris);
int kfx_save_mesh_indexed(kfx_ctx *ctx, const char *path);
int kfx_save_world_mesh_indexed(kfx_ctx *ctx, const kfx_brick_store *store, const char *path);

/* ---- world view: free-viewpoint render of window plus evicted bricks
 * Added under ABI version 2, nothing else changed.  kfx_render_view sees the
 * window only; these render a world (a brick list as in the world map above:
 * strictly ascending, an absent brick unobserved) from any camera.
 *
 * A box is origin[3] (world voxels, each a multiple of 8) and dims[3] (voxels,
 * each >= 1, not necessarily a multiple of 8; voxels of a brick past the box
 * and bricks wholly outside it are ignored).  The default box (both pointers
 * NULL) is the list's bounding box in bricks padded by one brick on every side:
 * origin_k = 8 (min b_k - 1), dims_k = 8 (max b_k - min b_k + 3).  The raycast
 * never reads a volume's outermost voxel layer; the pad keeps every listed
 * voxel clear of it.
 *
 * The world view is by definition kfx_render_view (maps and all three images)
 * of a virtual dense volume: dims = the box's; voxel size vs_k = volu_range[k] /
 * (float)volu_dims[k] of the context; range_k = volu_range[k] where dims_k ==
 * volu_dims[k], else (float)dims_k * vs_k; voxel (x, y, z) holds world voxel
 * origin + (x, y, z) of the list; pose R0, t = t0 + R0 (origin * vs) computed as
 * kfx_shift_volume computes its pose (float32, no contraction, that operation
 * order); cam2vol = pose^-1 * cam_pose; KFX_VIEW_COLOR with "lies in the
 * volume" read as "lies in the box".  With the box set to the window
 * (kfx_get_volume_origin, volu_dims) and the window's bricks it equals
 * kfx_render_view byte for byte.  A ray's samples start where it enters the
 * box, so the box is part of the result: two boxes around the same bricks give
 * slightly different images.
 *
 * kfx_world_view_load: uploads the records and builds what the march needs (a
 * grid over the box's bricks and the raycast's skip maps) in buffers of its
 * own: the kfx_world_* extraction calls and this one do not disturb each other.
 * The buffers grow on demand and are freed in kfx_destroy.  The loaded world
 * replaces the previous one; n = 0 unloads it.  It is a snapshot of the list:
 * kfx_reset, frames, shifts and restores do not touch it, and the list may be
 * freed once the call returns.  Stream ordering and blocking as
 * kfx_world_mesh_attr.  KFX_ERR_ARG, the previous world kept: that call's list
 * checks; exactly one of origin / dims NULL; an origin component that is no
 * multiple of 8 or with |origin_k| >= 2^23; a dims component below 1 or above
 * 2^15; a box of more than 2^26 bricks (a default box too).  KFX_ERR_STATE: a
 * slab of a world larger than 1.  KFX_ERR_OOM when a device buffer cannot be
 * allocated (no world is loaded then).
 *
 * kfx_world_view: kfx_render_view's arguments, checks, stream behaviour and
 * blocking; it reads the loaded world only, writes nothing the tracker reads,
 * keeps captured graphs and leaves a pending tracking status to the next
 * kfx_synchronize.  KFX_ERR_STATE when no world is loaded.
 *
 * kfx_get_world_view_ms: device ms (HIP events) of [0] the last load's device
 * work without the upload, [1] the last render's launch.
 * kfx_save_world_view: kfx_world_bricks, kfx_world_view_load with the default
 * box, kfx_world_view, kfx_write_ppm (an empty world: a black image). */
int kfx_world_view_load(kfx_ctx *ctx, const kfx_brick *bricks, int64_t n,
                        const int origin[3], const int dims[3]);
int kfx_world_view(kfx_ctx *ctx, const kfx_intrinsics *view, const kfx_pose *cam_pose,
                   int type, uint8_t *out, float *vmap, float *nmap, float *ts);
int kfx_get_world_view_ms(kfx_ctx *ctx, float out_ms[2]);
int kfx_save_world_view(kfx_ctx *ctx, const kfx_brick_store *store, const kfx_intrinsics *view,
                        const kfx_pose *cam_pose, int type, const char *path);

/* ---- dataset front-end (host only; no GPU needed) --------------------------
 * depth_sensor in its DATASET build (depth_sensor.cpp:11-46 open, :186-196
 * getFrame) without OpenCV: the PNG files of `<dir>/color` and `<dir>/depth` in
 * sorted name order (cv::glob), `<dir>/intr.txt` = the 3x3 camera matrix of
 * which the values > 0.1 are fx, cx, fy, cy, 1.  Frames come out as the
 * reference feeds them to kinectfusion::pipeline: colour = imread(IMREAD_COLOR)
 * (8-bit BGR: 16-bit samples keep the high byte, alpha dropped, grey
 * replicated, palette expanded), depth = imread(IMREAD_UNCHANGED) converted to
 * float (millimetres, one channel required).  Without intr.txt the camera is
 * left 640x480 with zero focal lengths and has_intr = 0. */
typedef struct kfx_dataset kfx_dataset;
int kfx_dataset_open(const char *dir, kfx_dataset **out);
int kfx_dataset_info(const kfx_dataset *ds, kfx_intrinsics *intr, int *n_frames, int *has_intr);
int kfx_dataset_read(const kfx_dataset *ds, int index, uint8_t *bgr, float *depth_mm);
int kfx_dataset_close(kfx_dataset *ds);
/* The PNG decoder and intr.txt parse underneath (any PNG colour type / bit
 * depth, Adam7, CRC-checked; sizes must match). */
int kfx_png_info(const char *path, int *width, int *height, int *channels, int *bit_depth);
int kfx_png_read_bgr8(const char *path, uint8_t *bgr, int width, int height);
int kfx_png_read_depth(const char *path, float *depth, int width, int height);
int kfx_parse_intr(const char *path, float out5[5]);

/* ---- Z-slab sharding (new; the reference is single-GPU) -------------------
 * One kf::kinectfusion stream split over `world` GPUs: slab
 * `rank` owns global z slices [cut(rank), cut(rank+1)) of the volume, cut(r) =
 * floor(Z*r/world) rounded down to a multiple of 8 (cut(world) = Z),
 * and stores 4 halo slices on each side, which it integrates itself.
 * Preprocess and ICP run on every slab (identical results, no collective);
 * raycast events are combined across slabs each frame (all-reduce MIN of the
 * per-pixel event sample index, then all-reduce MAX of the winner's map bits),
 * so every slab ends each frame with the same poses and model maps as a
 * single-GPU kfx_create context, bit for bit. */
int kfx_create_slab(const kfx_intrinsics *intr, const kfx_params *params, int device,
                    int rank, int world, kfx_ctx **out);
/* Work-balanced slabs: slab r owns [cuts[r], cuts[r+1]) (cuts[0] = 0,
 * cuts[world] = Z, multiples of 8, >= 8 slices each; every rank passes the
 * same cuts).  kfx_slice_work gives, per global slice, an estimate of a
 * frame's integrate cost at the first frame's pose (any context, slab or not;
 * from the frame's filtered depth: voxel slots visited plus 1/40 of the
 * slice's X*Y stored slots); kfx_slab_balance turns such a
 * histogram into cuts minimising the largest slab's stored-range work (halos
 * included).  Results stay bit-identical to the single volume for any cuts.
 * Side effect: kfx_slice_work(_parts) preprocesses the given frame into the
 * context's buffer set 0 (current-frame maps, colour input, {depth, 1/lambda}
 * table); the volume, poses and previous-frame maps are untouched.  Called on
 * a context mid-sequence, kfx_get_frame_maps(KFX_FRAME_CUR), kfx_render and
 * kfx_integrate_stats then describe this frame, not the last tracked one:
 * call it before the sequence (as bench.py does) or on a scratch context. */
int kfx_create_slab_cuts(const kfx_intrinsics *intr, const kfx_params *params, int device,
                         int rank, int world, const int *cuts, kfx_ctx **out);
int kfx_slice_work(kfx_ctx *ctx, const uint8_t *bgr, const float *depth_mm, int64_t *work);
/* The two parts kfx_slice_work measures, per global slice (it weighs cover): cover = the voxel
 * slots integrate's waves step through (64 per column tile whose z interval
 * holds the slice), updated = the voxels whose depth test passes. */
int kfx_slice_work_parts(kfx_ctx *ctx, const uint8_t *bgr, const float *depth_mm, int64_t *cover,
                         int64_t *updated);
/* kfx_slice_work of a frame seen from cam_pose (camera-to-world, as in the
 * pose record; null = the identity pose of a first frame), with its parts
 * (cover / updated may be null).  Averaging several frames of a sequence at
 * their poses gives cuts for the whole run rather than its first frame
 * (bench.py --cuts balanced). */
int kfx_slice_work_at(kfx_ctx *ctx, const uint8_t *bgr, const float *depth_mm, const kfx_pose *cam_pose,
                      int64_t *work, int64_t *cover, int64_t *updated);
int kfx_slab_balance(const int64_t *slice_work, int Z, int world, int *cuts);
/* Bounded slab raycast: a slab that combines with others over
 * a communicator or in a kfx_pipeline_group marches each ray only up to the
 * previous frame's model distance along it (+ 16 voxels + 2 %), records where
 * it stopped, and after the all-reduce of [keys | stop points] re-marches the
 * pixels no slab resolved below that point (an exact second pass), so slabs
 * behind the visible surface skip the occluded space.  mode 0: off (every
 * ray marched to its end; the default: on the benchmark scenes the slowest
 * slab holds the surfaces most rays end on, so the bound did not lower it and
 * the second pass cost more); 1: on; 2: on without the margin
 * (test: most pixels take the second pass).  Results are identical in every
 * mode.  The mode decides which collectives a frame's combine issues, so it is
 * one mode for the whole decomposition: on a context with a communicator the
 * call is collective (every rank calls it with the same mode; a mismatch, or
 * a mode outside 0..2 on any rank, returns KFX_ERR_ARG on every rank and
 * leaves the mode unchanged), the mode held at kfx_comm_init is checked the
 * same way (a mismatch there returns KFX_ERR_ARG and leaves the context
 * without a communicator, so no frame can issue mismatched collectives), and
 * kfx_pipeline_group refuses members whose modes differ. */
int kfx_set_slab_bound(kfx_ctx *ctx, int mode);
/* stored slices [zb, zb+zn), owned slices [own0, own1) */
int kfx_slab_info(kfx_ctx *ctx, int *zb, int *zn, int *own0, int *own1);
/* One process per GPU: rank 0 creates the id, every rank passes it to
 * kfx_comm_init (RCCL over xGMI); kfx_pipeline* then combine through RCCL. */
int kfx_comm_get_unique_id(uint8_t id[KFX_COMM_ID_BYTES]);
int kfx_comm_init(kfx_ctx *ctx, const uint8_t id[KFX_COMM_ID_BYTES]);
/* One process driving all slabs (members k = slab k of n, no communicator; on
 * one GPU or on several with peer access): one pipeline() frame. */
int kfx_pipeline_group(kfx_ctx **ctxs, int n, const uint8_t *bgr, const float *depth_mm);
/* kfx_download_tsdf / kfx_download_volume_soa on a slab write its owned slices
 * only (at their global offsets); kfx_upload_tsdf reads its stored slices.
 * With kfx_set_kernel_timing on the members, kfx_pipeline_group runs them one
 * after another (each alone on its GPU, as one rank per GPU would) and every
 * member's kfx_get_kernel_timing_ex reports its own ICP / integrate / local
 * raycast / combine ms. */
/* One slab frame with the exchange done by the caller over any transport
 * (gloo, MPI, ...; a slab context without a communicator):
 * kfx_slab_frame_local runs pipeline()'s frame on this slab up to its local
 * raycast and downloads its per-pixel event keys (n = width*height u32) and
 * {Ts, nx, ny, nz} payload planes (4n u32).  The caller all-reduces the keys
 * with MIN over the slabs, applies kfx_slab_mask_payload with them, all-reduces
 * the payload with MAX and passes it to kfx_slab_frame_finish, which rebuilds
 * the model maps and the pyramid on the device exactly like the RCCL combine
 * and returns pipeline()'s status. */
int kfx_slab_frame_local(kfx_ctx *ctx, const uint8_t *bgr, const float *depth_mm, uint32_t *keys,
                         uint32_t *payload);
int kfx_slab_frame_finish(kfx_ctx *ctx, const uint32_t *payload);

/* ---- ICP residual map and tracking quality ----------------
 * Added under ABI version 2, nothing else changed.  How well the CUR maps of a
 * level fit model maps under a relative pose: rigid_icp.cu:46-113's
 * correspondence gates with the outcome handed out per pixel instead of
 * folded into the 27 sums.
 *
 * Label, one byte per pixel of the level (w * h of them):
 * KFX_ICP_UNCOVERED outside the floor-covered region xe = (w/32)*32,
 * ye = (h/32)*32 the ICP never looks at; inside it the first gate that rejects
 * the pixel, in the kernel's order: NaN current normal (x component); vcur.z > 0
 * and the rounded projection inside the image; |vcur - vpre|^2 <= dist2_max;
 * |ncur x npre|^2 <= sine2_max (the thresholds in kfx_stage_icp_accumulate's
 * one-compare form; a NaN fails its gate); else KFX_ICP_ACCEPT.
 * Residual: r = dot(npre, vpre - vcur) of an accepted pixel, the row's seventh
 * entry in float32; 0.0f everywhere else.
 * Record: n[k] pixels of label k (they sum to w * h); sum_r2 the sum over
 * accepted pixels of rint(RN(r * r) * 2^32), exact and order-independent like
 * the 27 sums (|r| is a row entry: the bound checked at kfx_create covers it);
 * max_abs_r the largest |r| accepted, 0 when there is none.
 *
 * kfx_quality_figures (host only, no context):
 *   fitness = n[0] / (double)(n[0] + n[2] + n[3] + n[4])   (0 when that is 0)
 *   rmse    = sqrt(((double)sum_r2 / 4294967296.0) / (double)n[0])   (0 when n[0] is 0)
 * in double in this order; KFX_ERR_ARG on a null pointer or a negative count.
 *
 * kfx_stage_icp_residuals: kfx_stage_icp_accumulate's inputs (CUR against PREV
 * maps of `level` under the relative `pose`).  residual / label: w * h of that
 * level; any of the three outputs may be NULL, not all.  DevState is not
 * written: kfx_debug_get_icp_sums / kfx_debug_get_icp_step report what they
 * did before.
 * kfx_score_poses: the records of n relative poses in one launch (no per-pixel
 * output); out[k] is kfx_stage_icp_residuals' record of poses[k].  A block
 * walks kfx_quality_chunk(w, h, n) poses with its pixels in registers.  n = 0
 * does no device work; n above 2^16 or a non-finite pose entry returns
 * KFX_ERR_ARG with nothing written.
 * kfx_frame_quality: kfx_stage_icp_residuals under the identity on the maps as
 * they stand behind every queued frame: CUR, the measured maps of the last
 * frame, against PREV, the model raycast from that frame's pose: how well the
 * last frame sits on the model it was fused into.  kfx_stage_preprocess and
 * kfx_slice_work* replace the CUR maps.  After a bootstrap frame PREV holds
 * the measured maps (residuals 0); after a dropped frame what the reset left.
 * kfx_score_view: the CUR maps of `level` against the volume seen from the
 * world pose cam_pose: the model maps are kfx_render_view's vmap / nmap at
 * that level's intrinsics (one direct raycast, no resize pyramid, with the pose
 * in effect that kfx_render_view uses), then the identity relative pose.  The
 * hypothesis test for relocalisation or for resuming on an uploaded volume.
 * KFX_ERR_ARG on a non-finite pose entry, KFX_ERR_STATE on one slab of several.
 * kfx_get_quality_ms: device ms (HIP events) of the last residual launch or
 * batch [0] and of the view raycast in front of it [1] (0: there was none).
 *
 * All of them behave as kfx_render_view: on the context's stream behind every
 * queued frame (staged and overlapped ones included), blocking until the data
 * is on the host, writing only buffers of their own (grown on demand, freed in
 * kfx_destroy), outside every captured graph, and a pending tracking status is
 * left to the next kfx_synchronize.  All but kfx_score_view work on any slab
 * context (the maps are replicated).  KFX_ERR_ARG: level outside 0..L-1, a
 * null pose, every output null. */
#define KFX_ICP_ACCEPT 0
#define KFX_ICP_NAN 1
#define KFX_ICP_PROJ 2
#define KFX_ICP_DIST 3
#define KFX_ICP_ANGLE 4
#define KFX_ICP_UNCOVERED 5
typedef struct kfx_icp_quality {
  int64_t n[6];      /* pixels per label; they sum to the level's w*h */
  int64_t sum_r2;    /* sum over accepted pixels of rint(RN(r*r) * 2^32): the sums' fixed point */
  float   max_abs_r; /* max |r| over accepted pixels, 0 when there is none */
  int32_t level;
} kfx_icp_quality;   /* 64 bytes */
#ifdef __cplusplus
static_assert(sizeof(kfx_icp_quality) == 64, "kfx_icp_quality is 64 bytes");
#else
_Static_assert(sizeof(kfx_icp_quality) == 64, "kfx_icp_quality is 64 bytes");
#endif
int kfx_stage_icp_residuals(kfx_ctx *ctx, int level, const kfx_pose *pose, float *residual, uint8_t *label,
                            kfx_icp_quality *q);
int kfx_score_poses(kfx_ctx *ctx, int level, const kfx_pose *poses, int64_t n, kfx_icp_quality *out);
int kfx_frame_quality(kfx_ctx *ctx, int level, float *residual, uint8_t *label, kfx_icp_quality *q);
int kfx_score_view(kfx_ctx *ctx, int level, const kfx_pose *cam_pose, float *residual, uint8_t *label,
                   kfx_icp_quality *q);
int kfx_get_quality_ms(kfx_ctx *ctx, float out_ms[2]);
int kfx_quality_figures(const kfx_icp_quality *q, double *fitness, double *rmse);
/* poses per block of a kfx_score_poses batch of n >= 1 at a w x h level: with
 * pb = ceil(w * h / 1024) pixel blocks, clamp(n / ceil(512 / pb), 1, 16)
 * (integer division): the most, up to 16, that leave a grid of 512 blocks. */
int kfx_quality_chunk(int width, int height, int64_t n);

/* ---- multi-start ICP, tracking against a view, resuming at a pose
 * Added under ABI version 2, nothing else changed.  The tracker's coarse-to-fine
 * loop (ICPRegistration::rigidTransform, icp_registration.cpp:16-46: levels
 * L-1 .. 0, icp_iter_count[level] iterations each, the context's thresholds)
 * from each of n start poses instead of the identity, all n in one launch per
 * (level, iteration): 19 launches at the defaults whatever n is.  Each pose
 * runs kfx_stage_icp's arithmetic (exact int64 sums, the 3+3 block solve with
 * its determinant test, Rodrigues, pose = pose * Tinc), so out[k] is bit for
 * bit what the loop gives from starts[k], whatever the batch around it.  A
 * pose whose solve fails the determinant test stops there: status
 * KFX_TRACKING_LOST, (stop_level, stop_iter) the failing solve, pose the one
 * reached before it; the others go on.
 *
 * kfx_icp_multi: CUR against the PREV maps as they stand (kfx_stage_icp's
 * inputs).  n in 0..2^16; n = 0 returns KFX_OK and touches nothing.
 * KFX_ERR_ARG, with nothing written: n outside that, a null starts or out, a
 * non-finite pose entry.  q (may be NULL): n records, out[k].pose scored at
 * level 0 on the same model maps (kfx_score_poses' record; a lost pose is
 * scored where it stopped).
 * kfx_track_view: the same loop against the volume seen from the world pose
 * cam_pose.  The model maps are a pyramid of the call's own: at every level
 * one direct raycast at that level's intrinsics (kfx_score_view's maps of that
 * level, not the resize pyramid).  world (may be NULL): world[k] = cam_pose *
 * out[k].pose, the camera's world pose, composed on the host in float32 in
 * the order of the tracker's pose product.  KFX_ERR_ARG also on a null or
 * non-finite cam_pose; KFX_ERR_STATE on one slab of several.
 * kfx_icp_multi_chunk (host only, no context): poses one block walks in a
 * batch of n >= 1 at a w x h level: with pb = max(1, ceil(xe * ye / 1024))
 * pixel blocks of the floor-covered region (xe = (w/32)*32, ye = (h/32)*32),
 * clamp(n / ceil(512 / pb), 1, 16) (integer division).  Results do not depend
 * on it.
 * kfx_get_icp_multi_ms: device ms (HIP events) of the last call: the view
 * raycasts [0] (0: kfx_icp_multi), the loop's launches [1], the scoring [2]
 * (0: q was NULL).
 *
 * Both calls behave as kfx_render_view and kfx_score_poses: on the context's
 * stream behind every queued frame, blocking, writing only buffers of their
 * own (grown on demand, freed in kfx_destroy), outside every captured graph;
 * DevState is not written (kfx_debug_get_icp_sums / kfx_debug_get_icp_step
 * report what they did before) and a pending tracking status is left to the
 * next kfx_synchronize.
 *
 * kfx_resume_at: the next frame tracks from the world pose cam_pose against
 * the volume as it stands (after kfx_upload_tsdf on a fresh context: resume on
 * a restored volume).  Waits for every queued frame, appends cam_pose to the
 * pose record (KFX_ERR_STATE when the record is full), sets the frame count to
 * max(frame count, 1) + 1 so that the next frame tracks instead of
 * bootstrapping, and writes the PREV maps a frame tracked at cam_pose would
 * have left: kfx_stage_raycast at cam2vol = inv(volume pose in effect) *
 * cam_pose with the resize pyramid.  Holds in every graph mode, with frame
 * overlap on or off.  KFX_ERR_ARG on a null or non-finite pose, KFX_ERR_STATE
 * on one slab of several.  The only call of this section that writes tracker
 * state; a pending tracking status is left to the next kfx_synchronize. */
typedef struct kfx_icp_result {
  kfx_pose pose;      /* relative pose reached (the start, if no solve succeeded) */
  int32_t status;     /* KFX_OK or KFX_TRACKING_LOST */
  int32_t stop_level, stop_iter; /* the failing solve; -1, -1 when status is KFX_OK */
  int32_t solves;     /* solves that succeeded */
  double x[6];        /* last successful solve's increment; zeros if none */
} kfx_icp_result;     /* 112 bytes */
#ifdef __cplusplus
static_assert(sizeof(kfx_icp_result) == 112, "kfx_icp_result is 112 bytes");
#else
_Static_assert(sizeof(kfx_icp_result) == 112, "kfx_icp_result is 112 bytes");
#endif
int kfx_icp_multi(kfx_ctx *ctx, const kfx_pose *starts, int64_t n, kfx_icp_result *out, kfx_icp_quality *q);
int kfx_track_view(kfx_ctx *ctx, const kfx_pose *cam_pose, const kfx_pose *starts, int64_t n, kfx_icp_result *out,
                   kfx_pose *world, kfx_icp_quality *q);
int kfx_resume_at(kfx_ctx *ctx, const kfx_pose *cam_pose);
int kfx_icp_multi_chunk(int width, int height, int64_t n);
int kfx_get_icp_multi_ms(kfx_ctx *ctx, float out_ms[3]);

/* ---- relocalisation: fern keyframes, batched search, map kept on loss
 * Added under ABI version 2, nothing else changed.  The source of pose
 * hypotheses §26 / §27 left to the caller: a device-resident keyframe store
 * with randomized-fern frame codes (Glocker et al., "Real-Time RGB-D Camera
 * Relocalization via Randomized Ferns for Keyframe Encoding"), a batched
 * nearest-keyframe search, and the per-frame call that uses both without ever
 * dropping the map.  Off the frame path: no frame kernel or graph changes.
 *
 * Fern grid: the coarsest pyramid level L-1, wL x hL pixels, s = 2^(L-1).
 * Fern: kfx_fern, 0 <= x < wL, 0 <= y < hL, td in metres.
 * Table: m ferns, m a multiple of 16 in 16..1024, supplied by the caller or
 * generated from (seed, depth_min_mm, depth_max_mm) with splitmix64
 *   state += 0x9E3779B97F4A7C15; z = state;
 *   z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB;
 *   next = z ^ z>>31
 * per fern in this order: x = next % wL, y = next % hL, tb, tg, tr each
 * next % 256, td = (float)(depth_min_mm + next % (depth_max_mm - depth_min_mm
 * + 1)) / 1000.0f (one float32 division).  Defaults (a NULL kfx_fern_params):
 * m = 512, seed = 2013, depth 400..4000 mm.
 * Code of a frame: the frame is the CUR maps as they stand and the BGR image
 * they were made from (the one last given with kfx_pipeline* or
 * kfx_stage_preprocess: what the integrate stage would fuse).  Fern f yields a
 * nibble: bit 0 is SumB > tb * s*s, SumB the integer sum of the B bytes over the
 * s x s block of full-resolution pixels [x*s, x*s+s) x [y*s, y*s+s); bits 1
 * and 2 the same for G and R; bit 3 is d > td, d the CUR dmap of level L-1 at
 * (x, y) in metres (kfx_get_frame_maps; a hole, d = 0, gives 0).  Every compare
 * is strict and the arithmetic integer or one float compare: the code is exact.
 * Packed: m/16 uint64_t words, fern f in word f/16, bits 4*(f%16) .. +3.
 * Distance of two codes: the ferns whose nibbles differ, 0..m.
 * Match order: ascending (distance, keyframe id); the key is unique, so every
 * result is deterministic whatever the grid.
 * Keyframe: an id (0, 1, 2, ... in order of insertion, never reused), a world
 * camera pose and a code.
 *
 * kfx_fern_table (host only): the generated table for a camera and pyramid
 * height.  kfx_keyframes_create: an empty store on ctx's device (table NULL:
 * generated; params NULL: the defaults; with a table only n_ferns is used).
 * kfx_encode_frame: the frame's code (m/16 words).  kfx_keyframes_add: encode
 * and store at cam_pose (NULL: kfx_get_cur_camera_pose).  kfx_keyframes_put: a
 * pose and a code made elsewhere (host only; uploaded by the next call that
 * needs it).  kfx_keyframes_consider: encode, find the nearest keyframe, add
 * the frame at the current pose iff the store is empty or that distance is
 * > min_distance; *id the new id or -1, *nearest (may be NULL) the nearest
 * before the add ({-1, -1}: the store was empty).  kfx_keyframes_get: either
 * output may be NULL.  kfx_keyframes_search: the k nearest keyframes of each of
 * q codes (NULL: the frame's own code, q = 1) in match order, q*k entries;
 * slots past the store's size are {-1, -1}.  q in 0..65536 (0: nothing done,
 * KFX_OK), k in 1..16.  One launch per batch plus a small merge: a block keeps
 * 256 keyframes' words in registers and walks kfx_keyframes_search_chunk(n, q)
 * queries (host only: with kb = ceil(n / 256) keyframe blocks,
 * clamp(q / ceil(512 / kb), 1, 16)); results do not depend on it.
 * kfx_keyframes_export / _import: the store as plain data (a magic word, a
 * version, the parameters, grid, table, poses, codes).  blob NULL or cap too
 * small: *bytes alone is written (KFX_OK when blob is NULL, else KFX_ERR_ARG).
 * A blob that is truncated, corrupted or whose m or grid disagrees with the
 * importing context: KFX_ERR_ARG.  kfx_get_keyframe_ms: device ms (HIP events)
 * of the last encode [0] and the last search [1].
 *
 * The calls that take a context behave as kfx_score_poses: on the frame stream
 * behind every queued frame, blocking, writing only buffers of their own
 * (grown on demand, freed in kfx_destroy or kfx_keyframes_destroy), outside
 * every captured graph; DevState is not written and a pending tracking status
 * is left to the next kfx_synchronize.  A store is tied to the device and the
 * fern grid of the context it was created with (another context: KFX_ERR_ARG)
 * and may outlive it only for the host-only calls.  Argument errors write
 * nothing.
 *
 * kfx_relocalise, on the CUR maps as they stand: encode the frame, search the k
 * nearest keyframes, and for each match in match order run
 * kfx_track_view(keyframe pose, starts, n, ..., q) (starts NULL: the identity,
 * n = 1).  The candidates are the (match, start) pairs whose status is KFX_OK.
 * The winner has the largest fitness n[0] / (n[0]+n[2]+n[3]+n[4]), compared
 * exactly by integer cross-multiplication (a zero denominator loses); a tie
 * goes to the smaller sum_r2 / n[0] by a 128-bit cross product, then to the
 * earlier match, then the earlier start.  It is accepted iff
 * kfx_quality_figures' fitness >= min_fitness: status KFX_OK, the return value
 * too; else status and return value KFX_TRACKING_LOST, keyframe, distance and
 * start -1 and world, icp, q zero.  n_matches: keyframes retrieved;
 * n_converged: candidates.  Writes no tracker state: the caller adopts the pose
 * with kfx_resume_at.  KFX_ERR_STATE on one slab of several.
 *
 * kfx_pipeline_recover: "probe, then commit", composed on the host from the
 * calls above, so a committed frame is a kfx_pipeline frame.  Frame count 1:
 * kfx_pipeline, event 1.  Otherwise probe with kfx_stage_preprocess and
 * kfx_stage_icp (DevState restored, nothing reset).  Probe KFX_OK:
 * kfx_pipeline, event 0.  Probe lost: kfx_relocalise(k, identity,
 * min_fitness); a candidate accepted: kfx_resume_at(world) and probe again;
 * that probe KFX_OK: kfx_pipeline, event 2; lost: event 3, return
 * KFX_TRACKING_LOST, the volume untouched (the pose kfx_resume_at appended
 * stays in the pose record, and PREV is the model seen from it).  No candidate:
 * event 3, KFX_TRACKING_LOST, nothing written but the CUR maps.  After event
 * 0, 1 or 2, if kfx_frame_quality's level-0 fitness >= harvest_min_fitness (the
 * bootstrap frame always passes): kfx_keyframes_consider(harvest_min_distance),
 * keyframe_added = the new id or -1.  report->reloc is kfx_relocalise's result
 * where it ran, else status KFX_OK with -1 / zero fields.  params NULL: k = 4,
 * harvest_min_distance = m / 10, min_fitness = 0.15, harvest_min_fitness = 0.25
 * (a frame at its tracked pose reads 0.28..0.50 on the synthetic sequences, one
 * turned 5 degrees away 0.08: DESIGN.md §26, §28).
 * The price over kfx_pipeline is one extra preprocess and kfx_stage_icp per
 * frame, with their host syncs.  KFX_ERR_STATE on one slab of
 * several.  Holds in graph mode 0 and 1, with frame overlap on or off. */
typedef struct kfx_fern {
  int32_t x, y;
  uint8_t tb, tg, tr, pad;
  float td;
} kfx_fern; /* 16 bytes */
typedef struct kfx_keyframes kfx_keyframes; /* device-resident, tied to ctx's device */
typedef struct kfx_fern_params {
  int32_t n_ferns;
  uint32_t depth_min_mm, depth_max_mm;
  uint64_t seed;
} kfx_fern_params;
typedef struct kfx_keyframe_match {
  int32_t id;
  int32_t distance;
} kfx_keyframe_match;
typedef struct kfx_reloc_result {
  int32_t status;                    /* KFX_OK: a candidate was accepted; KFX_TRACKING_LOST: none */
  int32_t keyframe, distance, start; /* the winning candidate (-1 when none) */
  int32_t n_matches, n_converged;
  kfx_pose world;                    /* camera world pose of the winner */
  kfx_icp_result icp;
  kfx_icp_quality q;
} kfx_reloc_result; /* 248 bytes */
typedef struct kfx_recover_params {
  int32_t k;
  int32_t harvest_min_distance;
  double min_fitness, harvest_min_fitness;
} kfx_recover_params;
typedef struct kfx_recover_report {
  int32_t event; /* 0 tracked, 1 bootstrap, 2 relocalised, 3 lost, map kept */
  int32_t keyframe_added;
  kfx_reloc_result reloc;
} kfx_recover_report;
#ifdef __cplusplus
static_assert(sizeof(kfx_fern) == 16 && sizeof(kfx_reloc_result) == 248, "kfx_fern is 16 bytes, kfx_reloc_result 248");
#else
_Static_assert(sizeof(kfx_fern) == 16 && sizeof(kfx_reloc_result) == 248, "kfx_fern is 16 bytes, kfx_reloc_result 248");
#endif
int kfx_fern_table(const kfx_intrinsics *intr, int pyramid_height, const kfx_fern_params *params, kfx_fern *out);
int kfx_keyframes_create(kfx_ctx *ctx, const kfx_fern_params *params, const kfx_fern *table, kfx_keyframes **out);
int kfx_keyframes_destroy(kfx_keyframes *kf);
int kfx_keyframes_get_table(const kfx_keyframes *kf, kfx_fern *out);
int kfx_keyframes_count(const kfx_keyframes *kf, int64_t *n);
int kfx_encode_frame(kfx_ctx *ctx, kfx_keyframes *kf, uint64_t *code);
int kfx_keyframes_add(kfx_ctx *ctx, kfx_keyframes *kf, const kfx_pose *cam_pose, int32_t *id);
int kfx_keyframes_put(kfx_keyframes *kf, const kfx_pose *cam_pose, const uint64_t *code, int32_t *id);
int kfx_keyframes_consider(kfx_ctx *ctx, kfx_keyframes *kf, int32_t min_distance, int32_t *id,
                           kfx_keyframe_match *nearest);
int kfx_keyframes_get(const kfx_keyframes *kf, int32_t id, kfx_pose *cam_pose, uint64_t *code);
int kfx_keyframes_search(kfx_ctx *ctx, kfx_keyframes *kf, const uint64_t *codes, int64_t q, int k,
                         kfx_keyframe_match *out);
int kfx_keyframes_search_chunk(int64_t n_keyframes, int64_t q);
int kfx_keyframes_export(const kfx_keyframes *kf, void *blob, int64_t cap, int64_t *bytes);
int kfx_keyframes_import(kfx_ctx *ctx, const void *blob, int64_t bytes, kfx_keyframes **out);
int kfx_get_keyframe_ms(kfx_ctx *ctx, float out_ms[2]);
int kfx_relocalise(kfx_ctx *ctx, kfx_keyframes *kf, int k, const kfx_pose *starts, int64_t n, double min_fitness,
                   kfx_reloc_result *out);
int kfx_pipeline_recover(kfx_ctx *ctx, kfx_keyframes *kf, const uint8_t *bgr, const float *depth_mm,
                         const kfx_recover_params *params, kfx_recover_report *report);

#ifdef __cplusplus
}
#endif
#endif /* KFX_H */
