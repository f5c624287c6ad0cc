// kfx_ctx.h — what the host files behind the C-ABI share: the context, the
// error and allocation helpers.  Included by kfx_api.hip (which defines the
// functions declared here) and kfx_export.hip; no kernel file includes it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/kfx.h"
#include "kfx_internal.h"

using namespace kfx;  // (a host file's header: both includers name the kfx types unqualified)

// per-frame stage events: [0] start, [1] preprocess done, [2] ICP done,
// [3] integrate done, [4] frame done, [5] local raycast done, [6] combine starts,
// [7] / [8] a group combine's shared part (reductions, masks, resume) starts / ends
constexpr int kStageEvents = 9;

// What the last overlapped frame left for the next one (enqueue_frame_overlap
// reads it at its start and rewrites it at its end; nothing else writes it).
//
// Overlapped frame k runs its preprocess on pstream into buffer set p = k & 1
// and its ICP / integrate / raycast on the frame stream, which waits for
// ev_prep (recorded on pstream behind the preprocess).  Frame k's pstream work
// always starts behind ONE wait on frame k-1, the "start wait": for
// start_sig >= sig when frame k-1's raycast signals its start (sig != 0), else
// for ev_icp, which frame k-1 recorded behind its integrate.  Either way it
// completes only after frame k-1's integrate has, and the frame stream is in
// order, so after everything enqueued on the frame stream before that
// integrate.  (DESIGN.md §13 has the measurements behind this schedule.)
//
//  - Buffer set p.  Its last user is frame k-2's ICP / integrate / raycast, on
//    the frame stream before frame k-1's integrate: when `chained`, the start
//    wait alone orders the preprocess after it, and no ev_free[p] record was
//    or is made (each record between two frame kernels costs the frame stream
//    2-5 us).  Otherwise the preprocess also waits for ev_free[p], which the
//    last user of set p recorded at its end (free_rec[p]) or which is recorded
//    now, at the frame stream's tail.
//  - k_int_order (deep volumes: it rewrites the tile order the integrate reads)
//    runs on pstream between the preprocess and the ev_prep record when
//    order_pending.  The start wait orders it after frame k-1's integrate, the
//    one that read the old order and left the intervals it sorts; ev_prep,
//    which the frame stream waits for before frame k's ICP, orders it before
//    the integrate that reads the new order.  Neither depends on ev_free: with
//    the ev_free record elided the start wait is still enqueued, and it is
//    that wait, not ev_free, that orders the cross-stream k_int_order.
//  - `chained` holds only if the API call before this one (api_seq) enqueued
//    frame k-1.  Any call in between (a single-stream frame into set 0, a
//    stage hook, a group call) may have put work on the frame stream behind
//    frame k-1's integrate that uses set p or runs an integrate, which the
//    start wait does not cover: the chain is broken, and the ev_free[p] wait at
//    the stream's tail orders the preprocess and k_int_order after that work.
struct OverlapCarry {
  bool chained = false;              // the frame provides the start wait (signal, or ev_icp behind its integrate) ...
  unsigned long long api_seq = 0;    // ... and was enqueued by this API call
  unsigned sig = 0;                  // the serial its raycast signals (0: it recorded ev_icp)
  bool order_pending = false;        // its integrate left k_int_order to the next frame's pstream
  bool free_rec[2]{};                // the last frame that used set p recorded ev_free[p]
};

struct kfx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  kfx_intrinsics intr{};
  kfx_params p{};
  int L = 0;
  LevelGeom g[kMaxLevels]{};
  float angle_thr = 0.f;

  float *raw[kMaxLevels]{};  // raw[0] = f32 mm input, raw[l] = pyrDown outputs
  uint16_t *raw0_u16 = nullptr;
  uint8_t *bgr = nullptr;
  FrameView cur{}, prev{};
  float *inv_lambda = nullptr;
  float2 *dl0 = nullptr;  // level-0 {depth m, 1/lambda}, the integrate gather table (+ dmax shards)
  // cur maps, dl0 and the ICP plan over them are double-buffered: with frame
  // overlap, frame k+1's preprocess (on pstream) fills one set while frame k's
  // ICP / integrate / raycast (on stream) read the other.  cur/dl0/icp_plan
  // above alias set `par`, the one the last frame used.
  FrameView curb[2]{};
  float2 *dl0b[2]{};
  unsigned long long *skipcnt = nullptr;  // VolView::skipcnt's three words (kfx_debug_count_settled)
  char *itab = nullptr;  // VolView::itab's allocation (kfx_debug_int_tiles switches the view's pointer)
  IcpPlan planb[2]{};
  int par = 0;
  bool overlap = true;
  hipStream_t pstream = nullptr;
  hipEvent_t ev_prep = nullptr, ev_free[2]{};
  unsigned long long api_seq = 0;  // API calls into this context (counted by check_ctx)
  hipEvent_t ev_icp = nullptr;  // after the last overlapped frame's integrate (a group member: its ICP): the next preprocess starts there
  hipEvent_t ev_group = nullptr;  // kfx_pipeline_group combine: fork (member 0) / join (the others)
  // raycast start signal: fine-grained word an overlapped frame's raycast
  // stores its serial to as it starts; the next preprocess waits for it with
  // hipStreamWaitValue32 on its own stream (null: unsupported, ev_icp instead)
  unsigned *start_sig = nullptr;
  unsigned sig_serial = 0;  // the last serial handed out (serials only grow: the word holds the latest one stored)
  OverlapCarry ov;          // what the last overlapped frame left for the next one
  bool group_chain = false;     // kfx_pipeline_group member: record ev_icp after every ICP
  bool graphs_stale = false;    // a refused persistent ICP launch: captured graphs still hold it

  // sampled kernel timing (kfx_set_kernel_timing): every `timing_every`-th
  // pipelined frame records its stage events into the next unused set
  int timing_every = 0;
  unsigned long long frame_seq = 0;
  std::vector<hipEvent_t> tsets;  // kStageEvents per sample
  size_t tnext = 0;
  VolView vol{};
  DevState *st = nullptr;
  DevPose *pose_log = nullptr;
  int pose_cap = 0;
  unsigned long long *icp_shards = nullptr;  // 8 x 27 int64 + ticket (self-resetting)
  unsigned *icp_ticket = nullptr;
  IcpSync *icp_sync = nullptr;  // persistent ICP barrier + per-iteration shard slots
  IcpPlan icp_plan{};
  long long icp_exact_pixels = 0;  // pixels one block may sum exactly (icp_exact_pixels of the intrinsics)
  bool icp_persistent = false;  // plan fits and its grid is co-resident
  bool icp_persistent_enabled = true;
  bool icp_coop = false;  // cooperative launch of the persistent ICP (after a watchdog stall, or asked for)
  bool icp_sharded = false;  // slab ranks: ICP partials all-reduced (kfx_set_icp_allreduce)
  unsigned long long *counters = nullptr;
  float *xpose = nullptr;  // explicit stage poses (21 floats: pose R,t + Rinv)
  std::vector<void *> allocs;

  float *staged_depth = nullptr;
  uint8_t *staged_bgr = nullptr;
  int n_staged = 0;

  bool graph_mode = true;
  bool profiling = false;
  hipGraphExec_t graph[2] = {nullptr, nullptr};  // [u16 input], inputs in raw[0]/bgr
  std::vector<hipGraphExec_t> staged_graph;       // one per staged frame (reads it in place)
  // overlapped staged frames: per staged frame and buffer set p, [4i+2p] the
  // pyrDown/preprocess graph (pstream), [4i+2p+1] the ICP/integrate/raycast graph
  std::vector<hipGraphExec_t> ov_graph;
  bool ov_graph_full = false;  // also capture ICP/integrate/raycast (kfx_set_graph_mode 2)
  bool ov_main_refused = false;  // the main graph's capture failed (RCCL refused capture): eager
  hipError_t cap_err = hipSuccess;  // the last capture's HIP error (capture_graph)
  std::string graph_note;           // why the main graph was dropped (kfx_get_graph_note)
  const uint8_t *last_bgr = nullptr;              // colour the last frame integrated
  hipEvent_t ev[kStageEvents]{};  // stage events; [5]: local raycast done, [6]: combine starts (slabs)
  float stage_ms[5]{};
  int pending = 0;      // frames enqueued since the last host sync
  int known_poses = 1;  // n_poses at the last sync
  int known_fails = 0;  // DevState::fails at the last status check

  // Z-slab sharding: this context owns slab `rank` of `world`
  bool slab = false;
  int rank = 0, world = 1;
  uint8_t *render = nullptr;      // kfx_render output (allocated on first use)
  // kfx_render_view: output pixels and [vmap | nmap | ts] planes (allocated on
  // first use, grown for a larger view, freed in kfx_destroy), launch events
  uint8_t *view_out = nullptr;
  float *view_maps = nullptr;
  size_t view_out_cap = 0, view_maps_cap = 0;
  hipEvent_t ev_view[2]{};
  float view_ms = 0.f;            // device time of the last view's launch
  // moving volume: the pose the context was created with, the
  // accumulated shift in voxels (p.volu_pose is derived from both), and the
  // events around the last eviction's passes [0, 1] and the last shift [2, 3]
  kfx_pose volu_pose0{};
  int origin[3] = {0, 0, 0};
  hipEvent_t ev_shift[4]{};
  bool shift_timed[2] = {false, false};
  // bricks out and back in: the events around the last
  // kfx_evict_bricks [0, 1] and the last kfx_restore_bricks [2, 3]
  hipEvent_t ev_stream[4]{};
  bool stream_timed[2] = {false, false};
  // world map: the uploaded records, the neighbour table's
  // keys and entries, the count / scan workspace and the items (each grown on
  // demand, kept, freed in kfx_destroy), and the events around the last call's
  // table [0, 1], count + scan [1, 2] and emit [3, 4]
  void *world_buf[5]{};
  size_t world_cap[5]{};
  hipEvent_t ev_world[5]{};
  float world_ms[3]{};
  // indexed mesh: the world form's face list (its vertices and
  // their keys use world_buf[4]; grown on demand, kept, freed in kfx_destroy),
  // and the events of the last call, window or world: the table begins [0],
  // the count [1], scans done [2], vertex emit begins [3], index emit begins
  // [4], done [5]
  void *world_tris = nullptr;
  size_t world_tris_cap = 0;
  hipEvent_t ev_indexed[6]{};
  float indexed_ms[4]{};
  // world view: the loaded world.  Buffers of its own (grown
  // on demand, kept, freed in kfx_destroy): [0] the records, [1] the grid over
  // the box's bricks, [2] / [3] the box's occupancy maps.  wv_vol describes the
  // box as a volume (kfx_internal.h WorldGrid); wv_n = 0: nothing loaded.  The
  // images go through kfx_render_view's staging buffers.  Events: the last
  // load's device work [0, 1], the last render's launch [2, 3].
  void *wv_buf[4]{};
  size_t wv_cap[4]{};
  VolView wv_vol{};
  size_t wv_n = 0, wv_cells = 0;
  int wv_origin[3] = {0, 0, 0};
  DevPose wv_pose{};
  hipEvent_t ev_wv[4]{};
  float wv_ms[2]{};
  // ICP residuals and quality records.  Buffers of its own
  // (grown on demand, kept, freed in kfx_destroy): [0] the poses, [1] the
  // records, [2] residuals, [3] labels, [4] kfx_score_view's model maps
  // [vmap | nmap].  Events: the view raycast [0, 1], the residual launch [2, 3].
  void *q_buf[5]{};
  size_t q_cap[5]{};
  hipEvent_t ev_q[4]{};
  float q_ms[2]{};
  // multi-start ICP.  Buffers of its own (grown on demand,
  // kept, freed in kfx_destroy): [0] the batch's poses (IcpMultiPose), [1] their
  // sum rows and tickets, [2] kfx_track_view's model pyramid, per level
  // [vmap | nmap | the view's image].  Events: the view raycasts [0, 1], the
  // iterations' launches [2, 3].  m_ms: raycasts, loop, final scoring.
  void *m_buf[3]{};
  size_t m_cap[3]{};
  hipEvent_t ev_m[4]{};
  float m_ms[3]{};
  // fern keyframes.  Buffers of its own (grown on demand, kept,
  // freed in kfx_destroy): [0] a search's queries, [1] its per-block keys, [2]
  // its results.  Events: the last encode [0, 1], the last search [2, 3].
  void *kf_buf[3]{};
  size_t kf_cap[3]{};
  hipEvent_t ev_kf[4]{};
  float kf_ms[2]{};
  uint8_t *mc_tab = nullptr;    // marching-cubes table (uploaded on first use)
  // per pixel: [key | pend | Ts | nx | ny | nz] planes (k_raycast<kSlab>): the
  // sample index of this slab's decisive event, the first sample a bounded
  // march left unexamined, and the hit payload
  uint32_t *key_local = nullptr;
  uint32_t *key_min = nullptr;    // all-reduce MIN of the [key | pend] planes over the slabs
  int slab_bound = 0;             // kfx_set_slab_bound: 0 off (default: measured no faster), 1 on, 2 no margin
  bool group_combine = false;     // kfx_pipeline_group member (in-process combine), this call only
  bool pass1_bounded = false;     // the frame's slab raycast was bounded: the combine runs pass 2
  // kfx_pipeline_async: host frames copied into a pinned ring slot, uploaded on
  // the copy stream while earlier frames run (slot reuse ordered by events)
  static constexpr int kRing = 4;
  uint8_t *ring_host = nullptr, *ring_dev = nullptr;
  uint8_t *ring_host_dev = nullptr;  // ring_host as mapped into the device address space
  size_t ring_slot = 0;  // bytes per slot: f32 depth + BGR8
  hipEvent_t ring_h2d[kRing]{}, ring_done[kRing]{};
  bool ring_used[kRing]{};
  unsigned ring_sig[kRing]{};  // the raycast start signal of the slot's last frame (0: wait ring_done)
  hipGraphExec_t ring_graph[kRing][2][4]{};  // overlapped-frame graphs per slot and [u16 input]
  int ring_next = 0;
  bool ring_ready = false;  // every ring resource above created
  struct HostReg {
    uintptr_t host;
    size_t bytes;
    uint8_t *dev;  // the same pages mapped into the device address space
  };
  std::vector<HostReg> host_regs;  // kfx_register_host_buffer ranges
  hipStream_t cstream = nullptr;
  ncclComm_t comm = nullptr;      // RCCL communicator over the slab ranks (one process per GPU)
  int *comm_chk = nullptr;        // 2 device words of the collective slab-bound check (kfx_comm_init)
  hipEvent_t xev[5]{};            // extraction pass events (kfx_get_extract_ms)
  int extract_passes = 0;         // the last extraction: 1 (single pass) or 2 (count + emit)
  int extract_mode = 1;           // kfx_set_extract_passes: 1 single pass when a buffer is given, 2 always two
  float extract_ms[3]{};          // last extraction: count pass, scan, emit pass
  bool ext_open = false;          // kfx_slab_frame_local done, kfx_slab_frame_finish due
  hipEvent_t *ext_pending = nullptr;  // that frame's timing sample
};

#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return set_err(KFX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

namespace kfx {

// the text kfx_last_error returns (per thread); returns code
int set_err(int code, const std::string &msg);
// every API call's first step: counts the call, selects the context's device
int check_ctx(kfx_ctx *c);
// a zeroed device buffer that lives as long as the context (freed in kfx_destroy)
int dalloc(kfx_ctx *c, void **p, size_t bytes);
DevPose to_dev(const kfx_pose &p);
kfx_pose to_api(const DevPose &d);
// the volume pose of voxel origin o; the caller has both streams idle
void set_volume_origin(kfx_ctx *c, const int o[3]);
// kfx_brick_store.cpp: the store's bricks (s may be null: none) merged with the
// nw ascending bricks `win`, ascending, `win` winning an equal coordinate;
// returns how many there are and writes them when out is not null
int64_t brick_store_merge(const kfx_brick_store *s, const kfx_brick *win, int64_t nw, kfx_brick *out);

}  // namespace kfx
