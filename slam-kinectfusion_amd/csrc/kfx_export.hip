// kfx_export.hip — the host side of what reads the model out: the
// free-viewpoint render, point cloud / mesh extraction and PLY files, the
// moving volume, bricks out and back in, the world map, the indexed mesh and the world view
// (DESIGN.md §18, §20-§25), and of what scores, tracks and relocalises off the frame path (§26-§28).
// Host code only (no __global__ function: the kernels are in kfx_extract / kfx_view / kfx_shift /
// kfx_world / kfx_world_view / kfx_quality / kfx_reloc.hip); no frame runs any of it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "kfx_ctx.h"
#include "kfx_multi.h"
#include "kfx_reloc.h"
#include "kfx_scanws.h"

// The keyframe store: the host mirror (table, poses, codes) and
// on `device` the table, the word-major code table (word w of keyframe i at
// d_codes[w * cap + i]; keyframes [0, synced) are uploaded, the rest wait for
// the next call that searches) and the m / 16 words of the last encode.
struct kfx_keyframes {
  KeyframeHost h;
  int device = 0;
  int width = 0, height = 0;  // the camera whose frames it encodes
  kfx_fern *d_table = nullptr;
  unsigned long long *d_codes = nullptr, *d_code = nullptr;
  int64_t cap = 0, synced = 0;
};

namespace {

int hip_err(const char *call, hipError_t e) {
  (void)hipGetLastError();
  return set_err(KFX_ERR_HIP, std::string(call) + ": " + hipGetErrorString(e));
}

// grow a device buffer to at least `bytes` (never shrunk; nothing queued uses
// it: every call that reserves ends with a sync)
int reserve(void **p, size_t *cap, size_t bytes, const char *what) {
  if (*cap >= bytes) return KFX_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    *p = nullptr;
    (void)hipGetLastError();
    return set_err(KFX_ERR_OOM, std::string(what) + ": hipMalloc(" + std::to_string(bytes) + "): " + hipGetErrorString(e));
  }
  *cap = bytes;
  return KFX_OK;
}

// a device buffer one call owns: freed on every way out of the call
struct CallBuf {
  void *p = nullptr;
  size_t cap = 0;
  CallBuf() = default;
  CallBuf(const CallBuf &) = delete;
  CallBuf &operator=(const CallBuf &) = delete;
  ~CallBuf() {
    if (p) (void)hipFree(p);
  }
};

int make_events(hipEvent_t *ev, int n) {
  for (int i = 0; i < n; ++i)
    if (!ev[i]) HIPCHK(hipEventCreate(&ev[i]));
  return KFX_OK;
}

// out_ms[k] = the span ev[2k] .. ev[2k + 1] where timed[k], else 0 (kfx_get_shift_ms, kfx_get_stream_ms)
int timed_spans(kfx_ctx *c, const hipEvent_t ev[4], const bool timed[2], float out_ms[2]) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out_ms) return set_err(KFX_ERR_ARG, "null ms");
  for (int k = 0; k < 2; ++k) {
    out_ms[k] = 0.f;
    if (!timed[k]) continue;
    HIPCHK(hipEventSynchronize(ev[2 * k + 1]));
    HIPCHK(hipEventElapsedTime(&out_ms[k], ev[2 * k], ev[2 * k + 1]));
  }
  return KFX_OK;
}

// The export protocol: a count pass over n > 0 units, the
// offset scan, the total to the host, then min(total, cap) items of `item`
// bytes emitted at the scanned offsets into *items (grown to hold them: a
// CallBuf's, or one the context keeps) and copied to `out`.
//   count(w)              launches the pass that fills w.counts (and may fill
//                         w.total[1], [2]) on c->stream
//   emit(w, head, dst, m) launches the pass that writes the first m items to
//                         dst; head = the kScanHeadWords words at w.total
// One download and one sync when nothing is emitted (cap == 0 or total == 0),
// else two of each.  ev: the events recorded on the way (null: none): before
// the count, behind it, behind the scan, before the emit, and `end` behind the
// emit, or where nothing is emitted behind the total's download.
// *total is written once the count is known, also when a later step fails.
struct ScanEvents {
  hipEvent_t begin, counted, scanned, emit_begin, end;
};
// One counted quantity of an export: its workspace, the bytes of an item, the
// caller's buffer and cap, the device buffer the items are emitted into, and
// where the total goes.  side: device bytes per item reserved behind the m
// emitted items (at *items + m * item) that are not copied out.
struct ScanPart {
  ScanWs w;
  size_t item, side;
  int64_t cap;
  void *out;
  void **items;
  size_t *items_cap;
  int64_t *total;
};
// The protocol over kParts quantities counted by one pass (the indexed mesh:
// vertices and triangles): one scan and one total each, one emit call for all.
//   count(part)          fills every part[i].w.counts
//   emit(part, head, m)  writes the first m[i] items of each part to
//                        *part[i].items; head[i] = the words at part[i].w.total.
//                        Returns KFX_OK, or an error before it launches anything.
// whole: every part is emitted in full when every out is non-null and every
// total fits its cap, else nothing is (m[i] = 0 for all); without it each part
// gets its prefix min(total, cap).
template <int kParts, class Count, class Emit>
int count_scan_emit_parts(kfx_ctx *c, const char *call, const ScanPart (&part)[kParts], size_t n, bool whole,
                          const ScanEvents &ev, Count count, Emit emit) {
  hipStream_t s = c->stream;
  hipError_t e = hipSuccess;
  auto mark = [&](hipEvent_t x) {
    if (x && e == hipSuccess) e = hipEventRecord(x, s);
  };
  mark(ev.begin);
  count(part);
  mark(ev.counted);
  for (const ScanPart &p : part) launch_scan(s, p.w.counts, p.w.offsets, p.w.bsum, n, p.w.total);
  mark(ev.scanned);
  if (e == hipSuccess) e = hipGetLastError();
  unsigned long long head[kParts][kScanHeadWords] = {};
  for (int i = 0; i < kParts; ++i)
    if (e == hipSuccess) e = hipMemcpyAsync(head[i], part[i].w.total, sizeof(head[i]), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_err(call, e);
  unsigned long long m[kParts];
  bool fits = true, any = false;
  for (int i = 0; i < kParts; ++i) {
    *part[i].total = (int64_t)head[i][0];
    m[i] = (unsigned long long)std::min<int64_t>(*part[i].total, part[i].cap);
    fits = fits && part[i].out && *part[i].total <= part[i].cap;
  }
  for (int i = 0; i < kParts; ++i) {
    if (whole && !fits) m[i] = 0;
    any = any || m[i] > 0;
  }
  if (any) {
    for (int i = 0; i < kParts; ++i) {
      const int r = m[i] ? reserve(part[i].items, part[i].items_cap, (size_t)m[i] * (part[i].item + part[i].side), call) : KFX_OK;
      if (r) return r;
    }
    mark(ev.emit_begin);
    const int r = emit(part, head, m);
    if (r) return r;
    if (e == hipSuccess) e = hipGetLastError();
    mark(ev.end);
    for (int i = 0; i < kParts; ++i)
      if (m[i] && e == hipSuccess)
        e = hipMemcpyAsync(part[i].out, *part[i].items, (size_t)m[i] * part[i].item, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  } else {
    mark(ev.end);
  }
  return e == hipSuccess ? KFX_OK : hip_err(call, e);
}
// one counted quantity, a prefix of min(total, cap) items (the comment above)
template <class Count, class Emit>
int count_scan_emit(kfx_ctx *c, const char *call, const ScanWs &w, size_t n, size_t item, int64_t cap, void *out,
                    void **items, size_t *items_cap, const ScanEvents &ev, Count count, Emit emit, int64_t *total) {
  const ScanPart part[1] = {{w, item, 0, cap, out, items, items_cap, total}};
  return count_scan_emit_parts<1>(
      c, call, part, n, false, ev, [&](const ScanPart(&p)[1]) { count(p[0].w); },
      [&](const ScanPart(&p)[1], const unsigned long long(&head)[1][kScanHeadWords], const unsigned long long(&m)[1]) {
        emit(p[0].w, head[0], *p[0].items, m[0]);
        return KFX_OK;
      });
}

// the workspace of n units (+ extra bytes) in a buffer of the caller's
int scan_workspace(void **p, size_t *cap, size_t n, size_t extra, const char *call, ScanWs *w) {
  const int r = reserve(p, cap, scanws_layout(nullptr, n, extra).bytes, call);
  if (!r) *w = scanws_layout(*p, n, extra);
  return r;
}

// kfx_evict_points / kfx_evict_bricks behind their argument checks: the
// protocol over `units` units with per-call buffers, inside the one span
// ev[0] .. ev[1] their getter reports (recorded also when there is no unit)
template <class Count, class Emit>
int evict_items(kfx_ctx *c, const char *call, hipEvent_t ev[4], bool *timed, size_t units, size_t item, int64_t cap,
                void *out, int64_t *n, Count count, Emit emit) {
  int r = make_events(ev, 4);
  if (r) return r;
  HIPCHK(hipStreamSynchronize(c->stream));
  int64_t total = 0;
  HIPCHK(hipEventRecord(ev[0], c->stream));
  if (units > 0) {
    CallBuf ws, items;
    ScanWs w;
    if ((r = scan_workspace(&ws.p, &ws.cap, units, 0, call, &w))) return r;
    const ScanEvents marks = {nullptr, nullptr, nullptr, nullptr, ev[1]};
    if ((r = count_scan_emit(c, call, w, units, item, cap, out, &items.p, &items.cap, marks, count, emit, &total)))
      return r;
  } else {
    HIPCHK(hipEventRecord(ev[1], c->stream));
  }
  *timed = true;
  if (n) *n = total;
  return KFX_OK;
}

// The indexed mesh, both forms behind their checks, through the driver with two counted
// quantities per unit: vertices (28 bytes, a 16-bit key beside each on the
// device) and triangles (3 indices).  Both are emitted in full or not at all.
//   pass(which, wv, wt, verts, keys, tris)  launches pass 0 (the counts), 1 (the
//   vertices) or 2 (the indices) over the `units` units
// ws: the two scan workspaces' buffer; vbuf / tbuf: the device items.  ev[1..5]
// as kfx_ctx::ev_indexed; sets indexed_ms[1..3].
template <class Pass>
int indexed_run(kfx_ctx *c, const char *call, size_t units, void **ws, size_t *ws_cap, void **vbuf,
                       size_t *vbuf_cap, void **tbuf, size_t *tbuf_cap, kfx_vertex *verts, int64_t cap_verts,
                       uint32_t *tris, int64_t cap_tris, int64_t *n_verts, int64_t *n_tris, Pass pass) {
  ScanWs wv;
  int r = scan_workspace(ws, ws_cap, units, scanws_layout(nullptr, units).bytes, call, &wv);
  if (r) return r;
  const ScanWs wt = scanws_layout(wv.extra, units);  // (extra starts on a multiple of kScanAlign)
  hipEvent_t *ev = c->ev_indexed;
  const ScanEvents marks = {ev[1], nullptr, ev[2], ev[3], ev[5]};
  const ScanPart part[2] = {{wv, sizeof(kfx_vertex), sizeof(uint16_t), cap_verts, verts, vbuf, vbuf_cap, n_verts},
                            {wt, 3 * sizeof(uint32_t), 0, cap_tris, tris, tbuf, tbuf_cap, n_tris}};
  bool emitted = false;
  hipError_t mid = hipSuccess;
  r = count_scan_emit_parts<2>(
      c, call, part, units, true, marks,
      [&](const ScanPart(&)[2]) { pass(0, wv, wt, nullptr, nullptr, nullptr); },
      [&](const ScanPart(&)[2], const unsigned long long(&)[2][kScanHeadWords], const unsigned long long(&m)[2]) {
        if (m[0] > 0xffffffffull) return set_err(KFX_ERR_STATE, std::string(call) + ": more than 2^32 - 1 vertices");
        uint16_t *keys = reinterpret_cast<uint16_t *>(static_cast<char *>(*vbuf) + (size_t)m[0] * sizeof(kfx_vertex));
        pass(1, wv, wt, *vbuf, keys, nullptr);
        mid = hipEventRecord(ev[4], c->stream);
        if (m[1]) pass(2, wv, wt, *vbuf, keys, static_cast<uint32_t *>(*tbuf));
        emitted = true;
        return (int)KFX_OK;
      });
  if (r) return r;
  if (mid != hipSuccess) return hip_err(call, mid);
  if (*n_verts > (int64_t)0xffffffffll) return set_err(KFX_ERR_STATE, std::string(call) + ": more than 2^32 - 1 vertices");
  HIPCHK(hipEventElapsedTime(&c->indexed_ms[1], ev[1], ev[2]));
  if (emitted) {
    HIPCHK(hipEventElapsedTime(&c->indexed_ms[2], ev[3], ev[4]));
    HIPCHK(hipEventElapsedTime(&c->indexed_ms[3], ev[4], ev[5]));
  }
  return KFX_OK;
}

// An indexed mesh to a PLY file: size, fill, write; extract(verts, cap_verts, tris, cap_tris, &nv, &nt) is one of the two calls
template <class Extract>
int save_indexed(const char *path, const char *call, Extract extract) {
  int64_t nv = 0, nt = 0;
  int r = extract(nullptr, 0, nullptr, 0, &nv, &nt);
  if (r) return r;
  std::vector<kfx_vertex> v;
  std::vector<uint32_t> t;
  try {
    v.resize((size_t)nv);
    t.resize((size_t)nt * 3);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, std::string(call) + ": out of memory");
  }
  if (nv > 0 && (r = extract(v.data(), nv, t.data(), nt, &nv, &nt))) return r;
  return kfx_write_ply_mesh_indexed(path, v.data(), nv, t.data(), nt);
}

// Affine3f product and rigid inverse in the float order of the device's
// pose_mul / pose_inv (k_ray_pose; the oracle's kfo_pose_mul / kfo_pose_inv):
// this file is built without contraction, so the host sums round the same.
DevPose host_pose_mul(const DevPose &a, const DevPose &b) {
  DevPose r;
  pose_mul_f32(a.R, a.t, b.R, b.t, r.R, r.t);  // (kfx_multi.h: the same loops, where a host check can build them)
  return r;
}
DevPose host_pose_inv(const DevPose &a) {
  DevPose r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.R[3 * i + j] = a.R[3 * j + i];
  for (int j = 0; j < 3; ++j) {
    float d = 0.f;
    for (int k = 0; k < 3; ++k) d += a.R[3 * k + j] * a.t[k];
    r.t[j] = -d;
  }
  return r;
}

// What the two view calls do once their own refusals are past: reserve the
// staging buffers (`who` names the call in an out-of-memory message), place the
// optional maps in view_maps as [vmap | nmap | ts], compose cam2vol =
// box_pose^-1 * cam_pose (tsdf_volume.cpp:59), launch(g, cam2vol, eye, vmap,
// nmap, ts) between the two events ev, copy out what was asked
// for and leave the launch's device time in *ms.  On the frame stream, behind
// every queued frame's integrate; nothing the tracker reads is written, and
// the pending tracking status is left alone.
template <class Launch>
int view_run(kfx_ctx *c, const char *who, hipEvent_t *ev, float *ms, const DevPose &box_pose,
             const kfx_intrinsics *view, const kfx_pose *cam_pose, uint8_t *out, float *vmap, float *nmap, float *ts,
             Launch launch) {
  int r;
  const size_t np = (size_t)view->width * view->height;
  const bool maps = vmap || nmap || ts;
  if ((r = reserve((void **)&c->view_out, &c->view_out_cap, 3 * np, who))) return r;
  if (maps && (r = reserve((void **)&c->view_maps, &c->view_maps_cap, 28 * np, who))) return r;
  if ((r = make_events(ev, 2))) return r;
  float *dv = vmap ? c->view_maps : nullptr, *dn = nmap ? c->view_maps + 3 * np : nullptr,
        *dt = ts ? c->view_maps + 6 * np : nullptr;
  const DevPose cam = to_dev(*cam_pose);
  const DevPose c2v = host_pose_mul(host_pose_inv(box_pose), cam);
  const LevelGeom g = {view->width, view->height, view->fx, view->fy, view->cx, view->cy};
  HIPCHK(hipEventRecord(ev[0], c->stream));
  launch(g, c2v, cam.t, dv, dn, dt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev[1], c->stream));
  HIPCHK(hipMemcpyAsync(out, c->view_out, 3 * np, hipMemcpyDeviceToHost, c->stream));
  if (vmap) HIPCHK(hipMemcpyAsync(vmap, dv, 12 * np, hipMemcpyDeviceToHost, c->stream));
  if (nmap) HIPCHK(hipMemcpyAsync(nmap, dn, 12 * np, hipMemcpyDeviceToHost, c->stream));
  if (ts) HIPCHK(hipMemcpyAsync(ts, dt, 4 * np, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipEventElapsedTime(ms, ev[0], ev[1]));
  return KFX_OK;
}

}  // namespace

extern "C" {

// ---- free-viewpoint render --------------------------------

// a view's size (kfx_save_world_view checks it before anything else: null is a bad size there)
static int view_size(const kfx_intrinsics *view) {
  if (!view || view->width < 1 || view->height < 1 || (int64_t)view->width * view->height > ((int64_t)1 << 26))
    return set_err(KFX_ERR_ARG, "view size: width, height >= 1 and width * height <= 2^26");
  return KFX_OK;
}

// the argument checks kfx_render_view and kfx_world_view share
static int view_args(const kfx_intrinsics *view, const kfx_pose *cam_pose, const uint8_t *out, int type) {
  if (!view || !cam_pose || !out) return set_err(KFX_ERR_ARG, "null argument");
  if (type < KFX_VIEW_PHONG || type > KFX_VIEW_COLOR) return set_err(KFX_ERR_ARG, "view type outside 0..2");
  if (int r = view_size(view)) return r;
  if (!std::isfinite(view->fx) || !std::isfinite(view->fy) || view->fx == 0.f || view->fy == 0.f ||
      !std::isfinite(view->cx) || !std::isfinite(view->cy))
    return set_err(KFX_ERR_ARG, "view intrinsics: finite, fx and fy non-zero");
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(i < 9 ? cam_pose->R[i] : cam_pose->t[i - 9])) return set_err(KFX_ERR_ARG, "non-finite view pose");
  return KFX_OK;
}

int kfx_render_view(kfx_ctx *c, const kfx_intrinsics *view, const kfx_pose *cam_pose, int type, uint8_t *out,
                    float *vmap, float *nmap, float *ts) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = view_args(view, cam_pose, out, type))) return r;
  if (c->slab && c->world > 1) return set_err(KFX_ERR_STATE, "render_view on one slab of several");
  return view_run(c, "render_view", c->ev_view, &c->view_ms, to_dev(c->p.volu_pose), view, cam_pose, out, vmap, nmap,
                  ts, [&](const LevelGeom &g, const DevPose &c2v, const float *eye, float *dv, float *dn, float *dt) {
                    launch_view(c->stream, c->vol, g, c2v, eye, type, c->view_out, dv, dn, dt);
                  });
}

int kfx_get_view_ms(kfx_ctx *c, float *ms) {
  int r = check_ctx(c);
  if (r) return r;
  if (!ms) return set_err(KFX_ERR_ARG, "null ms");
  *ms = c->view_ms;
  return KFX_OK;
}

int kfx_write_ppm(const char *path, const uint8_t *bgr, int width, int height) {
  if (!path || !bgr || width < 1 || height < 1) return set_err(KFX_ERR_ARG, "bad argument");
  FILE *f = std::fopen(path, "wb");
  if (!f) return set_err(KFX_ERR_ARG, std::string("cannot open ") + path);
  std::fprintf(f, "P6\n%d %d\n255\n", width, height);
  std::vector<uint8_t> row(3 * (size_t)width);
  bool ok = true;
  for (int y = 0; y < height && ok; ++y) {
    const uint8_t *s = bgr + 3 * (size_t)y * width;
    for (int x = 0; x < width; ++x) {
      row[3 * x] = s[3 * x + 2];
      row[3 * x + 1] = s[3 * x + 1];
      row[3 * x + 2] = s[3 * x];
    }
    ok = std::fwrite(row.data(), 1, row.size(), f) == row.size();
  }
  ok = (std::fclose(f) == 0) && ok;
  return ok ? KFX_OK : set_err(KFX_ERR_ARG, std::string("write failed: ") + path);
}

// ---- point cloud / PLY -----------------------------------------------------

int kfx_set_extract_passes(kfx_ctx *c, int passes) {
  int r = check_ctx(c);
  if (r) return r;
  if (passes != 1 && passes != 2) return set_err(KFX_ERR_ARG, "extract passes are 1 or 2");
  c->extract_mode = passes;
  return KFX_OK;
}

int kfx_get_extract_passes(kfx_ctx *c, int *passes) {
  int r = check_ctx(c);
  if (r) return r;
  if (!passes) return set_err(KFX_ERR_ARG, "null out");
  *passes = c->extract_passes;
  return KFX_OK;
}

int kfx_get_extract_ms(kfx_ctx *c, float out_ms[3]) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out_ms) return set_err(KFX_ERR_ARG, "null out");
  for (int i = 0; i < 3; ++i) out_ms[i] = c->extract_ms[i];
  return KFX_OK;
}

// words per item: 3 per point, 9 per triangle; attributed 7 / 21 (kfx_vertex
// is 7 words: kfx_extract.hip kVertexWords)
static_assert(sizeof(kfx_vertex) == 28, "kfx_vertex is 7 32-bit words");
static int extract_item_words(bool mesh, bool attr) { return (mesh ? 3 : 1) * (attr ? 7 : 3); }

// one extraction's sweep over the slices [zlo, zhi): tab = null for points,
// the marching-cubes table for triangles
struct ExtractSweep {
  kfx_ctx *c;
  const uint8_t *tab;
  int zlo, zhi;
  bool attr;
  DevPose vp;
  // offs == null: counts per wave; else the first n items to dst at offs
  void pass(unsigned *counts, const unsigned long long *offs, float *dst, unsigned long long n) const {
    if (tab)
      launch_mesh(c->stream, c->vol, vp, zlo, zhi, tab, counts, offs, dst, n, attr);
    else
      launch_extract(c->stream, c->vol, vp, zlo, zhi, counts, offs, dst, n, attr);
  }
};

// One extraction of up to cap items over `waves` > 0 waves, through the driver.
// pool = false: the sweep counts, then emits (two reads of the volume).
// pool = true: ONE read of the volume.  The count pass is k_extract_pool
// (counts + items into an unordered pool), the emit pass k_extract_copy (pool
// -> canonical order); if the pool cannot hold every item the counts are
// still complete (w.total = {total, pool counter, overflow flag}) and the
// sweep's emit pass writes the first cap items instead.
// Sets kfx_get_extract_ms (count pass, scan, emit pass or 0 when nothing was
// emitted) and kfx_get_extract_passes when it succeeds.
constexpr int64_t kExtractPoolItems = (int64_t)1 << 23;  // single-pass pool: <= 8.4 M items (100 MB of points)
static int extract_run(const ExtractSweep &sw, const char *call, size_t waves, bool pool, void *out, int64_t cap,
                       int64_t *total) {
  kfx_ctx *c = sw.c;
  const int per = extract_item_words(sw.tab != nullptr, sw.attr);
  // the unordered pool holds at most kExtractPoolItems items whatever the
  // caller's cap (a larger result overflows it and takes the emit pass); the
  // ordered output is allocated once the count is known (min(total, cap)
  // items, not cap).  An attributed call's pool has the plain call's bytes,
  // not its item count (3/7 of the items): a 2048^3 call allocates what it did before.
  const int64_t pool_cap =
      std::min<int64_t>(cap, kExtractPoolItems * extract_item_words(sw.tab != nullptr, false) / per);
  // behind the scan's regions: where each wave's items lie in the pool, and the waves that have any
  const size_t o_list = scan_align(waves * 8);
  CallBuf ws, pl, items;
  ScanWs w;
  int r;
  if ((r = scan_workspace(&ws.p, &ws.cap, waves, pool ? o_list + scan_align(waves * 4) : 0, call, &w)) ||
      (pool && (r = reserve(&pl.p, &pl.cap, (size_t)pool_cap * per * sizeof(float), call))) ||
      (r = make_events(c->xev, 5)))
    return r;
  unsigned long long *pool_at = (unsigned long long *)w.extra;
  unsigned *list = pool ? (unsigned *)(w.extra + o_list) : nullptr;
  if (pool) HIPCHK(hipMemsetAsync(w.total, 0, kScanAlign, c->stream));
  bool overflow = !pool;
  const ScanEvents marks = {c->xev[0], c->xev[1], c->xev[2], c->xev[3], c->xev[4]};
  r = count_scan_emit(
      c, call, w, waves, (size_t)per * sizeof(float), cap, out, &items.p, &items.cap, marks,
      [&](const ScanWs &) {
        if (pool)
          launch_extract_pool(c->stream, c->vol, sw.vp, sw.zlo, sw.zhi, sw.tab, w.counts, w.total + 1, pool_at, list,
                              (float *)pl.p, (unsigned long long)pool_cap, (unsigned *)(w.total + 2), sw.attr);
        else
          sw.pass(w.counts, nullptr, nullptr, 0);
      },
      [&](const ScanWs &, const unsigned long long *head, void *dst, unsigned long long m) {
        if (pool) overflow = (unsigned)head[2] != 0;
        if (!overflow)
          launch_extract_copy(c->stream, list, (unsigned)(head[1] >> 40), w.counts, pool_at, w.offsets,
                              (const float *)pl.p, (float *)dst, m, per);
        else
          sw.pass(w.counts, w.offsets, (float *)dst, m);
      },
      total);
  if (r) return r;
  (void)hipEventElapsedTime(&c->extract_ms[0], c->xev[0], c->xev[1]);
  (void)hipEventElapsedTime(&c->extract_ms[1], c->xev[1], c->xev[2]);
  c->extract_ms[2] = 0.f;
  if (std::min(*total, cap) > 0) (void)hipEventElapsedTime(&c->extract_ms[2], c->xev[3], c->xev[4]);
  c->extract_passes = overflow ? 2 : 1;
  return KFX_OK;
}

static void build_mc_table(uint8_t tab[256 * 16]);

// the marching-cubes table, uploaded on first use
static int ensure_mc_table(kfx_ctx *c) {
  if (c->mc_tab) return KFX_OK;
  uint8_t tab[256 * 16];
  build_mc_table(tab);
  int r = dalloc(c, (void **)&c->mc_tab, sizeof(tab));
  if (r) return r;
  HIPCHK(hipMemcpy(c->mc_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
  return KFX_OK;
}

// kfx_extract_points / kfx_extract_mesh and their _attr forms: `out` holds cap
// items of extract_item_words(mesh, attr) 32-bit words.
static int extract_items(kfx_ctx *c, bool mesh, bool attr, void *out, int64_t cap, int64_t *n_items) {
  int r = check_ctx(c);
  if (r) return r;
  if (cap < 0 || (cap > 0 && !out)) return set_err(KFX_ERR_ARG, mesh ? "bad triangle buffer" : "bad point buffer");
  HIPCHK(hipStreamSynchronize(c->stream));
  if (mesh && (r = ensure_mc_table(c))) return r;
  // FullScan6 visits z = 0 .. Z-2 (it reads z + 1), as do the cubes z .. z+1;
  // a slab its owned part
  const ExtractSweep sw = {c,    mesh ? c->mc_tab : nullptr, std::max(0, c->vol.own0), std::min(c->vol.own1, c->vol.Z - 1),
                           attr, to_dev(c->p.volu_pose)};
  const char *call = mesh ? "extract_mesh" : "extract_points";
  const size_t waves = extract_waves(c->vol, sw.zlo, sw.zhi);
  int64_t total = 0;
  // one read of the volume into the caller's buffer; not for a count-only
  // call (cap = 0) or with kfx_set_extract_passes(2), and where it fails (its
  // buffers cannot be allocated) the two passes run instead
  const bool single = cap > 0 && cap <= (int64_t)1 << 36 && c->extract_mode != 2;
  if (waves == 0)
    c->extract_passes = 2;
  else if (!(single && extract_run(sw, call, waves, true, out, cap, &total) == KFX_OK) &&
           (r = extract_run(sw, call, waves, false, out, cap, &total)))
    return r;
  if (n_items) *n_items = total;
  return KFX_OK;
}


int kfx_extract_points(kfx_ctx *c, float *xyz, int64_t cap, int64_t *n_points) {
  return extract_items(c, false, false, xyz, cap, n_points);
}
int kfx_extract_points_attr(kfx_ctx *c, kfx_vertex *out, int64_t cap, int64_t *n_points) {
  return extract_items(c, false, true, out, cap, n_points);
}

// Marching-cubes triangle table, derived instead of typed in: for each of the
// 256 inside/outside corner patterns, every cube face contributes one segment
// per run of inside corners along its cycle (counter-clockwise seen from
// outside), from the edge entering the run to the edge leaving it — so on an
// ambiguous face the two inside corners are cut off separately, the same way
// from both cubes sharing the face (no cracks).  Each cut edge then starts one
// segment and ends one; the segments close into loops, each loop is fanned
// from its smallest edge index.  At most 5 triangles per cube.
static void build_mc_table(uint8_t tab[256 * 16]) {
  int lo[12], hi[12], n = 0;
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < 8; ++c)
      if (!((c >> a) & 1)) {
        lo[n] = c;
        hi[n] = c | (1 << a);
        ++n;
      }
  auto eid = [&](int u, int v) {
    for (int e = 0; e < 12; ++e)
      if ((lo[e] == u && hi[e] == v) || (lo[e] == v && hi[e] == u)) return e;
    return -1;
  };
  int cyc[6][4];
  for (int a = 0, f = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    static const int pb[4] = {0, 1, 1, 0}, pc[4] = {0, 0, 1, 1};
    for (int s = 0; s < 2; ++s, ++f)
      for (int i = 0; i < 4; ++i) {
        const int k = s ? i : 3 - i;  // the x=0 / y=0 / z=0 face reversed: outward normal -e_a
        cyc[f][i] = (s << a) | (pb[k] << b) | (pc[k] << c);
      }
  }
  std::memset(tab, 0, 256 * 16);
  for (int cfg = 0; cfg < 256; ++cfg) {
    int nxt[12];
    for (int &x : nxt) x = -1;
    for (int f = 0; f < 6; ++f) {
      bool ins[4];
      for (int i = 0; i < 4; ++i) ins[i] = (cfg >> cyc[f][i]) & 1;
      for (int i = 0; i < 4; ++i) {
        if (!ins[i] || ins[(i + 3) % 4]) continue;  // start of a run of inside corners
        int j = i;
        while (ins[(j + 1) % 4]) j = (j + 1) % 4;
        nxt[eid(cyc[f][(i + 3) % 4], cyc[f][i])] = eid(cyc[f][j], cyc[f][(j + 1) % 4]);
      }
    }
    bool seen[12] = {};
    int nt = 0;
    for (int s = 0; s < 12; ++s) {
      if (nxt[s] < 0 || seen[s]) continue;
      int loop[12], m = 0;
      for (int e = s; !seen[e]; e = nxt[e]) {
        seen[e] = true;
        loop[m++] = e;
      }
      for (int k = 1; k + 1 < m; ++k, ++nt) {
        tab[16 * cfg + 1 + 3 * nt] = (uint8_t)loop[0];
        tab[16 * cfg + 2 + 3 * nt] = (uint8_t)loop[k];
        tab[16 * cfg + 3 + 3 * nt] = (uint8_t)loop[k + 1];
      }
    }
    tab[16 * cfg] = (uint8_t)nt;
  }
}

int kfx_extract_mesh(kfx_ctx *c, float *tri_xyz, int64_t cap, int64_t *n_tris) {
  return extract_items(c, true, false, tri_xyz, cap, n_tris);
}
int kfx_extract_mesh_attr(kfx_ctx *c, kfx_vertex *out, int64_t cap, int64_t *n_tris) {
  return extract_items(c, true, true, out, cap, n_tris);
}

int kfx_write_ply_mesh(const char *path, const float *tri_xyz, int64_t n) {
  if (!path || n < 0 || (n > 0 && !tri_xyz)) return set_err(KFX_ERR_ARG, "bad argument");
  FILE *f = std::fopen(path, "w");
  if (!f) return set_err(KFX_ERR_ARG, std::string("cannot open ") + path);
  std::fprintf(f, "ply\nformat ascii 1.0\nelement vertex %lld\nproperty float x\nproperty float y\n"
               "property float z\nelement face %lld\nproperty list uchar int vertex_indices\nend_header\n",
               (long long)(3 * n), (long long)n);
  for (int64_t i = 0; i < 3 * n; ++i)
    std::fprintf(f, "%g %g %g\n", tri_xyz[3 * i], tri_xyz[3 * i + 1], tri_xyz[3 * i + 2]);
  for (int64_t i = 0; i < n; ++i)
    std::fprintf(f, "3 %lld %lld %lld\n", (long long)(3 * i), (long long)(3 * i + 1), (long long)(3 * i + 2));
  std::fclose(f);
  return KFX_OK;
}

int kfx_write_ply(const char *path, const float *xyz, int64_t n) {
  if (!path || n < 0 || (n > 0 && !xyz)) return set_err(KFX_ERR_ARG, "bad argument");
  FILE *f = std::fopen(path, "w");
  if (!f) return set_err(KFX_ERR_ARG, std::string("cannot open ") + path);
  // kinectfusion.cpp:154-165: ostream << float uses the default "%g" (6 digits)
  std::fprintf(f, "ply\nformat ascii 1.0\nelement vertex %lld\nproperty float x\nproperty float y\n"
               "property float z\nend_header\n", (long long)n);
  for (int64_t i = 0; i < n; ++i)
    std::fprintf(f, "%g %g %g\n", xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  std::fclose(f);
  return KFX_OK;
}

int kfx_save_pointcloud(kfx_ctx *c, const char *path, int64_t cap) {
  if (!path) return set_err(KFX_ERR_ARG, "null path");
  if (cap <= 0) cap = KFX_DEFAULT_CLOUD_POINTS;
  int64_t total = 0;
  int r = kfx_extract_points(c, nullptr, 0, &total);
  if (r) return r;
  const int64_t n = std::min(total, cap);
  std::vector<float> pts((size_t)n * 3);
  if (n > 0 && (r = kfx_extract_points(c, pts.data(), n, &total))) return r;
  return kfx_write_ply(path, pts.data(), n);
}

// x y z nx ny nz red green blue per vertex (n_verts of them), after the header
static void ply_attr_vertices(FILE *f, const kfx_vertex *v, int64_t n_verts) {
  for (int64_t i = 0; i < n_verts; ++i)
    std::fprintf(f, "%g %g %g %g %g %g %d %d %d\n", v[i].x, v[i].y, v[i].z, v[i].nx, v[i].ny, v[i].nz, (int)v[i].r,
                 (int)v[i].g, (int)v[i].b);
}
static const char kPlyAttrProps[] =
    "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
    "property float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n";

int kfx_write_ply_attr(const char *path, const kfx_vertex *v, int64_t n) {
  if (!path || n < 0 || (n > 0 && !v)) return set_err(KFX_ERR_ARG, "bad argument");
  FILE *f = std::fopen(path, "w");
  if (!f) return set_err(KFX_ERR_ARG, std::string("cannot open ") + path);
  std::fprintf(f, "ply\nformat ascii 1.0\nelement vertex %lld\n%send_header\n", (long long)n, kPlyAttrProps);
  ply_attr_vertices(f, v, n);
  std::fclose(f);
  return KFX_OK;
}

int kfx_write_ply_mesh_attr(const char *path, const kfx_vertex *v, int64_t n) {
  if (!path || n < 0 || (n > 0 && !v)) return set_err(KFX_ERR_ARG, "bad argument");
  FILE *f = std::fopen(path, "w");
  if (!f) return set_err(KFX_ERR_ARG, std::string("cannot open ") + path);
  std::fprintf(f, "ply\nformat ascii 1.0\nelement vertex %lld\n%s"
               "element face %lld\nproperty list uchar int vertex_indices\nend_header\n",
               (long long)(3 * n), kPlyAttrProps, (long long)n);
  ply_attr_vertices(f, v, 3 * n);
  for (int64_t i = 0; i < n; ++i)
    std::fprintf(f, "3 %lld %lld %lld\n", (long long)(3 * i), (long long)(3 * i + 1), (long long)(3 * i + 2));
  std::fclose(f);
  return KFX_OK;
}

// count, then extract min(total, cap) items and write them
static int save_attr(kfx_ctx *c, const char *path, int64_t cap, bool mesh) {
  if (!path) return set_err(KFX_ERR_ARG, "null path");
  if (cap <= 0) cap = KFX_DEFAULT_CLOUD_POINTS;
  int64_t total = 0;
  int r = extract_items(c, mesh, true, nullptr, 0, &total);
  if (r) return r;
  const int64_t n = std::min(total, cap);
  std::vector<kfx_vertex> v((size_t)n * (mesh ? 3 : 1));
  if (n > 0 && (r = extract_items(c, mesh, true, v.data(), n, &total))) return r;
  return mesh ? kfx_write_ply_mesh_attr(path, v.data(), n) : kfx_write_ply_attr(path, v.data(), n);
}
int kfx_save_pointcloud_attr(kfx_ctx *c, const char *path, int64_t cap) { return save_attr(c, path, cap, false); }
int kfx_save_mesh_attr(kfx_ctx *c, const char *path, int64_t cap) { return save_attr(c, path, cap, true); }

// ---- moving volume -------------------------------------------

// the checks kfx_shift_volume and kfx_evict_points share
static int shift_args(kfx_ctx *c, const int shift[3]) {
  if (!shift) return set_err(KFX_ERR_ARG, "null shift");
  for (int k = 0; k < 3; ++k)
    if (shift[k] % 8) return set_err(KFX_ERR_ARG, "shift components must be multiples of 8 voxels (whole bricks)");
  if (c->slab && c->world > 1)
    return set_err(KFX_ERR_STATE, "moving volume on one slab of several (a z shift would need an exchange)");
  return KFX_OK;
}

int kfx_shift_volume(kfx_ctx *c, const int shift[3]) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = shift_args(c, shift))) return r;
  if (!shift[0] && !shift[1] && !shift[2]) return KFX_OK;
  if ((r = make_events(c->ev_shift, 4))) return r;
  // the frames queued so far run at the old pose: captured graphs hold it as
  // a kernel argument, so they finish before the graphs are dropped
  HIPCHK(hipStreamSynchronize(c->pstream));
  HIPCHK(hipStreamSynchronize(c->stream));
  // the move, and with it the state an upload of the shifted records leaves:
  // both skip maps rebuilt from the new contents, no settled byte, the gate
  // open
  HIPCHK(hipEventRecord(c->ev_shift[2], c->stream));
  launch_shift(c->stream, c->vol, shift);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_shift[3], c->stream));
  c->shift_timed[1] = true;
  int o[3];
  for (int k = 0; k < 3; ++k) o[k] = c->origin[k] + shift[k];
  set_volume_origin(c, o);
  return KFX_OK;
}

int kfx_evict_points(kfx_ctx *c, const int shift[3], kfx_vertex *out, int64_t cap, int64_t *n) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = shift_args(c, shift))) return r;
  if (cap < 0 || (cap > 0 && !out)) return set_err(KFX_ERR_ARG, "bad point buffer");
  const DevPose vp = to_dev(c->p.volu_pose);
  return evict_items(
      c, "evict_points", c->ev_shift, &c->shift_timed[0], evict_units(c->vol, shift), sizeof(kfx_vertex), cap, out, n,
      [&](const ScanWs &w) { launch_evict(c->stream, c->vol, vp, shift, w.counts, nullptr, nullptr, 0); },
      [&](const ScanWs &w, const unsigned long long *, void *dst, unsigned long long m) {
        launch_evict(c->stream, c->vol, vp, shift, w.counts, w.offsets, (float *)dst, m);
      });
}

int kfx_get_volume_origin(kfx_ctx *c, int origin[3]) {
  int r = check_ctx(c);
  if (r) return r;
  if (!origin) return set_err(KFX_ERR_ARG, "null origin");
  for (int k = 0; k < 3; ++k) origin[k] = c->origin[k];
  return KFX_OK;
}

int kfx_get_volume_pose(kfx_ctx *c, kfx_pose *out) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out) return set_err(KFX_ERR_ARG, "null pose");
  *out = c->p.volu_pose;
  return KFX_OK;
}

int kfx_get_shift_ms(kfx_ctx *c, float out_ms[2]) { return timed_spans(c, c->ev_shift, c->shift_timed, out_ms); }

// ---- bricks out and back in ---------------------------------

int kfx_evict_bricks(kfx_ctx *c, const int shift[3], kfx_brick *out, int64_t cap, int64_t *n) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = shift_args(c, shift))) return r;
  if (cap < 0 || (cap > 0 && !out)) return set_err(KFX_ERR_ARG, "bad brick buffer");
  return evict_items(
      c, "evict_bricks", c->ev_stream, &c->stream_timed[0], brick_evict_units(c->vol, shift), sizeof(kfx_brick), cap, out, n,
      [&](const ScanWs &w) { launch_brick_count(c->stream, c->vol, shift, w.counts); },
      [&](const ScanWs &w, const unsigned long long *, void *dst, unsigned long long m) {
        launch_brick_emit(c->stream, c->vol, shift, c->origin, w.counts, w.offsets, dst, m);
      });
}

int kfx_restore_bricks(kfx_ctx *c, const kfx_brick *in, int64_t n, int64_t *n_restored) {
  int r = check_ctx(c);
  if (r) return r;
  if (n < 0 || (n > 0 && !in)) return set_err(KFX_ERR_ARG, "bad brick list");
  if (c->slab && c->world > 1)
    return set_err(KFX_ERR_STATE, "moving volume on one slab of several (a z shift would need an exchange)");
  // the host knows the origin: the bricks that land, and no two on one brick
  const int64_t nb[3] = {c->vol.tiles_x, c->vol.tiles_y, (c->vol.Z + 7) / 8};
  std::vector<uint64_t> cells;
  for (int64_t i = 0; i < n; ++i) {
    if (in[i].reserved != 0) return set_err(KFX_ERR_ARG, "restore_bricks: a reserved field that is not 0");
    int64_t q[3];
    bool inside = true;
    for (int k = 0; k < 3; ++k) {
      q[k] = (int64_t)in[i].b[k] - c->origin[k] / 8;
      inside = inside && q[k] >= 0 && q[k] < nb[k];
    }
    if (inside) cells.push_back((uint64_t)((q[2] * nb[1] + q[1]) * nb[0] + q[0]));
  }
  std::sort(cells.begin(), cells.end());
  if (std::adjacent_find(cells.begin(), cells.end()) != cells.end())
    return set_err(KFX_ERR_ARG, "restore_bricks: two bricks with the same coordinate inside the window");
  if (n_restored) *n_restored = (int64_t)cells.size();
  if (cells.empty()) return KFX_OK;  // no device work; the settled bytes stay
  if ((r = make_events(c->ev_stream, 4))) return r;
  // behind every queued frame, as the shift; the captured graphs hold neither
  // the volume's contents nor its maps and stay
  HIPCHK(hipStreamSynchronize(c->pstream));
  HIPCHK(hipStreamSynchronize(c->stream));
  void *din = nullptr;
  if (hipMalloc(&din, (size_t)n * sizeof(kfx_brick)) != hipSuccess)
    return set_err(KFX_ERR_OOM, "restore_bricks: hipMalloc(" + std::to_string((size_t)n * sizeof(kfx_brick)) + ")");
  hipError_t e = hipMemcpyAsync(din, in, (size_t)n * sizeof(kfx_brick), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipEventRecord(c->ev_stream[2], c->stream);
  if (e == hipSuccess) {
    launch_brick_restore(c->stream, c->vol, c->origin, din, (size_t)n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(c->ev_stream[3], c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(din);
  if (e != hipSuccess) return set_err(KFX_ERR_HIP, std::string("restore_bricks: ") + hipGetErrorString(e));
  c->stream_timed[1] = true;
  return KFX_OK;
}

int kfx_get_stream_ms(kfx_ctx *c, float out_ms[2]) { return timed_spans(c, c->ev_stream, c->stream_timed, out_ms); }

// ---- world map -------------------------------------------------

// the list checks kfx_world_points_attr and kfx_world_mesh_attr share
static int world_args(kfx_ctx *c, const kfx_brick *bricks, int64_t n, const void *out, int64_t cap) {
  if (n < 0 || (n > 0 && !bricks)) return set_err(KFX_ERR_ARG, "bad brick list");
  if (cap < 0 || (cap > 0 && !out)) return set_err(KFX_ERR_ARG, "bad item buffer");
  if (c->slab && c->world > 1)
    return set_err(KFX_ERR_STATE, "moving volume on one slab of several (a z shift would need an exchange)");
  for (int64_t i = 0; i < n; ++i) {
    const kfx_brick &b = bricks[i];
    if (b.reserved != 0) return set_err(KFX_ERR_ARG, "world: a reserved field that is not 0");
    for (int k = 0; k < 3; ++k)
      if (b.b[k] <= -(1 << 20) || b.b[k] >= (1 << 20))
        return set_err(KFX_ERR_ARG, "world: a brick coordinate outside (-2^20, 2^20)");
    if (i > 0) {
      const kfx_brick &a = bricks[i - 1];
      const bool up = a.b[2] != b.b[2] ? a.b[2] < b.b[2] : (a.b[1] != b.b[1] ? a.b[1] < b.b[1] : a.b[0] < b.b[0]);
      if (!up) return set_err(KFX_ERR_ARG, "world: the bricks must ascend strictly in (b[2], b[1], b[0])");
    }
  }
  return KFX_OK;
}

// kfx_world_points_attr / kfx_world_mesh_attr: `out` holds cap items of 1 / 3 kfx_vertex
static int world_items(kfx_ctx *c, const kfx_brick *bricks, int64_t n, bool mesh, kfx_vertex *out, int64_t cap,
                       int64_t *n_items) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = world_args(c, bricks, n, out, cap))) return r;
  for (float &m : c->world_ms) m = 0.f;
  if (n == 0) {  // no device work
    if (n_items) *n_items = 0;
    return KFX_OK;
  }
  if (n > ((int64_t)1 << 28)) return set_err(KFX_ERR_OOM, "world: more bricks than the record buffer can hold");
  if ((r = make_events(c->ev_world, 5))) return r;
  if (mesh && (r = ensure_mc_table(c))) return r;
  // the buffers the context keeps (grown on demand; the previous call has
  // completed): [0] records, [1] keys, [2] neighbour table, [3] scan workspace, [4] items
  const size_t nn = (size_t)n;
  void **buf = c->world_buf;
  size_t *bcap = c->world_cap;
  ScanWs w;
  if ((r = reserve(&buf[0], &bcap[0], nn * sizeof(kfx_brick), "world")) || (r = reserve(&buf[1], &bcap[1], nn * 8, "world")) ||
      (r = reserve(&buf[2], &bcap[2], nn * 27 * 4, "world")) || (r = scan_workspace(&buf[3], &bcap[3], nn, 0, "world", &w)))
    return r;
  unsigned long long *keys = (unsigned long long *)buf[1];
  int32_t *neigh = (int32_t *)buf[2];
  const uint8_t *tab = mesh ? c->mc_tab : nullptr;
  const DevPose p0 = to_dev(c->volu_pose0);  // (R0, t0): a voxel's position does not depend on where the window stands
  hipStream_t s = c->stream;                 // behind every queued frame
  HIPCHK(hipMemcpyAsync(buf[0], bricks, nn * sizeof(kfx_brick), hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(c->ev_world[0], s));
  launch_world_neigh(s, buf[0], nn, keys, neigh);
  // table [0, 1], count + scan [1, 2], emit [3, 4]
  const ScanEvents marks = {c->ev_world[1], nullptr, c->ev_world[2], c->ev_world[3], c->ev_world[4]};
  int64_t total = 0;
  r = count_scan_emit(
      c, "world", w, nn, (mesh ? 3 : 1) * sizeof(kfx_vertex), cap, out, &buf[4], &bcap[4], marks,
      [&](const ScanWs &w) {
        launch_world_sweep(s, buf[0], nn, neigh, p0, c->vol.vs, tab, w.counts, nullptr, nullptr, 0);
      },
      [&](const ScanWs &w, const unsigned long long *, void *dst, unsigned long long m) {
        launch_world_sweep(s, buf[0], nn, neigh, p0, c->vol.vs, tab, w.counts, w.offsets, (float *)dst, m);
      },
      &total);
  if (r) return r;
  if (std::min(total, cap) > 0) HIPCHK(hipEventElapsedTime(&c->world_ms[2], c->ev_world[3], c->ev_world[4]));
  HIPCHK(hipEventElapsedTime(&c->world_ms[0], c->ev_world[0], c->ev_world[1]));
  HIPCHK(hipEventElapsedTime(&c->world_ms[1], c->ev_world[1], c->ev_world[2]));
  if (n_items) *n_items = total;
  return KFX_OK;
}

int kfx_world_points_attr(kfx_ctx *c, const kfx_brick *bricks, int64_t n, kfx_vertex *out, int64_t cap,
                          int64_t *n_points) {
  return world_items(c, bricks, n, false, out, cap, n_points);
}
int kfx_world_mesh_attr(kfx_ctx *c, const kfx_brick *bricks, int64_t n, kfx_vertex *out, int64_t cap_tris,
                        int64_t *n_tris) {
  return world_items(c, bricks, n, true, out, cap_tris, n_tris);
}

int kfx_get_world_ms(kfx_ctx *c, float out_ms[3]) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out_ms) return set_err(KFX_ERR_ARG, "null ms");
  for (int k = 0; k < 3; ++k) out_ms[k] = c->world_ms[k];
  return KFX_OK;
}

int kfx_world_bricks(kfx_ctx *c, const kfx_brick_store *store, kfx_brick *out, int64_t cap, int64_t *n) {
  int r = check_ctx(c);
  if (r) return r;
  if (!n) return set_err(KFX_ERR_ARG, "null count");
  if (cap < 0 || (cap > 0 && !out)) return set_err(KFX_ERR_ARG, "bad brick buffer");
  // the window's non-empty bricks: what a shift that drops everything evicts
  const int all[3] = {(c->vol.X + 7) / 8 * 8, 0, 0};
  int64_t nw = 0;
  if ((r = kfx_evict_bricks(c, all, nullptr, 0, &nw))) return r;
  std::vector<kfx_brick> win;
  try {
    win.resize((size_t)nw);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "world_bricks: out of memory");
  }
  if (nw > 0 && (r = kfx_evict_bricks(c, all, win.data(), nw, &nw))) return r;
  *n = brick_store_merge(store, win.data(), nw, nullptr);
  if (cap < *n) return KFX_OK;  // nothing written: size the buffer and call again
  (void)brick_store_merge(store, win.data(), nw, out);
  return KFX_OK;
}

int kfx_save_world_mesh(kfx_ctx *c, const kfx_brick_store *store, const char *path, int64_t cap) {
  if (!path) return set_err(KFX_ERR_ARG, "null path");
  if (cap <= 0) cap = KFX_DEFAULT_CLOUD_POINTS;
  int64_t nb = 0, total = 0;
  int r = kfx_world_bricks(c, store, nullptr, 0, &nb);
  if (r) return r;
  std::vector<kfx_brick> bricks;
  std::vector<kfx_vertex> v;
  try {
    bricks.resize((size_t)nb);
    if (nb > 0 && (r = kfx_world_bricks(c, store, bricks.data(), nb, &nb))) return r;
    if ((r = kfx_world_mesh_attr(c, bricks.data(), nb, nullptr, 0, &total))) return r;
    v.resize((size_t)std::min(total, cap) * 3);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "save_world_mesh: out of memory");
  }
  const int64_t m = std::min(total, cap);
  if (m > 0 && (r = kfx_world_mesh_attr(c, bricks.data(), nb, v.data(), m, &total))) return r;
  return kfx_write_ply_mesh_attr(path, v.data(), m);
}

// ---- indexed mesh ----------------------------------------------

// the buffer checks both forms share
static int indexed_args(const kfx_vertex *verts, int64_t cap_verts, const uint32_t *tris, int64_t cap_tris,
                        const int64_t *n_verts, const int64_t *n_tris) {
  if (!n_verts || !n_tris) return set_err(KFX_ERR_ARG, "indexed mesh: null count");
  if (cap_verts < 0 || (cap_verts > 0 && !verts)) return set_err(KFX_ERR_ARG, "bad vertex buffer");
  if (cap_tris < 0 || (cap_tris > 0 && !tris)) return set_err(KFX_ERR_ARG, "bad index buffer");
  return KFX_OK;
}

int kfx_extract_mesh_indexed(kfx_ctx *c, kfx_vertex *verts, int64_t cap_verts, uint32_t *tris, int64_t cap_tris,
                             int64_t *n_verts, int64_t *n_tris) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = indexed_args(verts, cap_verts, tris, cap_tris, n_verts, n_tris))) return r;
  if (c->slab && c->world > 1)
    return set_err(KFX_ERR_STATE, "indexed mesh on one slab of several (a seam's vertices would need renumbering)");
  HIPCHK(hipStreamSynchronize(c->stream));
  if ((r = ensure_mc_table(c)) || (r = make_events(c->ev_indexed, 6))) return r;
  for (float &m : c->indexed_ms) m = 0.f;
  const DevPose vp = to_dev(c->p.volu_pose);
  CallBuf ws, vbuf, tbuf;
  return indexed_run(c, "extract_mesh_indexed", indexed_units(c->vol), &ws.p, &ws.cap, &vbuf.p, &vbuf.cap, &tbuf.p,
                     &tbuf.cap, verts, cap_verts, tris, cap_tris, n_verts, n_tris,
                     [&](int which, const ScanWs &wv, const ScanWs &wt, void *dv, uint16_t *keys, uint32_t *dt) {
                       launch_indexed(c->stream, c->vol, vp, c->mc_tab, which, wv.counts, wt.counts, wv.offsets,
                                      wt.offsets, dv, keys, dt);
                     });
}

int kfx_world_mesh_indexed(kfx_ctx *c, const kfx_brick *bricks, int64_t n, kfx_vertex *verts, int64_t cap_verts,
                           uint32_t *tris, int64_t cap_tris, int64_t *n_verts, int64_t *n_tris) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = indexed_args(verts, cap_verts, tris, cap_tris, n_verts, n_tris))) return r;
  if ((r = world_args(c, bricks, n, verts, cap_verts))) return r;
  for (float &m : c->indexed_ms) m = 0.f;
  if (n == 0) {  // no device work
    *n_verts = *n_tris = 0;
    return KFX_OK;
  }
  if (n > ((int64_t)1 << 28)) return set_err(KFX_ERR_OOM, "world: more bricks than the record buffer can hold");
  if ((r = make_events(c->ev_indexed, 6)) || (r = ensure_mc_table(c))) return r;
  // kfx_world_mesh_attr's buffers: [0] records, [1] keys, [2] neighbour table, [3] the scan workspaces,
  // [4] vertices and their keys; the face list has its own
  const size_t nn = (size_t)n;
  void **buf = c->world_buf;
  size_t *bcap = c->world_cap;
  if ((r = reserve(&buf[0], &bcap[0], nn * sizeof(kfx_brick), "world")) || (r = reserve(&buf[1], &bcap[1], nn * 8, "world")) ||
      (r = reserve(&buf[2], &bcap[2], nn * 27 * 4, "world")))
    return r;
  int32_t *neigh = (int32_t *)buf[2];
  const DevPose p0 = to_dev(c->volu_pose0);
  hipStream_t s = c->stream;  // behind every queued frame
  HIPCHK(hipMemcpyAsync(buf[0], bricks, nn * sizeof(kfx_brick), hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(c->ev_indexed[0], s));
  launch_world_neigh(s, buf[0], nn, (unsigned long long *)buf[1], neigh);
  r = indexed_run(c, "world_mesh_indexed", nn, &buf[3], &bcap[3], &buf[4], &bcap[4], &c->world_tris, &c->world_tris_cap,
                  verts, cap_verts, tris, cap_tris, n_verts, n_tris,
                  [&](int which, const ScanWs &wv, const ScanWs &wt, void *dv, uint16_t *keys, uint32_t *dt) {
                    launch_world_indexed(s, buf[0], nn, neigh, p0, c->vol.vs, c->mc_tab, which, wv.counts, wt.counts,
                                         wv.offsets, wt.offsets, dv, keys, dt);
                  });
  if (r) return r;
  HIPCHK(hipEventElapsedTime(&c->indexed_ms[0], c->ev_indexed[0], c->ev_indexed[1]));
  return KFX_OK;
}

int kfx_get_indexed_ms(kfx_ctx *c, float out_ms[4]) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out_ms) return set_err(KFX_ERR_ARG, "null ms");
  for (int k = 0; k < 4; ++k) out_ms[k] = c->indexed_ms[k];
  return KFX_OK;
}

int kfx_write_ply_mesh_indexed(const char *path, const kfx_vertex *verts, int64_t n_verts, const uint32_t *tris,
                               int64_t n_tris) {
  if (!path || n_verts < 0 || n_tris < 0 || (n_verts > 0 && !verts) || (n_tris > 0 && !tris))
    return set_err(KFX_ERR_ARG, "bad argument");
  for (int64_t i = 0; i < 3 * n_tris; ++i)  // before the file exists: none is left behind
    if ((int64_t)tris[i] >= n_verts) return set_err(KFX_ERR_ARG, "write_ply_mesh_indexed: an index past the vertex list");
  FILE *f = std::fopen(path, "w");
  if (!f) return set_err(KFX_ERR_ARG, std::string("cannot open ") + path);
  std::fprintf(f, "ply\nformat ascii 1.0\nelement vertex %lld\n%s"
               "element face %lld\nproperty list uchar int vertex_indices\nend_header\n",
               (long long)n_verts, kPlyAttrProps, (long long)n_tris);
  ply_attr_vertices(f, verts, n_verts);
  for (int64_t i = 0; i < n_tris; ++i)
    std::fprintf(f, "3 %u %u %u\n", tris[3 * i], tris[3 * i + 1], tris[3 * i + 2]);
  std::fclose(f);
  return KFX_OK;
}

int kfx_save_mesh_indexed(kfx_ctx *c, const char *path) {
  if (!path) return set_err(KFX_ERR_ARG, "null path");
  return save_indexed(path, "save_mesh_indexed", [&](kfx_vertex *v, int64_t cv, uint32_t *t, int64_t ct, int64_t *nv, int64_t *nt) {
    return kfx_extract_mesh_indexed(c, v, cv, t, ct, nv, nt);
  });
}

int kfx_save_world_mesh_indexed(kfx_ctx *c, const kfx_brick_store *store, const char *path) {
  if (!path) return set_err(KFX_ERR_ARG, "null path");
  int64_t nb = 0;
  int r = kfx_world_bricks(c, store, nullptr, 0, &nb);
  if (r) return r;
  std::vector<kfx_brick> bricks;
  try {
    bricks.resize((size_t)nb);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "save_world_mesh_indexed: out of memory");
  }
  if (nb > 0 && (r = kfx_world_bricks(c, store, bricks.data(), nb, &nb))) return r;
  return save_indexed(path, "save_world_mesh_indexed",
                      [&](kfx_vertex *v, int64_t cv, uint32_t *t, int64_t ct, int64_t *nv, int64_t *nt) {
                        return kfx_world_mesh_indexed(c, bricks.data(), nb, v, cv, t, ct, nv, nt);
                      });
}

// ---- world view ----------------------------------------------------

int kfx_world_view_load(kfx_ctx *c, const kfx_brick *bricks, int64_t n, const int origin[3], const int dims[3]) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = world_args(c, bricks, n, nullptr, 0))) return r;
  if ((origin == nullptr) != (dims == nullptr)) return set_err(KFX_ERR_ARG, "world_view_load: origin and dims go together");
  if (n > ((int64_t)1 << 28)) return set_err(KFX_ERR_OOM, "world: more bricks than the record buffer can hold");
  if (n == 0) {  // unload (the buffers stay for the next world)
    c->wv_n = 0;
    c->wv_ms[0] = 0.f;
    return KFX_OK;
  }
  int64_t o[3], d[3];
  if (origin) {
    for (int k = 0; k < 3; ++k) o[k] = origin[k], d[k] = dims[k];
  } else {  // the list's bounding box in bricks, one brick of padding on every side
    int64_t lo[3], hi[3];
    for (int k = 0; k < 3; ++k) lo[k] = hi[k] = bricks[0].b[k];
    for (int64_t i = 1; i < n; ++i)
      for (int k = 0; k < 3; ++k) {
        lo[k] = std::min<int64_t>(lo[k], bricks[i].b[k]);
        hi[k] = std::max<int64_t>(hi[k], bricks[i].b[k]);
      }
    for (int k = 0; k < 3; ++k) o[k] = 8 * (lo[k] - 1), d[k] = 8 * (hi[k] - lo[k] + 3);
  }
  int64_t nb[3];
  for (int k = 0; k < 3; ++k) {
    if (o[k] % 8) return set_err(KFX_ERR_ARG, "world_view_load: origin components must be multiples of 8 voxels");
    if (o[k] <= -((int64_t)1 << 23) || o[k] >= ((int64_t)1 << 23))
      return set_err(KFX_ERR_ARG, "world_view_load: an origin component outside (-2^23, 2^23)");
    if (d[k] < 1 || d[k] > (1 << 15)) return set_err(KFX_ERR_ARG, "world_view_load: a dims component outside 1..2^15");
    nb[k] = (d[k] + 7) / 8;
  }
  if (nb[0] * nb[1] * nb[2] > ((int64_t)1 << 26)) return set_err(KFX_ERR_ARG, "world_view_load: a box of more than 2^26 bricks");
  // the box as a volume: make_vol's map extents for a whole volume of these dims
  VolView v{};
  v.X = (int)d[0], v.Y = (int)d[1], v.Z = (int)d[2];
  v.zb = 0, v.zn = v.Z, v.own0 = 0, v.own1 = v.Z;
  v.tiles_x = (int)nb[0], v.tiles_y = (int)nb[1];
  v.slice = (size_t)v.X * v.Y;
  v.bz0 = 0, v.nbz = (int)nb[2], v.bw = (v.nbz + 63) / 64;
  v.sz0 = 0, v.nsz = ((v.Z - 1) >> 5) + 1, v.sw = (v.nsz + 31) / 32;
  v.stx = (v.tiles_x + 3) / 4, v.sty = (v.tiles_y + 3) / 4;
  for (int k = 0; k < 3; ++k) {
    v.vs[k] = c->vol.vs[k];
    v.range[k] = d[k] == c->p.volu_dims[k] ? c->p.volu_range[k] : (float)d[k] * v.vs[k];
  }
  v.trunc = c->vol.trunc, v.inv_trunc = c->vol.inv_trunc;
  const size_t nn = (size_t)n, cells = (size_t)(nb[0] * nb[1] * nb[2]);
  if ((r = make_events(c->ev_wv, 4))) return r;
  // from here on the previous world is gone (its buffers are reused)
  c->wv_n = 0;
  void **buf = c->wv_buf;
  size_t *bcap = c->wv_cap;
  if ((r = reserve(&buf[0], &bcap[0], nn * sizeof(kfx_brick), "world_view_load")) ||
      (r = reserve(&buf[1], &bcap[1], cells * 4, "world_view_load")) ||
      (r = reserve(&buf[2], &bcap[2], v.bocc_bytes(), "world_view_load")) ||
      (r = reserve(&buf[3], &bcap[3], v.socc_bytes(), "world_view_load")))
    return r;
  v.bocc = (unsigned long long *)buf[2];
  v.socc = (uint32_t *)buf[3];
  const WorldGrid wg = {buf[0], (uint32_t *)buf[1], nn, cells};
  const int oi[3] = {(int)o[0], (int)o[1], (int)o[2]};
  hipStream_t s = c->stream;  // behind every queued frame, as kfx_world_mesh_attr
  HIPCHK(hipMemcpyAsync(buf[0], bricks, nn * sizeof(kfx_brick), hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(c->ev_wv[0], s));
  launch_world_view_load(s, v, wg, oi);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_wv[1], s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipEventElapsedTime(&c->wv_ms[0], c->ev_wv[0], c->ev_wv[1]));
  // the box's pose: kfx_shift_volume's formula at this origin (set_volume_origin)
  const kfx_pose &p0 = c->volu_pose0;
  float dd[3];
  for (int k = 0; k < 3; ++k) dd[k] = (float)oi[k] * v.vs[k];
  c->wv_pose = to_dev(p0);
  for (int i = 0; i < 3; ++i) {
    const float a = p0.R[3 * i] * dd[0], b = p0.R[3 * i + 1] * dd[1], e = p0.R[3 * i + 2] * dd[2];
    const float sum = (a + b) + e;
    c->wv_pose.t[i] = p0.t[i] + sum;
  }
  c->wv_vol = v;
  c->wv_cells = cells;
  for (int k = 0; k < 3; ++k) c->wv_origin[k] = oi[k];
  c->wv_n = nn;
  return KFX_OK;
}

int kfx_world_view(kfx_ctx *c, const kfx_intrinsics *view, const kfx_pose *cam_pose, int type, uint8_t *out, float *vmap,
                   float *nmap, float *ts) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = view_args(view, cam_pose, out, type))) return r;
  if (c->slab && c->world > 1) return set_err(KFX_ERR_STATE, "world_view on one slab of several");
  if (c->wv_n == 0) return set_err(KFX_ERR_STATE, "world_view: no world is loaded (kfx_world_view_load)");
  VolView v = c->wv_vol;
  v.force64 = c->vol.force64;
  const WorldGrid wg = {c->wv_buf[0], (uint32_t *)c->wv_buf[1], c->wv_n, c->wv_cells};
  // it reads the loaded world only; ev_wv[0..1] are the load's
  return view_run(c, "world_view", c->ev_wv + 2, &c->wv_ms[1], c->wv_pose, view, cam_pose, out, vmap, nmap, ts,
                  [&](const LevelGeom &g, const DevPose &c2v, const float *eye, float *dv, float *dn, float *dt) {
                    launch_world_view(c->stream, v, wg, g, c2v, eye, type, c->view_out, dv, dn, dt);
                  });
}

int kfx_get_world_view_ms(kfx_ctx *c, float out_ms[2]) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out_ms) return set_err(KFX_ERR_ARG, "null ms");
  out_ms[0] = c->wv_ms[0];
  out_ms[1] = c->wv_ms[1];
  return KFX_OK;
}

int kfx_save_world_view(kfx_ctx *c, const kfx_brick_store *store, const kfx_intrinsics *view, const kfx_pose *cam_pose,
                        int type, const char *path) {
  if (!path) return set_err(KFX_ERR_ARG, "null path");
  int r = view_size(view);
  if (r) return r;
  int64_t nb = 0;
  if ((r = kfx_world_bricks(c, store, nullptr, 0, &nb))) return r;
  std::vector<kfx_brick> bricks;
  std::vector<uint8_t> img;
  try {
    bricks.resize((size_t)nb);
    img.assign(3 * (size_t)view->width * view->height, 0);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "save_world_view: out of memory");
  }
  if (nb > 0 && (r = kfx_world_bricks(c, store, bricks.data(), nb, &nb))) return r;
  if ((r = kfx_world_view_load(c, bricks.data(), nb, nullptr, nullptr))) return r;
  // an empty world is an empty image (nothing is loaded then)
  if (nb > 0 && (r = kfx_world_view(c, view, cam_pose, type, img.data(), nullptr, nullptr, nullptr))) return r;
  return kfx_write_ppm(path, img.data(), view->width, view->height);
}

int kfx_shift_for_pose(const kfx_params *p, const kfx_pose *vp, const kfx_pose *cam, float ahead_m, int shift[3]) {
  if (!p || !vp || !cam || !shift) return set_err(KFX_ERR_ARG, "null argument");
  if (!std::isfinite(ahead_m) || ahead_m < 0.f) return set_err(KFX_ERR_ARG, "ahead_m must be finite and >= 0");
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(i < 9 ? vp->R[i] : vp->t[i - 9]) || !std::isfinite(i < 9 ? cam->R[i] : cam->t[i - 9]))
      return set_err(KFX_ERR_ARG, "non-finite pose entry");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(p->volu_range[k]) || p->volu_range[k] <= 0.f || p->volu_dims[k] < 1)
      return set_err(KFX_ERR_ARG, "volume range and dims must be positive");
  double cw[3], q[3];
  for (int i = 0; i < 3; ++i) cw[i] = (double)cam->R[3 * i + 2] * (double)ahead_m + (double)cam->t[i];
  for (int j = 0; j < 3; ++j) {  // q = R_v^T (c - t_v)
    q[j] = 0.0;
    for (int i = 0; i < 3; ++i) q[j] += (double)vp->R[3 * i + j] * (cw[i] - (double)vp->t[i]);
  }
  for (int k = 0; k < 3; ++k) {
    const double vs = (double)p->volu_range[k] / (double)p->volu_dims[k];
    shift[k] = 8 * (int)std::lround(((q[k] - (double)p->volu_range[k] / 2.0) / vs) / 8.0);
  }
  return KFX_OK;
}

// ---- ICP residuals and quality records ---------------------

// n poses of CUR level `level` against the model maps (pv, pn): the records,
// and for one pose the per-pixel outcome.  On the frame stream behind every
// queued frame; only q_buf is written; the pending tracking status is left
// alone.  ev_q[2, 3] time the launch.
static int quality_run(kfx_ctx *c, int level, const float *pv, const float *pn, const kfx_pose *poses, int64_t n,
                       float *residual, uint8_t *label, kfx_icp_quality *out) {
  int r;
  const LevelGeom &g = c->g[level];
  const size_t np = (size_t)g.w * g.h;
  const bool store = residual || label;
  if ((r = reserve(&c->q_buf[0], &c->q_cap[0], sizeof(DevPose) * (size_t)n, "quality"))) return r;
  if ((r = reserve(&c->q_buf[1], &c->q_cap[1], sizeof(kfx_icp_quality) * (size_t)n, "quality"))) return r;
  if (store && (r = reserve(&c->q_buf[2], &c->q_cap[2], 4 * np, "quality"))) return r;
  if (store && (r = reserve(&c->q_buf[3], &c->q_cap[3], (np + 3) & ~(size_t)3, "quality"))) return r;
  if ((r = make_events(c->ev_q, 4))) return r;
  std::vector<DevPose> dp;
  std::vector<kfx_icp_quality> rec;
  try {
    dp.resize((size_t)n);
    rec.resize((size_t)n);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "quality: out of memory");
  }
  for (int64_t k = 0; k < n; ++k) dp[(size_t)k] = to_dev(poses[k]);
  HIPCHK(hipMemcpyAsync(c->q_buf[0], dp.data(), sizeof(DevPose) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(c->q_buf[1], 0, sizeof(kfx_icp_quality) * (size_t)n, c->stream));
  HIPCHK(hipEventRecord(c->ev_q[2], c->stream));
  launch_quality(c->stream, g, c->cur.v[level], c->cur.n[level], pv, pn, c->p.icp_dist_threshold, c->angle_thr,
                 static_cast<const DevPose *>(c->q_buf[0]), (int)n, c->q_buf[1], store ? (float *)c->q_buf[2] : nullptr,
                 store ? (uint8_t *)c->q_buf[3] : nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_q[3], c->stream));
  HIPCHK(hipMemcpyAsync(rec.data(), c->q_buf[1], sizeof(kfx_icp_quality) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  if (residual) HIPCHK(hipMemcpyAsync(residual, c->q_buf[2], 4 * np, hipMemcpyDeviceToHost, c->stream));
  if (label) HIPCHK(hipMemcpyAsync(label, c->q_buf[3], np, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipEventElapsedTime(&c->q_ms[0], c->ev_q[2], c->ev_q[3]));
  if (out)
    for (int64_t k = 0; k < n; ++k) {
      out[k] = rec[(size_t)k];
      out[k].level = level;
    }
  return KFX_OK;
}

static int quality_args(kfx_ctx *c, int level, const void *a, const void *b, const void *q) {
  if (level < 0 || level >= c->L) return set_err(KFX_ERR_ARG, "level outside 0..L-1");
  if (!a && !b && !q) return set_err(KFX_ERR_ARG, "residual, label and record all null");
  return KFX_OK;
}

int kfx_stage_icp_residuals(kfx_ctx *c, int level, const kfx_pose *pose, float *residual, uint8_t *label,
                            kfx_icp_quality *q) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = quality_args(c, level, residual, label, q))) return r;
  if (!pose) return set_err(KFX_ERR_ARG, "null pose");
  c->q_ms[1] = 0.f;
  return quality_run(c, level, c->prev.v[level], c->prev.n[level], pose, 1, residual, label, q);
}

int kfx_frame_quality(kfx_ctx *c, int level, float *residual, uint8_t *label, kfx_icp_quality *q) {
  const kfx_pose id = {{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}};
  return kfx_stage_icp_residuals(c, level, &id, residual, label, q);
}

int kfx_score_poses(kfx_ctx *c, int level, const kfx_pose *poses, int64_t n, kfx_icp_quality *out) {
  int r = check_ctx(c);
  if (r) return r;
  if (level < 0 || level >= c->L) return set_err(KFX_ERR_ARG, "level outside 0..L-1");
  if (n < 0 || n > 65536) return set_err(KFX_ERR_ARG, "n outside 0..2^16");
  if (n == 0) return KFX_OK;
  if (!poses || !out) return set_err(KFX_ERR_ARG, "null argument");
  for (int64_t k = 0; k < n; ++k)
    for (int i = 0; i < 12; ++i)
      if (!std::isfinite(i < 9 ? poses[k].R[i] : poses[k].t[i - 9])) return set_err(KFX_ERR_ARG, "non-finite pose entry");
  c->q_ms[1] = 0.f;
  return quality_run(c, level, c->prev.v[level], c->prev.n[level], poses, n, nullptr, nullptr, out);
}

int kfx_quality_chunk(int width, int height, int64_t n) {
  if (width < 1 || height < 1 || n < 1 || (int64_t)width * height > ((int64_t)1 << 26))
    return set_err(KFX_ERR_ARG, "quality_chunk: width, height, n >= 1 and width * height <= 2^26");
  return quality_chunk(width, height, n);
}

int kfx_score_view(kfx_ctx *c, int level, const kfx_pose *cam_pose, float *residual, uint8_t *label,
                   kfx_icp_quality *q) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = quality_args(c, level, residual, label, q))) return r;
  if (!cam_pose) return set_err(KFX_ERR_ARG, "null pose");
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(i < 9 ? cam_pose->R[i] : cam_pose->t[i - 9])) return set_err(KFX_ERR_ARG, "non-finite view pose");
  if (c->slab && c->world > 1) return set_err(KFX_ERR_STATE, "score_view on one slab of several");
  const LevelGeom &g = c->g[level];
  const size_t np = (size_t)g.w * g.h;
  // [vmap | nmap | the view's image (k_view always stores one)]
  if ((r = reserve(&c->q_buf[4], &c->q_cap[4], 27 * np, "score_view"))) return r;
  if ((r = make_events(c->ev_q, 4))) return r;
  float *dv = static_cast<float *>(c->q_buf[4]), *dn = dv + 3 * np;
  const DevPose cam = to_dev(*cam_pose);
  const DevPose c2v = host_pose_mul(host_pose_inv(to_dev(c->p.volu_pose)), cam);  // kfx_render_view's pose
  HIPCHK(hipEventRecord(c->ev_q[0], c->stream));
  launch_view(c->stream, c->vol, g, c2v, cam.t, KFX_VIEW_NORMAL, reinterpret_cast<uint8_t *>(dn + 3 * np), dv, dn,
              nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_q[1], c->stream));
  const kfx_pose id = {{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}};
  if ((r = quality_run(c, level, dv, dn, &id, 1, residual, label, q))) return r;
  HIPCHK(hipEventElapsedTime(&c->q_ms[1], c->ev_q[0], c->ev_q[1]));
  return KFX_OK;
}

int kfx_get_quality_ms(kfx_ctx *c, float out_ms[2]) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out_ms) return set_err(KFX_ERR_ARG, "null ms");
  out_ms[0] = c->q_ms[0];
  out_ms[1] = c->q_ms[1];
  return KFX_OK;
}

int kfx_quality_figures(const kfx_icp_quality *q, double *fitness, double *rmse) {
  if (!q || !fitness || !rmse) return set_err(KFX_ERR_ARG, "null argument");
  for (int k = 0; k < 6; ++k)
    if (q->n[k] < 0) return set_err(KFX_ERR_ARG, "negative count");
  const int64_t den = q->n[0] + q->n[2] + q->n[3] + q->n[4];
  *fitness = den ? (double)q->n[0] / (double)den : 0.0;
  *rmse = q->n[0] ? std::sqrt(((double)q->sum_r2 / 4294967296.0) / (double)q->n[0]) : 0.0;
  return KFX_OK;
}

// ---- multi-start ICP ----------------------------------------

static_assert(sizeof(IcpMultiPose) == sizeof(kfx_icp_result) && offsetof(IcpMultiPose, x) == offsetof(kfx_icp_result, x) &&
                  offsetof(IcpMultiPose, fail) == offsetof(kfx_icp_result, status),
              "the device record is the public one");

// the argument checks kfx_icp_multi and kfx_track_view share (n > 0 behind them)
static int multi_args(const kfx_pose *starts, int64_t n, const kfx_icp_result *out) {
  if (n < 0 || n > 65536) return set_err(KFX_ERR_ARG, "n outside 0..2^16");
  if (n == 0) return KFX_OK;
  if (!starts || !out) return set_err(KFX_ERR_ARG, "null argument");
  for (int64_t k = 0; k < n; ++k)
    for (int i = 0; i < 12; ++i)
      if (!std::isfinite(i < 9 ? starts[k].R[i] : starts[k].t[i - 9])) return set_err(KFX_ERR_ARG, "non-finite pose entry");
  return KFX_OK;
}

// ICPRegistration::rigidTransform's loop from each of n starts, CUR against the
// model maps (pv, pn) of every level: one launch per (level, iteration).  On
// the frame stream behind every queued frame; only m_buf[0, 1] are written; the
// pending tracking status is left alone.  ev_m[2, 3] time the launches.  With
// q, the poses reached are scored at level 0 on the same maps (quality_run;
// kfx_get_quality_ms reads as before).
static int multi_run(kfx_ctx *c, const float *const *pv, const float *const *pn, const kfx_pose *starts, int64_t n,
                     kfx_icp_result *out, kfx_icp_quality *q) {
  int r;
  const size_t rows = sizeof(unsigned long long) * 27 * (size_t)n;
  if ((r = reserve(&c->m_buf[0], &c->m_cap[0], sizeof(IcpMultiPose) * (size_t)n, "icp_multi"))) return r;
  if ((r = reserve(&c->m_buf[1], &c->m_cap[1], rows + sizeof(unsigned) * (size_t)n, "icp_multi"))) return r;
  if ((r = make_events(c->ev_m, 4))) return r;
  std::vector<IcpMultiPose> mp;
  try {
    mp.resize((size_t)n);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "icp_multi: out of memory");
  }
  for (int64_t k = 0; k < n; ++k) {
    IcpMultiPose &m = mp[(size_t)k];
    std::memset(&m, 0, sizeof(m));
    m.pose = to_dev(starts[k]);
    m.stop_level = m.stop_iter = -1;
  }
  IcpMultiPose *dp = static_cast<IcpMultiPose *>(c->m_buf[0]);
  unsigned long long *drows = static_cast<unsigned long long *>(c->m_buf[1]);
  unsigned *dtick = reinterpret_cast<unsigned *>(drows + 27 * (size_t)n);
  HIPCHK(hipMemcpyAsync(dp, mp.data(), sizeof(IcpMultiPose) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(drows, 0, rows + sizeof(unsigned) * (size_t)n, c->stream));
  HIPCHK(hipEventRecord(c->ev_m[2], c->stream));
  for (int level = c->L - 1; level >= 0; --level)
    for (int it = 0; it < c->p.icp_iter_count[level]; ++it)
      launch_icp_multi(c->stream, c->g[level], c->cur.v[level], c->cur.n[level], pv[level], pn[level],
                       c->p.icp_dist_threshold, c->angle_thr, dp, (int)n, drows, dtick, level, it);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_m[3], c->stream));
  HIPCHK(hipMemcpyAsync(mp.data(), dp, sizeof(IcpMultiPose) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipEventElapsedTime(&c->m_ms[1], c->ev_m[2], c->ev_m[3]));
  c->m_ms[2] = 0.f;
  for (int64_t k = 0; k < n; ++k) {
    const IcpMultiPose &m = mp[(size_t)k];
    kfx_icp_result &o = out[k];
    o.pose = to_api(m.pose);
    o.status = m.fail ? KFX_TRACKING_LOST : KFX_OK;
    o.stop_level = m.stop_level;
    o.stop_iter = m.stop_iter;
    o.solves = m.solves;
    std::memcpy(o.x, m.x, sizeof(o.x));
  }
  if (q) {
    std::vector<kfx_pose> reached;
    try {
      reached.resize((size_t)n);
    } catch (const std::bad_alloc &) {
      return set_err(KFX_ERR_OOM, "icp_multi: out of memory");
    }
    for (int64_t k = 0; k < n; ++k) reached[(size_t)k] = out[k].pose;
    const float keep = c->q_ms[0];
    r = quality_run(c, 0, pv[0], pn[0], reached.data(), n, nullptr, nullptr, q);
    c->m_ms[2] = c->q_ms[0];
    c->q_ms[0] = keep;
    if (r) return r;
  }
  return KFX_OK;
}

int kfx_icp_multi(kfx_ctx *c, const kfx_pose *starts, int64_t n, kfx_icp_result *out, kfx_icp_quality *q) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = multi_args(starts, n, out)) || n == 0) return r;
  c->m_ms[0] = 0.f;
  return multi_run(c, c->prev.v, c->prev.n, starts, n, out, q);
}

int kfx_track_view(kfx_ctx *c, const kfx_pose *cam_pose, const kfx_pose *starts, int64_t n, kfx_icp_result *out,
                   kfx_pose *world, kfx_icp_quality *q) {
  int r = check_ctx(c);
  if (r) return r;
  if (!cam_pose) return set_err(KFX_ERR_ARG, "null pose");
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(i < 9 ? cam_pose->R[i] : cam_pose->t[i - 9])) return set_err(KFX_ERR_ARG, "non-finite view pose");
  if ((r = multi_args(starts, n, out)) || n == 0) return r;
  if (c->slab && c->world > 1) return set_err(KFX_ERR_STATE, "track_view on one slab of several");
  // the model pyramid: per level [vmap | nmap | the view's image (k_view always stores one)], one direct
  // raycast each at that level's intrinsics (kfx_score_view's, not the resize pyramid)
  size_t off[kMaxLevels + 1] = {0};
  for (int l = 0; l < c->L; ++l) off[l + 1] = off[l] + ((27 * (size_t)c->g[l].w * c->g[l].h + 15) & ~(size_t)15);
  if ((r = reserve(&c->m_buf[2], &c->m_cap[2], off[c->L], "track_view"))) return r;
  if ((r = make_events(c->ev_m, 4))) return r;
  const DevPose cam = to_dev(*cam_pose);
  const DevPose c2v = host_pose_mul(host_pose_inv(to_dev(c->p.volu_pose)), cam);  // kfx_render_view's pose
  const float *pv[kMaxLevels] = {}, *pn[kMaxLevels] = {};
  HIPCHK(hipEventRecord(c->ev_m[0], c->stream));
  for (int l = 0; l < c->L; ++l) {
    const size_t np = (size_t)c->g[l].w * c->g[l].h;
    float *dv = reinterpret_cast<float *>(static_cast<char *>(c->m_buf[2]) + off[l]), *dn = dv + 3 * np;
    launch_view(c->stream, c->vol, c->g[l], c2v, cam.t, KFX_VIEW_NORMAL, reinterpret_cast<uint8_t *>(dn + 3 * np), dv, dn,
                nullptr);
    pv[l] = dv;
    pn[l] = dn;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_m[1], c->stream));
  if ((r = multi_run(c, pv, pn, starts, n, out, q))) return r;
  HIPCHK(hipEventElapsedTime(&c->m_ms[0], c->ev_m[0], c->ev_m[1]));
  if (world)
    for (int64_t k = 0; k < n; ++k) world[k] = to_api(host_pose_mul(cam, to_dev(out[k].pose)));
  return KFX_OK;
}

int kfx_icp_multi_chunk(int width, int height, int64_t n) {
  if (width < 1 || height < 1 || n < 1 || (int64_t)width * height > ((int64_t)1 << 26))
    return set_err(KFX_ERR_ARG, "icp_multi_chunk: width, height, n >= 1 and width * height <= 2^26");
  return icp_multi_chunk(width, height, n);
}

int kfx_get_icp_multi_ms(kfx_ctx *c, float out_ms[3]) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out_ms) return set_err(KFX_ERR_ARG, "null ms");
  for (int k = 0; k < 3; ++k) out_ms[k] = c->m_ms[k];
  return KFX_OK;
}

// The next frame tracks from cam_pose against the volume as it stands: the
// pose joins the record, the frame count leaves the bootstrap, and PREV is what
// a frame tracked at cam_pose would have left (kfx_stage_raycast at cam2vol =
// inv(volume pose) * cam_pose, Rinv = its rotation transposed).  The captured
// graphs read the record, the count and PREV from device memory at the
// addresses they hold, none of which moves here, so they stay.
int kfx_resume_at(kfx_ctx *c, const kfx_pose *cam_pose) {
  int r = check_ctx(c);
  if (r) return r;
  if (!cam_pose) return set_err(KFX_ERR_ARG, "null pose");
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(i < 9 ? cam_pose->R[i] : cam_pose->t[i - 9])) return set_err(KFX_ERR_ARG, "non-finite pose entry");
  if (c->slab && c->world > 1) return set_err(KFX_ERR_STATE, "resume_at on one slab of several");
  if (c->cstream) HIPCHK(hipStreamSynchronize(c->cstream));
  HIPCHK(hipStreamSynchronize(c->pstream));
  HIPCHK(hipStreamSynchronize(c->stream));
  DevState s;
  HIPCHK(hipMemcpy(&s, c->st, sizeof(s), hipMemcpyDeviceToHost));
  if (s.n_poses >= c->pose_cap) return set_err(KFX_ERR_STATE, "resume_at: the pose record is full");
  const DevPose cam = to_dev(*cam_pose);
  HIPCHK(hipMemcpy(c->pose_log + s.n_poses, &cam, sizeof(cam), hipMemcpyHostToDevice));
  // the state's head, frame_count .. n_poses, as read (nothing runs that could write it), in one copy
  static_assert(offsetof(DevState, frame_count) == 0 && offsetof(DevState, n_poses) == 3 * sizeof(int), "the head");
  s.n_poses += 1;
  s.frame_count = std::max(s.frame_count, 1) + 1;
  HIPCHK(hipMemcpy(c->st, &s, 4 * sizeof(int), hipMemcpyHostToDevice));
  c->known_poses = s.n_poses;  // every queued frame has completed (the pending status is left to kfx_synchronize)
  const DevPose c2v = host_pose_mul(host_pose_inv(to_dev(c->p.volu_pose)), cam);  // tsdf_volume.cpp:59
  const kfx_pose cam2vol = to_api(c2v);
  float Rinv[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rinv[3 * i + j] = c2v.R[3 * j + i];
  return kfx_stage_raycast(c, &cam2vol, Rinv);
}

// ---- fern keyframes and relocalisation -----------------------

static const kfx_fern_params kFernDefaults = {512, 400u, 4000u, 2013ull};
constexpr int64_t kMaxKeyframes = (int64_t)1 << 24;
constexpr size_t kSearchPartBytes = (size_t)64 << 20;  // the per-block keys of one search launch at the most

static bool pose_finite(const kfx_pose &p) {
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(i < 9 ? p.R[i] : p.t[i - 9])) return false;
  return true;
}

int kfx_fern_table(const kfx_intrinsics *intr, int pyramid_height, const kfx_fern_params *params, kfx_fern *out) {
  if (!intr || !out) return set_err(KFX_ERR_ARG, "null argument");
  if (pyramid_height < 1 || pyramid_height > KFX_MAX_LEVELS) return set_err(KFX_ERR_ARG, "pyramid height outside 1..4");
  const FernGrid g = fern_grid(intr->width, intr->height, pyramid_height);
  if (intr->width < 1 || intr->height < 1 || g.wL < 1 || g.hL < 1) return set_err(KFX_ERR_ARG, "empty fern grid");
  const kfx_fern_params p = params ? *params : kFernDefaults;
  if (!fern_params_ok(p)) return set_err(KFX_ERR_ARG, "n_ferns: a multiple of 16 in 16..1024; depth_min_mm <= depth_max_mm");
  fern_table(g, p, out);
  return KFX_OK;
}

static void kf_free(kfx_keyframes *kf) {
  (void)hipSetDevice(kf->device);
  if (kf->d_table) (void)hipFree(kf->d_table);
  if (kf->d_codes) (void)hipFree(kf->d_codes);
  if (kf->d_code) (void)hipFree(kf->d_code);
  delete kf;
  (void)hipGetLastError();
}

// a store around the host mirror h on c's device: the table uploaded, no codes yet
static int kf_make(kfx_ctx *c, KeyframeHost &&h, kfx_keyframes **out) {
  kfx_keyframes *kf = new (std::nothrow) kfx_keyframes;
  if (!kf) return set_err(KFX_ERR_OOM, "keyframes: out of memory");
  kf->h = std::move(h);
  kf->device = c->device;
  kf->width = c->intr.width;
  kf->height = c->intr.height;
  const size_t tb = kf->h.table.size() * sizeof(kfx_fern);
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&kf->d_table), tb);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&kf->d_code), sizeof(uint64_t) * kf->h.words);
  if (e == hipSuccess) e = hipMemcpy(kf->d_table, kf->h.table.data(), tb, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    kf_free(kf);
    return hip_err("keyframes", e);
  }
  *out = kf;
  return KFX_OK;
}

// the store belongs to this context's device and fern grid
static int kf_args(kfx_ctx *c, const kfx_keyframes *kf) {
  if (!kf) return set_err(KFX_ERR_ARG, "null keyframe store");
  const FernGrid g = fern_grid(c->intr.width, c->intr.height, c->L);
  if (kf->device != c->device || kf->width != c->intr.width || kf->height != c->intr.height || kf->h.grid.wL != g.wL ||
      kf->h.grid.hL != g.hL || kf->h.grid.s != g.s)
    return set_err(KFX_ERR_ARG, "the keyframe store belongs to another device or fern grid");
  return KFX_OK;
}

int kfx_keyframes_create(kfx_ctx *c, const kfx_fern_params *params, const kfx_fern *table, kfx_keyframes **out) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out) return set_err(KFX_ERR_ARG, "null out");
  const kfx_fern_params p = params ? *params : kFernDefaults;
  if (!(table ? fern_count_ok(p.n_ferns) : fern_params_ok(p)))
    return set_err(KFX_ERR_ARG, "n_ferns: a multiple of 16 in 16..1024; depth_min_mm <= depth_max_mm");
  KeyframeHost h;
  h.par = p;
  h.grid = fern_grid(c->intr.width, c->intr.height, c->L);
  h.words = p.n_ferns / 16;
  try {
    h.table.resize((size_t)p.n_ferns);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "keyframes: out of memory");
  }
  if (table) {
    if (!fern_table_ok(h.grid, table, p.n_ferns)) return set_err(KFX_ERR_ARG, "a fern outside the grid or a bad td");
    std::memcpy(h.table.data(), table, h.table.size() * sizeof(kfx_fern));
  } else {
    fern_table(h.grid, p, h.table.data());
  }
  return kf_make(c, std::move(h), out);
}

int kfx_keyframes_destroy(kfx_keyframes *kf) {
  if (kf) kf_free(kf);
  return KFX_OK;
}

int kfx_keyframes_get_table(const kfx_keyframes *kf, kfx_fern *out) {
  if (!kf || !out) return set_err(KFX_ERR_ARG, "null argument");
  std::memcpy(out, kf->h.table.data(), kf->h.table.size() * sizeof(kfx_fern));
  return KFX_OK;
}

int kfx_keyframes_count(const kfx_keyframes *kf, int64_t *n) {
  if (!kf || !n) return set_err(KFX_ERR_ARG, "null argument");
  *n = kf->h.count();
  return KFX_OK;
}

int kfx_keyframes_put(kfx_keyframes *kf, const kfx_pose *cam_pose, const uint64_t *code, int32_t *id) {
  if (!kf || !cam_pose || !code) return set_err(KFX_ERR_ARG, "null argument");
  if (!pose_finite(*cam_pose)) return set_err(KFX_ERR_ARG, "non-finite pose entry");
  if (kf->h.count() >= kMaxKeyframes) return set_err(KFX_ERR_STATE, "the keyframe store is full");
  int32_t k;
  try {
    k = kf->h.put(*cam_pose, code);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "keyframes: out of memory");
  }
  if (id) *id = k;
  return KFX_OK;
}

int kfx_keyframes_get(const kfx_keyframes *kf, int32_t id, kfx_pose *cam_pose, uint64_t *code) {
  if (!kf) return set_err(KFX_ERR_ARG, "null keyframe store");
  if (id < 0 || id >= kf->h.count()) return set_err(KFX_ERR_ARG, "no such keyframe");
  if (cam_pose) *cam_pose = kf->h.poses[(size_t)id];
  if (code) std::memcpy(code, kf->h.codes.data() + (size_t)id * kf->h.words, sizeof(uint64_t) * kf->h.words);
  return KFX_OK;
}

int kfx_keyframes_search_chunk(int64_t n_keyframes, int64_t q) {
  if (n_keyframes < 0 || n_keyframes > kMaxKeyframes || q < 1 || q > 65536)
    return set_err(KFX_ERR_ARG, "search_chunk: n in 0..2^24, q in 1..2^16");
  return search_chunk_rule(n_keyframes, q);
}

int kfx_keyframes_export(const kfx_keyframes *kf, void *blob, int64_t cap, int64_t *bytes) {
  if (!kf || !bytes) return set_err(KFX_ERR_ARG, "null argument");
  const int64_t need = blob_bytes(kf->h);
  *bytes = need;
  if (!blob) return KFX_OK;
  if (cap < need) return set_err(KFX_ERR_ARG, "export: the buffer is smaller than the blob");
  blob_write(kf->h, blob);
  return KFX_OK;
}

int kfx_keyframes_import(kfx_ctx *c, const void *blob, int64_t bytes, kfx_keyframes **out) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out) return set_err(KFX_ERR_ARG, "null out");
  KeyframeHost h;
  try {
    if (const char *why = blob_read(blob, bytes, fern_grid(c->intr.width, c->intr.height, c->L), &h))
      return set_err(KFX_ERR_ARG, std::string("import: ") + why);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "keyframes: out of memory");
  }
  if (h.count() > kMaxKeyframes) return set_err(KFX_ERR_ARG, "import: more keyframes than a store holds");
  return kf_make(c, std::move(h), out);
}

// The device's code table holds keyframes [0, count) and has room for `need`:
// grown (and filled again from the mirror) where it is too small, then the
// keyframes kfx_keyframes_put left on the host uploaded, one strided copy.
static int kf_sync(kfx_ctx *c, kfx_keyframes *kf, int64_t need) {
  const int W = kf->h.words;
  const int64_t n = kf->h.count();
  if (need > kf->cap) {
    const int64_t cap = std::max<int64_t>(need, std::max<int64_t>(1024, 2 * kf->cap));
    if (kf->d_codes) (void)hipFree(kf->d_codes);  // nothing queued reads it: every call that does ends with a sync
    kf->d_codes = nullptr;
    kf->cap = kf->synced = 0;
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&kf->d_codes), sizeof(uint64_t) * (size_t)W * (size_t)cap);
    if (e != hipSuccess) {
      kf->d_codes = nullptr;
      (void)hipGetLastError();
      return set_err(KFX_ERR_OOM, std::string("keyframes: hipMalloc: ") + hipGetErrorString(e));
    }
    kf->cap = cap;
  }
  if (kf->synced < n) {
    const int64_t lo = kf->synced, cnt = n - lo;
    std::vector<uint64_t> stage;
    try {
      stage.resize((size_t)cnt * W);
    } catch (const std::bad_alloc &) {
      return set_err(KFX_ERR_OOM, "keyframes: out of memory");
    }
    for (int64_t i = 0; i < cnt; ++i)
      for (int w = 0; w < W; ++w) stage[(size_t)w * cnt + i] = kf->h.codes[(size_t)(lo + i) * W + w];
    HIPCHK(hipMemcpy2DAsync(kf->d_codes + lo, sizeof(uint64_t) * (size_t)kf->cap, stage.data(), sizeof(uint64_t) * (size_t)cnt,
                            sizeof(uint64_t) * (size_t)cnt, (size_t)W, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    kf->synced = n;
  }
  return KFX_OK;
}

// The frame's code: the CUR dmap of level L - 1 and the colour the integrate
// stage would fuse, on the frame stream behind every queued frame.  slot: also
// into the code table's column `count` (kf_sync(count + 1) came first), where
// it counts once the host mirror takes the keyframe.  ev_kf[0, 1] time it.
static int kf_encode(kfx_ctx *c, kfx_keyframes *kf, bool slot, uint64_t *code) {
  int r;
  if ((r = make_events(c->ev_kf, 4))) return r;
  const int W = kf->h.words;
  HIPCHK(hipEventRecord(c->ev_kf[0], c->stream));
  launch_fern_encode(c->stream, kf->d_table, kf->h.par.n_ferns, c->last_bgr ? c->last_bgr : c->bgr, c->intr.width,
                     c->cur.d[c->L - 1], kf->h.grid.wL, kf->h.grid.s, kf->d_code,
                     slot ? kf->d_codes + kf->h.count() : nullptr, kf->cap);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_kf[1], c->stream));
  HIPCHK(hipMemcpyAsync(code, kf->d_code, sizeof(uint64_t) * W, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipEventElapsedTime(&c->kf_ms[0], c->ev_kf[0], c->ev_kf[1]));
  return KFX_OK;
}

// The k nearest keyframes of q codes (host; null: the last encode's, on the
// device, q = 1), q * k matches in match order.  Launches of at most
// kSearchPartBytes of per-block keys each.  ev_kf[2, 3] time them.
static int kf_search(kfx_ctx *c, kfx_keyframes *kf, const uint64_t *codes, int64_t q, int k, kfx_keyframe_match *out) {
  static_assert(sizeof(kfx_keyframe_match) == sizeof(uint64_t), "a match is a key's two halves");
  int r;
  const int W = kf->h.words;
  const int64_t n = kf->h.count();
  c->kf_ms[1] = 0.f;
  if (n == 0) {
    for (int64_t i = 0; i < q * k; ++i) out[i] = {-1, -1};
    return KFX_OK;
  }
  if ((r = kf_sync(c, kf, n))) return r;
  const size_t per_query = (size_t)search_key_blocks(n) * k * sizeof(uint64_t);
  const int64_t qb = std::max<int64_t>(1, std::min<int64_t>(q, (int64_t)(kSearchPartBytes / per_query)));
  if (codes && (r = reserve(&c->kf_buf[0], &c->kf_cap[0], sizeof(uint64_t) * (size_t)q * W, "search"))) return r;
  if ((r = reserve(&c->kf_buf[1], &c->kf_cap[1], per_query * (size_t)qb, "search"))) return r;
  if ((r = reserve(&c->kf_buf[2], &c->kf_cap[2], sizeof(uint64_t) * (size_t)q * k, "search"))) return r;
  if ((r = make_events(c->ev_kf, 4))) return r;
  if (codes)
    HIPCHK(hipMemcpyAsync(c->kf_buf[0], codes, sizeof(uint64_t) * (size_t)q * W, hipMemcpyHostToDevice, c->stream));
  const unsigned long long *dq = codes ? static_cast<const unsigned long long *>(c->kf_buf[0]) : kf->d_code;
  unsigned long long *dout = static_cast<unsigned long long *>(c->kf_buf[2]);
  HIPCHK(hipEventRecord(c->ev_kf[2], c->stream));
  for (int64_t q0 = 0; q0 < q; q0 += qb)
    launch_fern_search(c->stream, kf->d_codes, kf->cap, (int)n, W, dq + (size_t)q0 * W, (int)std::min(qb, q - q0), k,
                       static_cast<unsigned long long *>(c->kf_buf[1]), dout + (size_t)q0 * k);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_kf[3], c->stream));
  HIPCHK(hipMemcpyAsync(out, dout, sizeof(uint64_t) * (size_t)q * k, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipEventElapsedTime(&c->kf_ms[1], c->ev_kf[2], c->ev_kf[3]));
  return KFX_OK;
}

int kfx_encode_frame(kfx_ctx *c, kfx_keyframes *kf, uint64_t *code) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = kf_args(c, kf))) return r;
  if (!code) return set_err(KFX_ERR_ARG, "null code");
  uint64_t tmp[kFernMaxWords];
  if ((r = kf_encode(c, kf, false, tmp))) return r;
  std::memcpy(code, tmp, sizeof(uint64_t) * kf->h.words);
  return KFX_OK;
}

// encode into the table's next column and take the keyframe into the mirror
static int kf_add(kfx_ctx *c, kfx_keyframes *kf, const kfx_pose &pose, bool encoded, uint64_t *code, int32_t *id) {
  int r;
  if (kf->h.count() >= kMaxKeyframes) return set_err(KFX_ERR_STATE, "the keyframe store is full");
  if (!encoded) {
    if ((r = kf_sync(c, kf, kf->h.count() + 1))) return r;
    if ((r = kf_encode(c, kf, true, code))) return r;
  }
  int32_t k;
  try {
    k = kf->h.put(pose, code);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "keyframes: out of memory");
  }
  kf->synced = kf->h.count();  // the encode wrote this column
  if (id) *id = k;
  return KFX_OK;
}

int kfx_keyframes_add(kfx_ctx *c, kfx_keyframes *kf, const kfx_pose *cam_pose, int32_t *id) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = kf_args(c, kf))) return r;
  kfx_pose pose;
  if (cam_pose) {
    if (!pose_finite(*cam_pose)) return set_err(KFX_ERR_ARG, "non-finite pose entry");
    pose = *cam_pose;
  } else if ((r = kfx_get_cur_camera_pose(c, &pose))) {
    return r;
  }
  uint64_t code[kFernMaxWords];
  return kf_add(c, kf, pose, false, code, id);
}

int kfx_keyframes_consider(kfx_ctx *c, kfx_keyframes *kf, int32_t min_distance, int32_t *id,
                           kfx_keyframe_match *nearest) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = kf_args(c, kf))) return r;
  if (!id) return set_err(KFX_ERR_ARG, "null id");
  if (kf->h.count() >= kMaxKeyframes) return set_err(KFX_ERR_STATE, "the keyframe store is full");
  kfx_pose pose;
  if ((r = kfx_get_cur_camera_pose(c, &pose))) return r;
  uint64_t code[kFernMaxWords];
  if ((r = kf_sync(c, kf, kf->h.count() + 1))) return r;
  if ((r = kf_encode(c, kf, true, code))) return r;
  kfx_keyframe_match m = {-1, -1};
  if (kf->h.count() && (r = kf_search(c, kf, nullptr, 1, 1, &m))) return r;
  int32_t added = -1;
  if (m.id < 0 || m.distance > min_distance)
    if ((r = kf_add(c, kf, pose, true, code, &added))) return r;
  *id = added;
  if (nearest) *nearest = m;
  return KFX_OK;
}

int kfx_keyframes_search(kfx_ctx *c, kfx_keyframes *kf, const uint64_t *codes, int64_t q, int k,
                         kfx_keyframe_match *out) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = kf_args(c, kf))) return r;
  if (q < 0 || q > 65536) return set_err(KFX_ERR_ARG, "q outside 0..2^16");
  if (k < 1 || k > kSearchMaxK) return set_err(KFX_ERR_ARG, "k outside 1..16");
  if (q == 0) return KFX_OK;
  if (!out) return set_err(KFX_ERR_ARG, "null out");
  if (!codes) {
    uint64_t code[kFernMaxWords];
    q = 1;
    if ((r = kf_encode(c, kf, false, code))) return r;
  }
  std::vector<kfx_keyframe_match> res;
  try {
    res.resize((size_t)q * k);
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "search: out of memory");
  }
  if ((r = kf_search(c, kf, codes, q, k, res.data()))) return r;
  std::memcpy(out, res.data(), res.size() * sizeof(kfx_keyframe_match));
  return KFX_OK;
}

int kfx_get_keyframe_ms(kfx_ctx *c, float out_ms[2]) {
  int r = check_ctx(c);
  if (r) return r;
  if (!out_ms) return set_err(KFX_ERR_ARG, "null ms");
  out_ms[0] = c->kf_ms[0];
  out_ms[1] = c->kf_ms[1];
  return KFX_OK;
}

static void reloc_none(kfx_reloc_result *o, int status) {
  std::memset(o, 0, sizeof(*o));
  o->status = status;
  o->keyframe = o->distance = o->start = -1;
}

int kfx_relocalise(kfx_ctx *c, kfx_keyframes *kf, int k, const kfx_pose *starts, int64_t n, double min_fitness,
                   kfx_reloc_result *out) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = kf_args(c, kf))) return r;
  if (k < 1 || k > kSearchMaxK) return set_err(KFX_ERR_ARG, "k outside 1..16");
  if (!out) return set_err(KFX_ERR_ARG, "null out");
  if (std::isnan(min_fitness)) return set_err(KFX_ERR_ARG, "min_fitness is not a number");
  const kfx_pose id = {{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}};
  if (!starts) {
    starts = &id;
    n = 1;
  }
  if (n < 0 || n > 65536) return set_err(KFX_ERR_ARG, "n outside 0..2^16");
  for (int64_t i = 0; i < n; ++i)
    if (!pose_finite(starts[i])) return set_err(KFX_ERR_ARG, "non-finite pose entry");
  if (c->slab && c->world > 1) return set_err(KFX_ERR_STATE, "relocalise on one slab of several");
  uint64_t code[kFernMaxWords];
  kfx_keyframe_match match[kSearchMaxK];
  if ((r = kf_encode(c, kf, false, code))) return r;
  if ((r = kf_search(c, kf, nullptr, 1, k, match))) return r;
  int n_matches = 0;
  while (n_matches < k && match[n_matches].id >= 0) ++n_matches;
  std::vector<kfx_icp_result> icp;
  std::vector<kfx_pose> world;
  std::vector<kfx_icp_quality> qual;
  std::vector<RelocCand> cand;
  try {
    icp.resize((size_t)n_matches * n);
    world.resize(icp.size());
    qual.resize(icp.size());
    cand.reserve(icp.size());
  } catch (const std::bad_alloc &) {
    return set_err(KFX_ERR_OOM, "relocalise: out of memory");
  }
  for (int m = 0; m < n_matches && n > 0; ++m) {
    const size_t o = (size_t)m * n;
    if ((r = kfx_track_view(c, &kf->h.poses[(size_t)match[m].id], starts, n, &icp[o], &world[o], &qual[o]))) return r;
    for (int64_t s = 0; s < n; ++s)
      if (icp[o + s].status == KFX_OK) cand.push_back(reloc_cand(qual[o + s], m, (int)s));
  }
  const int best = reloc_select(cand.data(), (int)cand.size());
  double fitness = 0.0, rmse = 0.0;
  bool accept = false;
  size_t at = 0;
  if (best >= 0) {
    at = (size_t)cand[best].match * n + cand[best].start;
    if ((r = kfx_quality_figures(&qual[at], &fitness, &rmse))) return r;
    accept = fitness >= min_fitness;
  }
  if (!accept) {
    reloc_none(out, KFX_TRACKING_LOST);
  } else {
    reloc_none(out, KFX_OK);
    out->keyframe = match[cand[best].match].id;
    out->distance = match[cand[best].match].distance;
    out->start = cand[best].start;
    out->world = world[at];
    out->icp = icp[at];
    out->q = qual[at];
  }
  out->n_matches = n_matches;
  out->n_converged = (int32_t)cand.size();
  return out->status;
}

// kfx_stage_preprocess + kfx_stage_icp: would this frame track from the state as it stands?
static int recover_probe(kfx_ctx *c, const uint8_t *bgr, const float *depth_mm) {
  const int r = kfx_stage_preprocess(c, bgr, depth_mm);
  return r ? r : kfx_stage_icp(c, nullptr);
}

int kfx_pipeline_recover(kfx_ctx *c, kfx_keyframes *kf, const uint8_t *bgr, const float *depth_mm,
                         const kfx_recover_params *params, kfx_recover_report *report) {
  int r = check_ctx(c);
  if (r) return r;
  if ((r = kf_args(c, kf))) return r;
  if (!bgr || !depth_mm) return set_err(KFX_ERR_ARG, "null image");
  if (!report) return set_err(KFX_ERR_ARG, "null report");
  const kfx_recover_params p = params ? *params : kfx_recover_params{4, kf->h.par.n_ferns / 10, 0.15, 0.25};
  if (p.k < 1 || p.k > kSearchMaxK || std::isnan(p.min_fitness) || std::isnan(p.harvest_min_fitness))
    return set_err(KFX_ERR_ARG, "recover: k outside 1..16 or a fitness that is not a number");
  if (c->slab && c->world > 1) return set_err(KFX_ERR_STATE, "pipeline_recover on one slab of several");
  kfx_recover_report rep;
  rep.event = 0;
  rep.keyframe_added = -1;
  reloc_none(&rep.reloc, KFX_OK);
  int count = 0;
  if ((r = kfx_get_frame_count(c, &count))) return r;
  if (count == 1) {
    rep.event = 1;
  } else {
    r = recover_probe(c, bgr, depth_mm);
    if (r == KFX_TRACKING_LOST) {
      r = kfx_relocalise(c, kf, p.k, nullptr, 1, p.min_fitness, &rep.reloc);
      if (r == KFX_OK) {
        if ((r = kfx_resume_at(c, &rep.reloc.world))) return r;
        r = recover_probe(c, bgr, depth_mm);
        if (r == KFX_OK) rep.event = 2;
      }
      if (r == KFX_TRACKING_LOST) {  // no candidate, or the adopted pose does not track: the map is kept
        rep.event = 3;
        *report = rep;
        return KFX_TRACKING_LOST;
      }
    }
    if (r) return r;
  }
  if ((r = kfx_pipeline(c, bgr, depth_mm)) < 0) return r;
  if (r == KFX_TRACKING_LOST) {  // the committed frame disagreed with its probe: kfx_pipeline's reset has been applied
    *report = rep;
    return set_err(KFX_ERR_STATE, "pipeline_recover: the probe tracked and the committed frame did not");
  }
  bool harvest = rep.event == 1;
  if (!harvest) {
    kfx_icp_quality q;
    double fitness = 0.0, rmse = 0.0;
    if ((r = kfx_frame_quality(c, 0, nullptr, nullptr, &q))) return r;
    if ((r = kfx_quality_figures(&q, &fitness, &rmse))) return r;
    harvest = fitness >= p.harvest_min_fitness;
  }
  if (harvest && (r = kfx_keyframes_consider(c, kf, p.harvest_min_distance, &rep.keyframe_added, nullptr))) return r;
  *report = rep;
  return KFX_OK;
}

}  // extern "C"
