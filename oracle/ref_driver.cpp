/*
 * ref_driver.cpp — TEST INFRASTRUCTURE ONLY.
 *
 * extern "C" entry points over the reference's own host-compiled kernels
 * (oracle/Makefile, target `ref`; oracle/ref_shim/).  Each wrapper builds the
 * reference's argument structs over the caller's buffers and calls the
 * reference's launcher; nothing is computed here.  Conventions shared with
 * kfx_oracle.h: R is row-major float[9], maps are dense (step = cols * element
 * size), the volume is the reference's own 8-byte voxel records, x fastest.
 */
#include <device_types.hpp>
#include <device_utils.cuh>

using namespace kf;
using namespace kf::device;

/* PoseR::data[i] is column i of R (cv2cuda(Matx33f)) */
static PoseR pose_r(const float *R) {
  PoseR r;
  for (int i = 0; i < 3; i++) r.data[i] = make_float3(R[i], R[3 + i], R[6 + i]);
  return r;
}
static PoseT pose_t(const float *R, const float *t) {
  PoseT p;
  p.R = pose_r(R);
  p.t = make_float3(t[0], t[1], t[2]);
  return p;
}
static GpuMat mat(void *p, int w, int h, size_t elem) {
  GpuMat m;
  m.data = p;
  m.cols = w;
  m.rows = h;
  m.step = w * elem;
  return m;
}
/* voxel_size as TSDFVolume forms it: range / dims per axis, in float */
static Volume volume(void *rec, const int *d, const float *rg, float trunc) {
  const float3 vs = make_float3(rg[0] / d[0], rg[1] / d[1], rg[2] / d[2]);
  Volume v((Voxel *)rec, make_int3(d[0], d[1], d[2]), make_float3(rg[0], rg[1], rg[2]), vs);
  v.trun_dist = trunc;
  return v;
}
/* k = {fx, fy, cx, cy} */
static Intrs intrs(const float *k) {
  Intrinsics i;
  i.fx = k[0];
  i.fy = k[1];
  i.cx = k[2];
  i.cy = k[3];
  return Intrs(i);
}

extern "C" {

int ref_voxel_bytes() { return (int)sizeof(Voxel); }

void ref_integrate(void *rec, const int *dims, const float *range, float trunc, const float *k, const float *R,
                   const float *t, float *dmap, int w, int h, unsigned char *bgr) {
  Volume v = volume(rec, dims, range, trunc);
  GpuMat dm = mat(dmap, w, h, 4), cm = mat(bgr, w, h, 3);
  integrate(intrs(k), pose_t(R, t), v, dm, cm);
}

void ref_raycast(void *rec, const int *dims, const float *range, const float *k, const float *R, const float *t,
                 const float *Rinv, float *vmap, float *nmap, int w, int h) {
  Volume v = volume(rec, dims, range, 0.f);
  GpuMat vm = mat(vmap, w, h, 12), nm = mat(nmap, w, h, 12);
  raycast(intrs(k), pose_t(R, t), pose_r(Rinv), v, vm, nm);
}

void ref_depth_truncation(float *dmap, int w, int h, float max_dist) {
  GpuMat dm = mat(dmap, w, h, 4);
  depthTruncation(dm, max_dist);
}

void ref_vertex_map(float *dmap, int w, int h, const float *k, float *vmap) {
  GpuMat dm = mat(dmap, w, h, 4), vm = mat(vmap, w, h, 12);
  getVertexmap(dm, vm, intrs(k));
}

void ref_normal_map(float *vmap, int w, int h, float *nmap) {
  GpuMat vm = mat(vmap, w, h, 12), nm = mat(nmap, w, h, 12);
  getNormalmap(vm, nm);
}

/* big maps are 2 ws x 2 hs */
void ref_resize(float *vbig, float *nbig, int ws, int hs, float *vsmall, float *nsmall) {
  GpuMat vb = mat(vbig, 2 * ws, 2 * hs, 12), nb = mat(nbig, 2 * ws, 2 * hs, 12);
  GpuMat v = mat(vsmall, ws, hs, 12), n = mat(nsmall, ws, hs, 12);
  resizePointsNormals(vb, nb, v, n);
}

/* type 0: renderPhong, 1: renderNormals; out is w * h uchar3, zeroed by the caller */
void ref_render(float *vmap, float *nmap, int w, int h, const float *eye, int type, unsigned char *out) {
  GpuMat vm = mat(vmap, w, h, 12), nm = mat(nmap, w, h, 12), cm = mat(out, w, h, 3);
  if (type == 0)
    renderPhong(make_float3(eye[0], eye[1], eye[2]), vm, nm, cm);
  else
    renderNormals(nm, cm);
}

/* in / out: {width, height} and {fx, fy, cx, cy} */
void ref_level_intrinsics(const int *size, const float *k, int level, int *size_out, float *k_out) {
  Intrinsics i;
  i.width = size[0];
  i.height = size[1];
  i.fx = k[0];
  i.fy = k[1];
  i.cx = k[2];
  i.cy = k[3];
  const Intrinsics o = i.level((size_t)level);
  size_out[0] = o.width;
  size_out[1] = o.height;
  k_out[0] = o.fx;
  k_out[1] = o.fy;
  k_out[2] = o.cx;
  k_out[3] = o.cy;
}

/* ICP::findCoresp on every pixel; rows = w * h * 7 floats laid out as the
 * reference's kernel forms them (cross(s, n), n, dot(n, d - s)), zeros where
 * no correspondence is found */
void ref_icp_rows(float *cur_v, float *cur_n, float *pre_v, float *pre_n, int w, int h, const float *k,
                  const float *R, const float *t, float dist_thres, float angle_thres, float *rows) {
  ICP icp(dist_thres, angle_thres);
  icp.cur_vmap = mat(cur_v, w, h, 12);
  icp.cur_nmap = mat(cur_n, w, h, 12);
  icp.pre_vmap = mat(pre_v, w, h, 12);
  icp.pre_nmap = mat(pre_n, w, h, 12);
  icp.setIntrs(intrs(k), w, h);
  icp.curpose = pose_t(R, t);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      float3 n, d, s;
      float *r = rows + 7 * ((size_t)y * w + x);
      if (icp.findCoresp(x, y, n, d, s)) {
        const float3 c = cross(s, n);
        r[0] = c.x, r[1] = c.y, r[2] = c.z;
        r[3] = n.x, r[4] = n.y, r[5] = n.z;
        r[6] = dot(n, d - s);
      } else {
        for (int i = 0; i < 7; i++) r[i] = 0.f;
      }
    }
}

}  // extern "C"
