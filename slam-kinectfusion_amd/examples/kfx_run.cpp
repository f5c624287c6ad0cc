// kfx_run — the reference's main.cpp loop (main.cpp:63-98) on a dataset
// directory, over the C-ABI only (no OpenCV, no viz): depth_sensor::open /
// getFrame → kinectfusion::pipeline per frame → poses.txt (and optionally the
// point cloud PLY, main.cpp:43-44; the coloured, oriented cloud and mesh are
// extensions: kfx_save_pointcloud_attr / kfx_save_mesh_attr; view.ppm is the
// fused colour rendered from the last tracked pose, kfx_render_view;
// followed_cloud.ply makes the volume follow the camera, kfx_shift_for_pose /
// kfx_evict_points / kfx_shift_volume after every frame, and holds the evicted
// points followed by the final cloud; a non-empty eighth argument makes the
// follow loop lossless, DESIGN.md §21: the bricks a shift drops go into a host
// brick store, kfx_evict_bricks / kfx_brick_store_put, and those of the new
// window come back, kfx_brick_store_take_window / kfx_restore_bricks.  The
// followed cloud keeps its meaning, the points evicted at each shift, then the
// final window: a surface that left and returned appears once per departure;
// a ninth argument, with the eighth, writes the world mesh at the end, DESIGN.md
// §22: the window's bricks merged with the store's, kfx_save_world_mesh, every
// surface once wherever the window stands; a tenth argument writes the window's
// indexed mesh, DESIGN.md §24: shared vertices and a face list,
// kfx_save_mesh_indexed; an eleventh, with the eighth, the world's,
// kfx_save_world_mesh_indexed; a twelfth, with the eighth, world_view.ppm, DESIGN.md
// §25: window plus store in fused colour, seen from the first recorded pose
// through the dataset's intrinsics, kfx_save_world_view: the whole map, also
// where the window has moved on; a thirteenth names a text file that gets one
// line per processed frame, DESIGN.md §26: frame index, kfx_pipeline's status,
// the six label counts at level 0, fitness and rmse of kfx_frame_quality after
// the frame; a fourteenth is a number N > 0, DESIGN.md §27: after every Nth
// frame, frame N on, the frame is tracked again against the model seen from the
// pose N frames back, kfx_track_view from the identity start, and one line goes
// to the standard output: "track_view", the frame index, the status, the
// distance (m) and the angle (rad) between the world pose recovered and the one
// the tracker recorded, fitness and rmse at the pose reached; status -1 and
// zeros where the record does not reach N frames back); a fifteenth names a text
// file, DESIGN.md §28: the frames then go through kfx_pipeline_recover with the
// default parameters and a keyframe store of the default table instead of
// kfx_pipeline, and the file gets one line per frame: frame index, the event (0
// tracked, 1 bootstrap, 2 relocalised, 3 lost with the map kept), the keyframe
// added or -1, the keyframe relocalised against and its code distance or -1 -1,
// and the fitness of kfx_frame_quality after the frame (0 after event 3).  An
// empty name skips its
// output, the followed cloud's included, so that a later argument can be given alone.
//   usage: kfx_run <dataset dir> [poses.txt] [cloud.ply] [colored_cloud.ply] [colored_mesh.ply] [view.ppm]
//                  [followed_cloud.ply] [stream] [world_mesh.ply] [indexed_mesh.ply] [world_indexed_mesh.ply]
//                  [world_view.ppm] [quality.txt] [N] [recover.txt]
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/kfx.h"

int main(int argc, char **argv) {
  if (argc < 2) {
    std::fprintf(stderr,
                 "usage: %s <dataset dir> [poses.txt] [cloud.ply] [colored_cloud.ply] [colored_mesh.ply] [view.ppm] "
                 "[followed_cloud.ply] [stream] [world_mesh.ply] [indexed_mesh.ply] [world_indexed_mesh.ply] "
                 "[world_view.ppm] [quality.txt] [N] [recover.txt]\n",
                 argv[0]);
    return 2;
  }
  const char *poses = argc > 2 ? argv[2] : "poses.txt";
  kfx_dataset *ds = nullptr;
  if (kfx_dataset_open(argv[1], &ds) != KFX_OK) {
    std::fprintf(stderr, "error: %s\n", kfx_last_error());  // "error: no camera!"
    return 1;
  }
  kfx_intrinsics intr;
  int n = 0, has_intr = 0;
  kfx_dataset_info(ds, &intr, &n, &has_intr);
  if (!has_intr) {
    std::fprintf(stderr, "error: %s/intr.txt missing or malformed\n", argv[1]);
    return 1;
  }
  kfx_params p;
  kfx_default_params(&p);  // kinectfuison_params::default_params (kinectfusion.cpp:167-190)
  kfx_ctx *ctx = nullptr;
  if (kfx_create(&intr, &p, 0, &ctx) != KFX_OK) {
    std::fprintf(stderr, "error: %s\n", kfx_last_error());
    return 1;
  }
  std::printf("KinectFusion: start (%d frames, %dx%d)\n", n, intr.width, intr.height);
  std::vector<uint8_t> bgr((size_t)intr.width * intr.height * 3);
  std::vector<float> depth((size_t)intr.width * intr.height);
  double gpu_s = 0;
  const bool follow = argc > 7 && argv[7][0];  // the volume follows the camera
  const float ahead = 0.5f + p.volu_range[2] / 2;
  std::vector<kfx_vertex> evicted;
  int shifts = 0;
  // lossless follow: what a shift drops waits in the store until the window returns to it
  const bool stream = argc > 8 && argv[8][0];
  kfx_brick_store *store = nullptr;
  std::vector<kfx_brick> bricks;
  long long bricks_out = 0, bricks_in = 0;
  if (stream && kfx_brick_store_create(&store) != KFX_OK) {
    std::fprintf(stderr, "error: %s\n", kfx_last_error());
    return 1;
  }
  std::FILE *qlog = nullptr;  // per-frame tracking quality
  if (argc > 13 && argv[13][0] && !(qlog = std::fopen(argv[13], "w"))) {
    std::fprintf(stderr, "error: cannot open %s\n", argv[13]);
    return 1;
  }
  const int every = argc > 14 && argv[14][0] ? std::atoi(argv[14]) : 0;  // track against an earlier view
  std::FILE *rlog = nullptr;  // probe, then commit: the map is kept when tracking is lost
  kfx_keyframes *keyframes = nullptr;
  if (argc > 15 && argv[15][0]) {
    if (!(rlog = std::fopen(argv[15], "w"))) {
      std::fprintf(stderr, "error: cannot open %s\n", argv[15]);
      return 1;
    }
    if (kfx_keyframes_create(ctx, nullptr, nullptr, &keyframes) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
  }
  std::vector<kfx_pose> record;
  for (int k = 0; k < n; ++k) {
    if (kfx_dataset_read(ds, k, bgr.data(), depth.data()) != KFX_OK) {
      std::printf("no image! (%s)\n", kfx_last_error());
      break;
    }
    const auto t0 = std::chrono::steady_clock::now();
    kfx_recover_report rep;
    const int r = rlog ? kfx_pipeline_recover(ctx, keyframes, bgr.data(), depth.data(), nullptr, &rep)
                       : kfx_pipeline(ctx, bgr.data(), depth.data());
    gpu_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (r == KFX_TRACKING_LOST) {
      std::printf("tracking fail!\n");  // kinectfusion.cpp:99
    } else if (r != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    if (rlog) {
      kfx_icp_quality q;
      double fitness = 0, rmse = 0;
      if (rep.event != 3 && (kfx_frame_quality(ctx, 0, nullptr, nullptr, &q) != KFX_OK ||
                             kfx_quality_figures(&q, &fitness, &rmse) != KFX_OK)) {
        std::fprintf(stderr, "error: %s\n", kfx_last_error());
        return 1;
      }
      std::fprintf(rlog, "%d %d %d %d %d %.9g\n", k, rep.event, rep.keyframe_added, rep.reloc.keyframe, rep.reloc.distance,
                   fitness);
    }
    if (qlog) {  // how well the frame sits on the model it was fused into
      kfx_icp_quality q;
      double fitness = 0, rmse = 0;
      if (kfx_frame_quality(ctx, 0, nullptr, nullptr, &q) != KFX_OK || kfx_quality_figures(&q, &fitness, &rmse) != KFX_OK) {
        std::fprintf(stderr, "error: %s\n", kfx_last_error());
        return 1;
      }
      std::fprintf(qlog, "%d %d %lld %lld %lld %lld %lld %lld %.9g %.9g\n", k, r, (long long)q.n[0], (long long)q.n[1],
                   (long long)q.n[2], (long long)q.n[3], (long long)q.n[4], (long long)q.n[5], fitness, rmse);
    }
    if (every > 0 && k > 0 && k % every == 0) {
      int got = 0;
      if (kfx_get_pose_record(ctx, nullptr, 0, &got) != KFX_OK) {
        std::fprintf(stderr, "error: %s\n", kfx_last_error());
        return 1;
      }
      record.resize((size_t)got);
      if (got > 0 && kfx_get_pose_record(ctx, record.data(), got, &got) != KFX_OK) {
        std::fprintf(stderr, "error: %s\n", kfx_last_error());
        return 1;
      }
      int status = -1;
      double dist = 0, angle = 0, fitness = 0, rmse = 0;
      if (got - 1 - every >= 0) {
        const kfx_pose id = {{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}};
        const kfx_pose &tracked = record[(size_t)got - 1];
        kfx_icp_result res;
        kfx_icp_quality q;
        kfx_pose world;
        if (kfx_track_view(ctx, &record[(size_t)(got - 1 - every)], &id, 1, &res, &world, &q) != KFX_OK ||
            kfx_quality_figures(&q, &fitness, &rmse) != KFX_OK) {
          std::fprintf(stderr, "error: %s\n", kfx_last_error());
          return 1;
        }
        status = res.status;
        double d2 = 0, tr = 0;  // |t_w - t_t| and the angle of R_w^T R_t from its trace
        for (int i = 0; i < 3; ++i) d2 += ((double)world.t[i] - tracked.t[i]) * ((double)world.t[i] - tracked.t[i]);
        for (int i = 0; i < 9; ++i) tr += (double)world.R[i] * tracked.R[i];
        dist = std::sqrt(d2);
        angle = std::acos(std::fmin(1.0, std::fmax(-1.0, (tr - 1.0) / 2.0)));
      }
      std::printf("track_view %d %d %.9g %.9g %.9g %.9g\n", k, status, dist, angle, fitness, rmse);
    }
    if (!follow) continue;
    if (r == KFX_TRACKING_LOST) {  // the device reset cannot move the volume back: kfx.h (the store is kept)
      if (kfx_reset(ctx) != KFX_OK) {
        std::fprintf(stderr, "error: %s\n", kfx_last_error());
        return 1;
      }
      continue;
    }
    kfx_pose vol, cam;
    int s[3] = {0, 0, 0};
    int64_t ne = 0;
    if (kfx_get_volume_pose(ctx, &vol) != KFX_OK || kfx_get_cur_camera_pose(ctx, &cam) != KFX_OK ||
        kfx_shift_for_pose(&p, &vol, &cam, ahead, s) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    if (!s[0] && !s[1] && !s[2]) continue;
    if (kfx_evict_points(ctx, s, nullptr, 0, &ne) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    const size_t at = evicted.size();
    evicted.resize(at + (size_t)ne);
    if (ne > 0 && kfx_evict_points(ctx, s, evicted.data() + at, ne, &ne) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    if (stream) {  // the bricks themselves, before they go
      int64_t nb = 0;
      if (kfx_evict_bricks(ctx, s, nullptr, 0, &nb) != KFX_OK) {
        std::fprintf(stderr, "error: %s\n", kfx_last_error());
        return 1;
      }
      bricks.resize((size_t)nb);
      if ((nb > 0 && kfx_evict_bricks(ctx, s, bricks.data(), nb, &nb) != KFX_OK) ||
          kfx_brick_store_put(store, bricks.data(), nb) != KFX_OK) {
        std::fprintf(stderr, "error: %s\n", kfx_last_error());
        return 1;
      }
      bricks_out += nb;
    }
    if (kfx_shift_volume(ctx, s) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    ++shifts;
    if (stream) {  // and those the new window holds, back in
      int origin[3];
      int64_t nb = 0, nr = 0;
      if (kfx_get_volume_origin(ctx, origin) != KFX_OK ||
          kfx_brick_store_take_window(store, origin, p.volu_dims, nullptr, 0, &nb) != KFX_OK) {
        std::fprintf(stderr, "error: %s\n", kfx_last_error());
        return 1;
      }
      bricks.resize((size_t)nb);
      if ((nb > 0 && kfx_brick_store_take_window(store, origin, p.volu_dims, bricks.data(), nb, &nb) != KFX_OK) ||
          kfx_restore_bricks(ctx, bricks.data(), nb, &nr) != KFX_OK) {
        std::fprintf(stderr, "error: %s\n", kfx_last_error());
        return 1;
      }
      bricks_in += nr;
    }
  }
  int frames = 0;
  kfx_get_frame_count(ctx, &frames);
  if (kfx_write_poses_txt(ctx, poses) != KFX_OK) {
    std::fprintf(stderr, "error: %s\n", kfx_last_error());
    return 1;
  }
  // (an empty name skips that output, so a later one can be asked for alone)
  if ((argc > 3 && argv[3][0] && kfx_save_pointcloud(ctx, argv[3], 0) != KFX_OK) ||
      (argc > 4 && argv[4][0] && kfx_save_pointcloud_attr(ctx, argv[4], 0) != KFX_OK) ||
      (argc > 5 && argv[5][0] && kfx_save_mesh_attr(ctx, argv[5], 0) != KFX_OK)) {
    std::fprintf(stderr, "error: %s\n", kfx_last_error());
    return 1;
  }
  if (argc > 6 && argv[6][0]) {  // the fused colour seen from the last tracked pose, at the dataset's intrinsics
    kfx_pose last;
    std::vector<uint8_t> img((size_t)intr.width * intr.height * 3);
    if (kfx_get_cur_camera_pose(ctx, &last) != KFX_OK ||
        kfx_render_view(ctx, &intr, &last, KFX_VIEW_COLOR, img.data(), nullptr, nullptr, nullptr) != KFX_OK ||
        kfx_write_ppm(argv[6], img.data(), intr.width, intr.height) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
  }
  if (follow) {  // what left the volume, then what is in it
    int64_t nf = 0;
    const size_t at = evicted.size();
    if (kfx_extract_points_attr(ctx, nullptr, 0, &nf) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    evicted.resize(at + (size_t)nf);
    if ((nf > 0 && kfx_extract_points_attr(ctx, evicted.data() + at, nf, &nf) != KFX_OK) ||
        kfx_write_ply_attr(argv[7], evicted.data(), (int64_t)evicted.size()) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    std::printf("followed: %d shifts, %lld evicted points, %lld in the volume\n", shifts, (long long)at,
                (long long)nf);
  }
  if (stream && argc > 9 && argv[9][0]) {  // the world map: what the window holds and what it left behind
    int64_t nb = 0, nt = 0;
    if (kfx_world_bricks(ctx, store, nullptr, 0, &nb) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    bricks.resize((size_t)nb);
    if ((nb > 0 && kfx_world_bricks(ctx, store, bricks.data(), nb, &nb) != KFX_OK) ||
        kfx_world_mesh_attr(ctx, bricks.data(), nb, nullptr, 0, &nt) != KFX_OK ||
        kfx_save_world_mesh(ctx, store, argv[9], 0) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    std::printf("world: %lld bricks, %lld triangles\n", (long long)nb, (long long)nt);
  }
  if (argc > 10 && argv[10][0]) {  // the window's mesh with shared vertices and a face list
    int64_t nv = 0, nt = 0;
    if (kfx_extract_mesh_indexed(ctx, nullptr, 0, nullptr, 0, &nv, &nt) != KFX_OK ||
        kfx_save_mesh_indexed(ctx, argv[10]) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    std::printf("indexed: %lld vertices, %lld triangles\n", (long long)nv, (long long)nt);
  }
  if (stream && argc > 11 && argv[11][0]) {  // and the world's
    int64_t nb = 0, nv = 0, nt = 0;
    if (kfx_world_bricks(ctx, store, nullptr, 0, &nb) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    bricks.resize((size_t)nb);
    if ((nb > 0 && kfx_world_bricks(ctx, store, bricks.data(), nb, &nb) != KFX_OK) ||
        kfx_world_mesh_indexed(ctx, bricks.data(), nb, nullptr, 0, nullptr, 0, &nv, &nt) != KFX_OK ||
        kfx_save_world_mesh_indexed(ctx, store, argv[11]) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    std::printf("world indexed: %lld bricks, %lld vertices, %lld triangles\n", (long long)nb, (long long)nv, (long long)nt);
  }
  if (stream && argc > 12 && argv[12][0]) {  // the whole map from where the run began
    kfx_pose first;
    int got = 0;
    if (kfx_get_pose_record(ctx, &first, 1, &got) != KFX_OK || got < 1 ||
        kfx_save_world_view(ctx, store, &intr, &first, KFX_VIEW_COLOR, argv[12]) != KFX_OK) {
      std::fprintf(stderr, "error: %s\n", kfx_last_error());
      return 1;
    }
    float ms[2] = {0.f, 0.f};
    kfx_get_world_view_ms(ctx, ms);
    std::printf("world view: load %.3f ms, render %.3f ms\n", ms[0], ms[1]);
  }
  if (stream) {
    int64_t held = 0;
    kfx_brick_store_count(store, &held);
    std::printf("streamed: %lld bricks out, %lld back in, %lld held\n", bricks_out, bricks_in, (long long)held);
    kfx_brick_store_destroy(store);
  }
  if (qlog) std::fclose(qlog);
  if (rlog) {
    int64_t held = 0;
    kfx_keyframes_count(keyframes, &held);
    std::printf("recover: %lld keyframes\n", (long long)held);
    std::fclose(rlog);
    kfx_keyframes_destroy(keyframes);
  }
  std::printf("end! %d frames, frame_count %d, %.3f ms/frame in kfx_pipeline (host frames, PCIe incl.)\n", n,
              frames, n ? 1e3 * gpu_s / n : 0.0);
  kfx_destroy(ctx);
  kfx_dataset_close(ds);
  return 0;
}
