// kinect_model_test -- a model taught from two Kinect views through createModelFromKinectViews_HIP, and put to use:
//
//   kinect_model_test [--merge] [--min-views K] view0.gray view0.depth view1.gray view1.depth width height name out_dir
//
// *.gray = width x height raw 8-bit pixels, *.depth = width x height x 4 raw floats (x, y, z, valid), the object's pose in
// both views the identity.  The first view becomes model 0 of an empty store, the second is appended without the
// keypoints the model holds already (merge ratio 0.8, 2 mm).  The model is saved through mh_models_add_rows +
// With --merge the second view goes in through createMergedModelFromKinectViews_HIP instead: the keypoints the model holds
// are folded into their rows, and with --min-views K the rows fewer than K views saw are dropped; a line
//   VIEWS n1 n2 ...        (rows seen by 1, 2, ... views)
// follows the MODEL line.  The model is saved through mh_models_add_rows +
// mh_models_write_xml to <out_dir>/<name>.moped.xml, the store's arrays are dumped to <out_dir>/store.{desc,xyz,model}
// (mh_db_debug_fetch), and view 0's image runs as a frame.  Prints
//   MODEL <name> INDEX i ROWS n BBOX x0 y0 z0 x1 y1 z1 / FILE <path> / STORE ROWS N MODELS m /
//   FRAME KEYPOINTS n MATCHES m OBJECTS k / OBJ model score n_points qx qy qz qw tx ty tz      (one per object)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "moped_types.hpp"

#include "kinect_models_hip.hpp"

using namespace MopedNS;

static bool read_file(const char* path, vector<unsigned char>& data, size_t bytes) {
  data.resize(bytes);
  FILE* f = std::fopen(path, "rb");
  const bool ok = f && std::fread(&data[0], 1, bytes, f) == bytes;
  if (f) std::fclose(f);
  if (!ok) std::perror(path);
  return ok;
}

static bool dump(mh_ctx* ctx, int which, size_t bytes, const std::string& path) {
  vector<unsigned char> buf(bytes ? bytes : 1);
  if (mh_db_debug_fetch(ctx, which, &buf[0], bytes) != MH_OK) return false;
  std::ofstream out(path.c_str(), std::ios::binary);
  out.write((const char*)&buf[0], (std::streamsize)bytes);
  return (bool)out;
}

int main(int argc, char** argv) {
  bool merge = false;
  int min_views = 1;
  while (argc > 1 && argv[1][0] == '-' && argv[1][1] == '-') {
    const std::string opt = argv[1];
    if (opt == "--merge") {
      merge = true;
      ++argv, --argc;
    } else if (opt == "--min-views" && argc > 2) {
      min_views = std::atoi(argv[2]);
      argv += 2, argc -= 2;
    } else {
      break;
    }
  }
  if (argc != 9 || min_views < 1 || (min_views > 1 && !merge)) {
    std::fprintf(stderr, "usage: kinect_model_test [--merge] [--min-views K] view0.gray view0.depth view1.gray view1.depth width height name out_dir\n"
                         "       (--min-views needs --merge)\n");
    return 2;
  }
  const int w = std::atoi(argv[5]), h = std::atoi(argv[6]);
  const std::string name = argv[7], dir = argv[8], path = dir + "/" + name + ".moped.xml";
  if (w <= 0 || h <= 0) return 2;
  vector<SP_Image> images, depthmaps;
  vector<Pose> poses;
  for (int v = 0; v < 2; ++v) {
    SP_Image image(new Image), depth(new Image);
    image->name = name;
    image->width = depth->width = w;
    image->height = depth->height = h;
    image->intrinsicLinearCalibration.init(800.f, 800.f, 320.f, 240.f);
    image->intrinsicNonlinearCalibration.init(0.f, 0.f, 0.f, 0.f);
    image->cameraPose.rotation.init(0.f, 0.f, 0.f, 1.f);
    image->cameraPose.translation.init(0.f, 0.f, 0.f);
    if (!read_file(argv[1 + 2 * v], image->data, (size_t)w * h) || !read_file(argv[2 + 2 * v], depth->data, (size_t)w * h * 16)) return 2;
    images.push_back(image);
    depthmaps.push_back(depth);
    Pose p;
    p.rotation.init(0.f, 0.f, 0.f, 1.f);
    p.translation.init(0.f, 0.f, 0.f);
    poses.push_back(p);
  }
  mh_ctx* ctx = HipSession::get();
  if (!ctx) return 3;   // no device

  // teach
  int index = -1;
  vector<int> views;
  SP_Model model = merge ? createMergedModelFromKinectViews_HIP(ctx, name, images, depthmaps, poses, min_views, &index, &views)
                         : createModelFromKinectViews_HIP(ctx, name, images, depthmaps, poses, &index);
  if (!model) return 4;
  const vector<Model::IP>& ips = model->IPs["SIFT"];
  std::printf("MODEL %s INDEX %d ROWS %zu BBOX %.9g %.9g %.9g %.9g %.9g %.9g\n", model->name.c_str(), index, ips.size(),
              model->boundingBox[0][0], model->boundingBox[0][1], model->boundingBox[0][2], model->boundingBox[1][0],
              model->boundingBox[1][1], model->boundingBox[1][2]);
  if (merge) {
    vector<int> seen(3, 0);   // [k]: rows k views saw
    for (size_t k = 0; k < views.size(); ++k) {
      if ((size_t)views[k] >= seen.size()) seen.resize(views[k] + 1, 0);
      ++seen[views[k]];
    }
    std::printf("VIEWS");
    for (size_t k = 1; k < seen.size(); ++k) std::printf(" %d", seen[k]);
    std::printf("\n");
  }

  // save it: the rows as the store got them
  {
    vector<float> desc(ips.size() * MH_DESC_DIM + 1), xyz(ips.size() * 3 + 1);
    for (size_t k = 0; k < ips.size(); ++k) {
      std::memcpy(&desc[k * MH_DESC_DIM], &ips[k].descriptor[0], MH_DESC_DIM * sizeof(float));
      for (int j = 0; j < 3; ++j) xyz[k * 3 + j] = ips[k].coord3D[j];
    }
    mh_model_set* set = 0;
    if (mh_models_create(&set, 0) != MH_OK || mh_models_add_rows(set, name.c_str(), &desc[0], &xyz[0], (int64_t)ips.size()) != MH_OK ||
        mh_models_write_xml(set, 0, path.c_str()) != MH_OK) {
      std::fprintf(stderr, "%s\n", set ? mh_models_last_error(set) : "mh_models_create");
      return 5;
    }
    mh_models_destroy(set);
  }
  std::printf("FILE %s\n", path.c_str());

  // the store it left
  int N = 0, n_models = 0;
  mh_db_size(ctx, &N, &n_models);
  const size_t n_pad = ((size_t)N + 127) / 128 * 128;
  if (!dump(ctx, 0, n_pad * MH_DESC_DIM * 4, dir + "/store.desc") || !dump(ctx, 2, (size_t)N * 12, dir + "/store.xyz") ||
      !dump(ctx, 3, (size_t)N * 4, dir + "/store.model")) {
    HipSession::warn("mh_db_debug_fetch");
    return 6;
  }
  std::printf("STORE ROWS %d MODELS %d\n", N, n_models);

  // view 0's image as a frame
  if (mh_reserve(ctx, 8192, 1024, 4096) != MH_OK) return 7;
  void* gray = 0;
  if (mh_host_alloc(ctx, images[0]->data.size(), &gray) != MH_OK) return 8;
  std::memcpy(gray, &images[0]->data[0], images[0]->data.size());
  const mh_cam cam = hipCamOf(*images[0]);
  mh_frame_params prm;
  mh_frame_default_params(&prm);
  vector<mh_object> objects(64);
  int32_t n_objects = 0, counts[4] = {0, 0, 0, 0}, n_keypoints = 0;
  if (mh_frame_enqueue_image(ctx, (const uint8_t*)gray, w, h, 1, 8192, &cam, &prm, 1) != MH_OK ||
      mh_frame_fetch(ctx, &objects[0], (int)objects.size(), &n_objects, counts) != MH_OK ||
      mh_frame_keypoints(ctx, &n_keypoints) != MH_OK) {
    HipSession::warn("mh_frame_enqueue_image");
    return 9;
  }
  mh_host_free(ctx, gray);
  std::printf("FRAME KEYPOINTS %d MATCHES %d OBJECTS %d\n", n_keypoints, counts[0], n_objects);
  for (int i = 0; i < n_objects; ++i) {
    const mh_object& o = objects[i];
    std::printf("OBJ %d %.9g %d %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", o.model, o.score, o.n_points, o.pose[0], o.pose[1], o.pose[2],
                o.pose[3], o.pose[4], o.pose[5], o.pose[6]);
  }
  return 0;
}
