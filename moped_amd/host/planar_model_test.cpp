// planar_model_test -- samples/createModels/createModels.cpp on the device, and the model it makes put to use:
//
//   planar_model_test image.gray width height name out_dir
//
// image.gray = width x height raw 8-bit pixels.  The image becomes a planar model through
// createPlanarModelsFromImages_HIP (scale = 0.8 / fx: the plane 0.8 in front of the camera); the tree is printed to
// <out_dir>/<name>.moped.xml as createModels.cpp:121-126 does; the file is read back with mh_models_add_xml and uploaded;
// the same image then runs as a frame (mh_frame_enqueue_image).  Prints
//   MODEL <name> ROWS n / FILE <path> / LOADED <name> ROWS n / FRAME KEYPOINTS n MATCHES m OBJECTS k /
//   OBJ model score n_points qx qy qz qw tx ty tz      (one per object)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "moped_types.hpp"

#include "planar_models_hip.hpp"

using namespace MopedNS;

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: planar_model_test image.gray width height name out_dir\n");
    return 2;
  }
  const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
  const std::string name = argv[4], path = std::string(argv[5]) + "/" + name + ".moped.xml";
  if (w <= 0 || h <= 0) return 2;
  SP_Image image(new Image);
  image->name = name;
  image->width = w;
  image->height = h;
  image->data.resize((size_t)w * h);
  image->intrinsicLinearCalibration.init(800.f, 800.f, 320.f, 240.f);
  image->intrinsicNonlinearCalibration.init(0.f, 0.f, 0.f, 0.f);
  image->cameraPose.rotation.init(0.f, 0.f, 0.f, 1.f);
  image->cameraPose.translation.init(0.f, 0.f, 0.f);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(&image->data[0], 1, image->data.size(), f) != image->data.size()) {
    std::perror(argv[1]);
    return 2;
  }
  std::fclose(f);
  mh_ctx* ctx = HipSession::get();
  if (!ctx) return 3;   // no device

  // teach
  vector<SP_Image> images(1, image);
  const Float scale = 0.8f / image->intrinsicLinearCalibration[0];
  vector<shared_ptr<sXML> > xmls = createPlanarModelsFromImages_HIP(ctx, images, scale);
  if (xmls.size() != 1) return 4;
  std::printf("MODEL %s ROWS %zu\n", (*xmls[0])["name"].c_str(), xmls[0]->children[0].children.size());
  {
    std::ofstream out(path.c_str());
    xmls[0]->print(out);
    if (!out) return 5;
  }
  std::printf("FILE %s\n", path.c_str());

  // load it back and make it the database
  mh_model_set* set = 0;
  if (mh_models_create(&set, 0) != MH_OK || mh_models_add_xml(set, path.c_str()) != MH_OK) {
    std::fprintf(stderr, "%s\n", set ? mh_models_last_error(set) : "mh_models_create");
    return 6;
  }
  std::printf("LOADED %s ROWS %lld\n", mh_models_name(set, 0), (long long)mh_models_rows(set));
  if (mh_db_upload_models(ctx, set, 0, 1) != MH_OK || mh_reserve(ctx, 8192, 1024, 4096) != MH_OK) {
    HipSession::warn("mh_db_upload_models");
    return 7;
  }
  mh_models_destroy(set);

  // the same image as a frame
  void* gray = 0;
  if (mh_host_alloc(ctx, image->data.size(), &gray) != MH_OK) return 8;
  std::memcpy(gray, &image->data[0], image->data.size());
  const mh_cam cam = hipCamOf(*image);
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
