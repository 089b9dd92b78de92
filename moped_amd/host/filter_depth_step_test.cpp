// filter_depth_step_test -- FILTER_PROJECTION_DEPTH_HIP driven the way moped3d's pipeline drives a FILTER slot: the
// active algorithm of the step runs on a FrameData that holds matches, objects, a depth map and (optionally) its
// ".distance" map (tests/test_gpu_filter_depth_host.py):
//   filter_depth_step_test in.bin [TestSampleSize2]
// With a second sample size: TWO instances, FILTER (TestSampleSize) and FILTER2 (TestSampleSize2), over TWO frames with
// the same input (instance k selects its points on rand() seeded with seed + k) -- both share the session's device context, each must run on its own sample in both frames.  The
// output then has a "STEP frame slot" line before every block (slot 0 FILTER, 1 FILTER2).
// in.bin (little endian):
//   int32   w, h, n_models, n_obj, TestSampleSize, MinPoints, srand seed, has_distance, has_depth
//   float32 K[4], cam[7] of the colour image; K[4], cam[7] of the depth map;
//           FeatureDistance, PlausibleSqDistance, MinScore, DepthFraction, MinKeypointFraction
//   per model: int32 n_keypoints, float32 xyz[n][3]; int32 n_matches, float32 (u, v, x, y, z)[n]
//   int32 obj_model[n_obj]; float32 obj_pose[n_obj][7]
//   float32 depth[h][w][4] (has_depth); float32 distance[h][w] (has_distance)
// A model's keypoints are split over two descriptor types ("SIFT" the first half, "SURF" the rest): the step must walk
// them in map order.  Prints
//   CAPABLE c / OBJECTS n / OBJ <index in the input list> <score bits> / CLUSTER m k <members...>
#define MOPED_AMD_WITH_DEPTH
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "moped_types.hpp"
#include "FILTER_PROJECTION_DEPTH_HIP.hpp"

using namespace MopedNS;

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s in.bin\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int32_t head[9];
  float fl[27];
  if (!rd(f, head, sizeof head) || !rd(f, fl, sizeof fl)) return 2;
  const int w = head[0], h = head[1], nm = head[2], nobj = head[3];
  vector<SP_Model> models;
  FrameData frameData;
  frameData.matches.resize(nm);
  for (int m = 0; m < nm; ++m) {
    SP_Model model(new Model);
    model->name = "model" + toString(m);
    int32_t n = 0;
    if (!rd(f, &n, 4)) return 2;
    vector<float> xyz(3 * (size_t)n);
    if (!rd(f, xyz.empty() ? 0 : &xyz[0], xyz.size() * 4)) return 2;
    for (int k = 0; k < n; ++k) {
      Model::IP ip;
      ip.coord3D.init(xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]);
      model->IPs[k < n / 2 ? "SIFT" : "SURF"].push_back(ip);
    }
    if (!rd(f, &n, 4)) return 2;
    vector<float> mt(5 * (size_t)n);
    if (!rd(f, mt.empty() ? 0 : &mt[0], mt.size() * 4)) return 2;
    for (int k = 0; k < n; ++k) {
      FrameData::Match match;
      match.imageIdx = 0;
      match.coord2D.init(mt[5 * k], mt[5 * k + 1]);
      match.coord3D.init(mt[5 * k + 2], mt[5 * k + 3], mt[5 * k + 4]);
      frameData.matches[m].push_back(match);
    }
    models.push_back(model);
  }
  vector<int32_t> om(nobj);
  vector<float> op(7 * (size_t)nobj);
  if (!rd(f, om.empty() ? 0 : &om[0], om.size() * 4) || !rd(f, op.empty() ? 0 : &op[0], op.size() * 4)) return 2;
  list<SP_Object> objects;
  vector<Object*> input;
  vector<SP_Object> inputObjects;
  for (int o = 0; o < nobj; ++o) {
    SP_Object obj(new Object);
    obj->model = models[om[o]];
    obj->pose.rotation.init(op[7 * o], op[7 * o + 1], op[7 * o + 2], op[7 * o + 3]);
    obj->pose.translation.init(op[7 * o + 4], op[7 * o + 5], op[7 * o + 6]);
    obj->score = 0;
    inputObjects.push_back(obj);
    input.push_back(obj.get());
  }
  frameData.objects = &objects;
  SP_Image gray(new Image);
  gray->imageType = IMAGE_TYPE_GRAY_IMAGE;
  gray->name = "camera";
  gray->width = 640;
  gray->height = 480;
  for (int j = 0; j < 4; ++j) gray->intrinsicLinearCalibration[j] = fl[j];
  for (int j = 0; j < 4; ++j) gray->cameraPose.rotation[j] = fl[4 + j];
  for (int j = 0; j < 3; ++j) gray->cameraPose.translation[j] = fl[8 + j];
  frameData.images.push_back(gray);
  if (head[8]) {
    SP_Image depth(new Image);
    depth->imageType = IMAGE_TYPE_DEPTH_MAP;
    depth->name = "camera.depth";
    depth->width = w;
    depth->height = h;
    for (int j = 0; j < 4; ++j) depth->intrinsicLinearCalibration[j] = fl[11 + j];
    for (int j = 0; j < 4; ++j) depth->cameraPose.rotation[j] = fl[15 + j];
    for (int j = 0; j < 3; ++j) depth->cameraPose.translation[j] = fl[19 + j];
    depth->data.resize((size_t)w * h * 4 * sizeof(Float));
    if (!rd(f, &depth->data[0], depth->data.size())) return 2;
    frameData.images.push_back(depth);
    if (head[7]) {
      SP_Image dist(new Image);
      dist->imageType = IMAGE_TYPE_PROB_MAP;
      dist->name = "camera.depth.distance";
      dist->width = w;
      dist->height = h;
      dist->data.resize((size_t)w * h * sizeof(Float));
      if (!rd(f, &dist->data[0], dist->data.size())) return 2;
      frameData.images.push_back(dist);
    }
  }
  std::fclose(f);

  const int second = argc > 2 ? std::atoi(argv[2]) : 0;
  MopedPipeline pipeline;
  pipeline.addAlg("FILTER", new FILTER_PROJECTION_DEPTH_HIP(head[5], fl[22], fl[23], fl[24], fl[25], head[4], fl[26]));
  if (second > 0)
    pipeline.addAlg("FILTER2", new FILTER_PROJECTION_DEPTH_HIP(head[5], fl[22], fl[23], fl[24], fl[25], second, fl[26]));
  list<MopedAlg*> algs = pipeline.getAlgs(true);
  if (algs.empty()) {
    std::fprintf(stderr, "FILTER: no gfx950 device / HIP library -- not capable\n");
    return 3;
  }
  for (list<MopedAlg*>::iterator a = algs.begin(); a != algs.end(); ++a) (*a)->modelsUpdated(models);
  for (int frame = 0; frame < (second > 0 ? 2 : 1); ++frame) {
    objects.assign(inputObjects.begin(), inputObjects.end());   // the same input list for every frame
    frameData.clusters.clear();
    int slot = 0;
    for (list<MopedAlg*>::iterator a = algs.begin(); a != algs.end(); ++a, ++slot) {
      // the step selects its test points in its first process(): every instance from a stream of its own, seeded here
      // (what the device runtime draws from rand() while it loads kernels is then no part of it)
      if (frame == 0) std::srand((unsigned)(head[6] + slot));
      (*a)->process(frameData);
      if (second > 0) std::printf("STEP %d %d\n", frame, slot);
      std::printf("CAPABLE %d\n", (int)(*a)->isCapable());
      std::printf("OBJECTS %d\n", (int)objects.size());
      for (list<SP_Object>::iterator it = objects.begin(); it != objects.end(); ++it) {
        int idx = 0;
        while (input[idx] != it->get()) ++idx;
        uint32_t bits;
        std::memcpy(&bits, &(*it)->score, 4);
        std::printf("OBJ %d %08x\n", idx, bits);
      }
      for (size_t m = 0; m < frameData.clusters.size(); ++m)
        for (size_t k = 0; k < frameData.clusters[m].size(); ++k) {
          std::printf("CLUSTER %d %d", (int)m, (int)k);
          for (FrameData::Cluster::iterator i = frameData.clusters[m][k].begin(); i != frameData.clusters[m][k].end(); ++i)
            std::printf(" %d", *i);
          std::printf("\n");
        }
    }
  }
  return 0;
}
