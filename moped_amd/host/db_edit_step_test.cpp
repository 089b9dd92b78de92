// db_edit_step_test -- Moped::addModel / removeModel (src/moped.cpp:139-159) while frames flow, through the step plugins:
//
//   db_edit_step_test scene.bin <IncrementalModels: 0 | 1>
//
// scene.bin: scripts/dump_scene.py dump(), at least five models.  The host adds models 0, 1, 2 and runs a frame, removes
// the middle one and runs a frame, adds model 3's points under the known name "model2" (a replace) and runs a frame,
// adds model 4 (an append) and runs a frame.  Every change goes through modelsUpdated() like MopedPimpl's; with
// IncrementalModels = 1 MATCH_BRUTE_HIP::Update() edits the resident database instead of uploading all models again.
// Per frame it prints
//   FRAME f MODELS n MATCHES total TAG <hash of frameData.matches> / M <name> <matches> / OBJ <name> <pose> <score>
// and at the end FULL_UPLOADS / SPLICES as HipResidentModels counted them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "moped_types.hpp"

#include "CLUSTER_MEAN_SHIFT_HIP.hpp"
#include "FILTER_PROJECTION_HIP.hpp"
#include "MATCH_BRUTE_HIP.hpp"
#include "POSE_RANSAC_P3P_HIP.hpp"

using namespace MopedNS;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

static vector<SP_Model> g_models;
static list<MopedAlg*> g_algs;

static void models_updated() {   // src/moped.cpp:94-99
  for (list<MopedAlg*>::iterator a = g_algs.begin(); a != g_algs.end(); ++a) (*a)->modelsUpdated(g_models);
}
static void add_model(const SP_Model& model) {   // src/moped.cpp:139-150
  for (size_t i = 0; i < g_models.size(); ++i)
    if (g_models[i]->name == model->name) {
      g_models[i] = model;
      models_updated();
      return;
    }
  g_models.push_back(model);
  models_updated();
}
static void remove_model(const string& name) {   // src/moped.cpp:152-159
  for (size_t i = 0; i < g_models.size(); ++i)
    if (g_models[i]->name == name) {
      g_models.erase(g_models.begin() + i);
      models_updated();
      return;
    }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s scene.bin <IncrementalModels: 0 | 1>\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int32_t nm = 0, Q = 0;
  float K[4], cam[7];
  if (!rd(f, &nm, 1) || !rd(f, &Q, 1) || !rd(f, K, 4) || !rd(f, cam, 7) || nm < 5 || Q <= 0) return 2;
  SP_Image image(new Image);
  image->width = 640;
  image->height = 480;
  image->intrinsicLinearCalibration.init(K[0], K[1], K[2], K[3]);
  image->intrinsicNonlinearCalibration.init(0.f, 0.f, 0.f, 0.f);
  image->cameraPose.rotation.init(cam[0], cam[1], cam[2], cam[3]);
  image->cameraPose.translation.init(cam[4], cam[5], cam[6]);
  image->name = "camera";
  vector<SP_Model> all;
  for (int m = 0; m < nm; ++m) {
    int32_t n = 0;
    if (!rd(f, &n, 1) || n < 0) return 2;
    vector<float> xyz((size_t)n * 3), desc((size_t)n * 128);
    if (!rd(f, &xyz[0], xyz.size()) || !rd(f, &desc[0], desc.size())) return 2;
    SP_Model model(new Model);
    model->name = "model" + toString(m);
    vector<Model::IP>& ips = model->IPs["SIFT"];
    ips.resize(n);
    for (int i = 0; i < n; ++i) {
      ips[i].coord3D.init(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
      ips[i].descriptor.assign(desc.begin() + (size_t)i * 128, desc.begin() + (size_t)(i + 1) * 128);
    }
    all.push_back(model);
  }
  vector<float> uv((size_t)Q * 2), qd((size_t)Q * 128);
  if (!rd(f, &uv[0], uv.size()) || !rd(f, &qd[0], qd.size())) return 2;
  std::fclose(f);

  MopedPipeline pipeline;
  pipeline.addAlg("MATCH_SIFT", new MATCH_BRUTE_HIP(128, "SIFT", 0.8));
  pipeline.addAlg("CLUSTER", new CLUSTER_MEAN_SHIFT_HIP(200, 20, 7, 100));
  pipeline.addAlg("POSE", new POSE_RANSAC_P3P_HIP(1024, 4, 5, 6, 10));
  pipeline.addAlg("FILTER", new FILTER_PROJECTION_HIP(5, 4096., 2));
  pipeline.addAlg("POSE2", new POSE_RANSAC_P3P_HIP(1024, 4, 6, 8, 5));
  pipeline.addAlg("FILTER2", new FILTER_PROJECTION_HIP(7, 4096., 3));
  g_algs = pipeline.getAlgs();
  for (list<MopedAlg*>::iterator a = g_algs.begin(); a != g_algs.end(); ++a)
    if (!(*a)->isCapable()) {
      std::fprintf(stderr, "step %s: no gfx950 device / HIP library -- not capable\n", (*a)->_stepName.c_str());
      return 3;
    }
  map<string, string> config;
  config["MATCH_SIFT:0:MATCH_BRUTE_HIP/IncrementalModels"] = argv[2];
  for (list<MopedAlg*>::iterator a = g_algs.begin(); a != g_algs.end(); ++a) (*a)->setConfig(config);

  for (int frame = 0; frame < 4; ++frame) {
    if (frame == 0) {
      for (int m = 0; m < 3; ++m) add_model(all[m]);
    } else if (frame == 1) {
      remove_model("model1");
    } else if (frame == 2) {
      SP_Model again(new Model(*all[3]));   // a known name: replaces, keeps its index (:141-144)
      again->name = "model2";
      add_model(again);
    } else {
      add_model(all[4]);
    }
    list<SP_Object> objects;
    FrameData frameData;
    frameData.objects = &objects;
    frameData.images.push_back(image);
    vector<FrameData::DetectedFeature>& feats = frameData.detectedFeatures["SIFT"];
    feats.resize(Q);
    for (int i = 0; i < Q; ++i) {
      feats[i].imageIdx = 0;
      feats[i].coord2D.init(uv[2 * i], uv[2 * i + 1]);
      feats[i].descriptor.assign(qd.begin() + (size_t)i * 128, qd.begin() + (size_t)(i + 1) * 128);
    }
    list<MopedAlg*> algs = pipeline.getAlgs(true);
    for (list<MopedAlg*>::iterator a = algs.begin(); a != algs.end(); ++a) (*a)->process(frameData);
    size_t nmatch = 0;
    for (size_t m = 0; m < frameData.matches.size(); ++m) nmatch += frameData.matches[m].size();
    std::printf("FRAME %d MODELS %zu MATCHES %zu TAG %llx\n", frame, g_models.size(), nmatch, HipHandover::tagMatches(frameData));
    for (size_t m = 0; m < frameData.matches.size(); ++m)
      std::printf("M %s %zu\n", g_models[m]->name.c_str(), frameData.matches[m].size());
    for (list<SP_Object>::iterator o = objects.begin(); o != objects.end(); ++o)
      std::printf("OBJ %s %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", (*o)->model->name.c_str(),
                  (*o)->pose.translation[0], (*o)->pose.translation[1], (*o)->pose.translation[2],
                  (*o)->pose.rotation[0], (*o)->pose.rotation[1], (*o)->pose.rotation[2], (*o)->pose.rotation[3],
                  (*o)->score);
  }
  std::printf("FULL_UPLOADS %lu SPLICES %lu\n", HipResidentModels::get().fullUploads, HipResidentModels::get().splices);
  return 0;
}
