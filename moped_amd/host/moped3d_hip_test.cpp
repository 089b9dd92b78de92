// moped3d_hip_test -- stand-alone driver for moped3d's (Kinect) pipeline through its STEP plugins, in the shape of
// moped_hip_test: a MopedPipeline wired as moped3d/libmoped/src/config.hpp:38-49 with the HIP classes in the slots, fed a
// scene file (models + one frame: features or a gray image, the depth map, optionally its distance map), the frame's
// lists printed after every step so that a test can hold each step against the oracle.
//
//   moped3d_hip_test [--resident] [--loop N] [--maps-out file] [--level-fill] [--linkage-rowmax] scene.bin
//       --resident       the same scene through FRAME_RESIDENT_3D_HIP (one step, mh_frame_run_kinect_host)
//       --level-fill     DEPTHFILL in MH_DEPTH_FILL_LEVELS mode (DEPTH_FILL_EXACT_HIP's levelFill, the one-step plugin's LevelFill key)
//       --cluster-wms R M MinPts MaxIter HWD   CLUSTER_WEIGHTED_MEAN_SHIFT_HIP with these arguments in the CLUSTER slot of the
//                        step wiring, or -- with --resident -- as FRAME_RESIDENT_3D_HIP's ClusterWeighted... keys (moped3d's
//                        other depth-aware clusterer)
//       --linkage-rowmax CLUSTER in MH_LINKAGE_ROWMAX mode (CLUSTER_LINKAGE_HIP's RowMaxima key, the one-step plugin's LinkageRowMaxima)
//       --depth-verify FD MM MD DF   DEPTH_VERIFY_HIP( FeatureDistance, MaxMultiplier, MaxDistance, DepthFraction ) behind
//                        FILTER2 in the step wiring, or -- with --resident -- FRAME_RESIDENT_3D_HIP's DepthVerify / Verify... keys
//       --loop N         the frame N times; prints FPS (process() time only), the lists of the last frame
//       --maps-out file  the frame's depth map [h][w][4] and distance map [h][w] (floats) as the steps left them
//
// Scene file (little endian, written by scripts/dump_scene.py dump_kinect):
//   int32 n_models, Q, width, height, has_image, has_distance, patch_size, fill_scale, max_keypoints
//   float feature_density, match_density ; float K[4] ; float cam[7]
//   per model: int32 n_pts ; float xyz[n_pts][3] ; float desc[n_pts][128]      (boundingBox = the points' extent)
//   float q_uv[Q][2] ; float q_desc[Q][128]                                    (Q = 0: FEAT runs on the image)
//   uint8 gray[height][width] if has_image ; float depth[height][width][4] ; float distance[height][width] if has_distance
//
// Output, after every step (line "STEP <name>"), whatever the frame holds at that point:
//   MATCH m q u v x y z          matches[m] in list order; q = the feature with that coord2D (-1: none); hex floats
//   DEPTH m k valid x y z depth fillDistance      depthData of matches[m][k] (after DEPTHPROP), hex floats
//   CLUSTER m c i0 i1 ...        clusters[m][c], members in order
//   OBJ m tx ty tz qx qy qz qw score              objects in list order, hex floats
// and once: CONTROL m a b c d (the four control points of model m, hex floats), COUNTS (--resident: mh_frame_fetch's).
#define MOPED_AMD_WITH_DEPTH 1
#include <cstdio>
#include <cstring>
#include <ctime>
#include <iostream>

#include "moped_types.hpp"

#include "DEPTH_FILL_EXACT_HIP.hpp"
#include "FEAT_SIFT_HIP.hpp"
#include "DEPTHFILTER_HIP.hpp"
#include "MATCH_ADAPTIVE_BRUTE_HIP.hpp"
#include "DEPTHMAP_PROP_HIP.hpp"
#include "CLUSTER_LINKAGE_HIP.hpp"
#include "CLUSTER_WEIGHTED_MEAN_SHIFT_HIP.hpp"
#include "POSE_RANSAC_P3P_DEPTH_HIP.hpp"
#include "FILTER_PROJECTION_HIP.hpp"
#include "DEPTH_VERIFY_HIP.hpp"
#include "FRAME_RESIDENT_3D_HIP.hpp"

using namespace MopedNS;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

struct Scene {
  int32_t nm, Q, w, h, has_image, has_distance, patch, fill_scale, max_keypoints;
  float density1, density2, K[4], cam[7];
  vector<SP_Model> models;
  vector<float> uv, qd, depth, distance;
  vector<unsigned char> gray;
};

static bool load(const char* path, Scene& s) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::perror(path); return false; }
  int32_t head[9];
  if (!rd(f, head, 9) || !rd(f, &s.density1, 1) || !rd(f, &s.density2, 1) || !rd(f, s.K, 4) || !rd(f, s.cam, 7)) return false;
  s.nm = head[0]; s.Q = head[1]; s.w = head[2]; s.h = head[3]; s.has_image = head[4]; s.has_distance = head[5];
  s.patch = head[6]; s.fill_scale = head[7]; s.max_keypoints = head[8];
  if (s.nm < 0 || s.nm > 4096 || s.Q < 0 || s.w <= 0 || s.h <= 0 || s.w > 8192 || s.h > 8192) return false;
  for (int m = 0; m < s.nm; ++m) {
    int32_t n = 0;
    if (!rd(f, &n, 1) || n < 0) return false;
    vector<float> xyz((size_t)n * 3), desc((size_t)n * 128);
    if (!rd(f, xyz.empty() ? (float*)0 : &xyz[0], xyz.size()) || !rd(f, desc.empty() ? (float*)0 : &desc[0], desc.size())) return false;
    SP_Model model(new Model);
    model->name = "model" + toString(m);
    vector<Model::IP>& ips = model->IPs["SIFT"];
    ips.resize(n);
    for (int k = 0; k < 3; ++k) model->boundingBox[0][k] = model->boundingBox[1][k] = n > 0 ? xyz[k] : 0.f;
    for (int i = 0; i < n; ++i) {
      ips[i].coord3D.init(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
      ips[i].descriptor.assign(desc.begin() + (size_t)i * 128, desc.begin() + (size_t)(i + 1) * 128);
      for (int k = 0; k < 3; ++k) {
        if (xyz[3 * i + k] < model->boundingBox[0][k]) model->boundingBox[0][k] = xyz[3 * i + k];
        if (xyz[3 * i + k] > model->boundingBox[1][k]) model->boundingBox[1][k] = xyz[3 * i + k];
      }
    }
    s.models.push_back(model);
  }
  const size_t px = (size_t)s.w * s.h;
  s.uv.resize((size_t)s.Q * 2);
  s.qd.resize((size_t)s.Q * 128);
  s.gray.resize(s.has_image ? px : 0);
  s.depth.resize(px * 4);
  s.distance.resize(s.has_distance ? px : 0);
  const bool ok = rd(f, s.uv.empty() ? (float*)0 : &s.uv[0], s.uv.size()) && rd(f, s.qd.empty() ? (float*)0 : &s.qd[0], s.qd.size()) &&
                  rd(f, s.gray.empty() ? (unsigned char*)0 : &s.gray[0], s.gray.size()) && rd(f, &s.depth[0], s.depth.size()) &&
                  rd(f, s.distance.empty() ? (float*)0 : &s.distance[0], s.distance.size());
  std::fclose(f);
  return ok;
}

static SP_Image make_image(const Scene& s, Image_Type type, const char* name, const void* data, size_t bytes) {
  SP_Image image(new Image);
  image->imageType = type;
  image->name = name;
  image->width = s.w;
  image->height = s.h;
  image->intrinsicLinearCalibration.init(s.K[0], s.K[1], s.K[2], s.K[3]);
  image->intrinsicNonlinearCalibration.init(0.f, 0.f, 0.f, 0.f);
  image->cameraPose.rotation.init(s.cam[0], s.cam[1], s.cam[2], s.cam[3]);
  image->cameraPose.translation.init(s.cam[4], s.cam[5], s.cam[6]);
  image->data.resize(bytes);
  if (data && bytes) std::memcpy(&image->data[0], data, bytes);
  return image;
}

// moped3d/libmoped/src/config.hpp:38-49 with the HIP classes (UNDISTORTED_IMAGE: the scenes are undistorted)
// wms (--cluster-wms): Radius, Merge, MinPts, MaxIterations, halfWeightDistance of CLUSTER_WEIGHTED_MEAN_SHIFT_HIP in the
// CLUSTER slot instead (0 is returned then: the linkage step's own key has nobody to go to)
static CLUSTER_LINKAGE_HIP* createPipeline(MopedPipeline& pipeline, const Scene& s, bool level_fill, const double* wms,
                                           const double* verify) {
  CLUSTER_LINKAGE_HIP* cluster = wms ? 0 : new CLUSTER_LINKAGE_HIP(0.1, 7, 2, 1, 0.0, 1, -1, -1);
  if (s.fill_scale != 0) pipeline.addAlg("DEPTHFILL", new DEPTH_FILL_EXACT_HIP(s.fill_scale, false, level_fill));
  if (s.Q == 0 && s.has_image) pipeline.addAlg("SIFT", new FEAT_SIFT_HIP("-1"));
  pipeline.addAlg("DEPTHFILTER", new DEPTHFILTER_HIP(s.patch, s.density1, 1));
  pipeline.addAlg("MATCH_SIFT", new MATCH_ADAPTIVE_BRUTE_HIP(128, "SIFT", 0.6, 0.75, 0.65, 0.8, 150, 50));
  pipeline.addAlg("DEPTHFILTER2", new DEPTHFILTER_HIP(s.patch, s.density2, 2));
  pipeline.addAlg("DEPTHPROP", new DEPTHMAP_PROP_HIP());
  if (wms) pipeline.addAlg("CLUSTER", new CLUSTER_WEIGHTED_MEAN_SHIFT_HIP(wms[0], wms[1], (unsigned)wms[2], (unsigned)wms[3], wms[4]));
  else pipeline.addAlg("CLUSTER", cluster);
  pipeline.addAlg("POSE", new POSE_RANSAC_P3P_DEPTH_HIP(1024, 4, 5, 6, 8, 0.5));
  pipeline.addAlg("FILTER", new FILTER_PROJECTION_HIP(6, 4096., 2));
  pipeline.addAlg("POSE2", new POSE_RANSAC_P3P_DEPTH_HIP(1024, 4, 6, 8, 5, 0.5));
  pipeline.addAlg("FILTER2", new FILTER_PROJECTION_HIP(8, 8192., 1e-4));
  if (verify) pipeline.addAlg("DEPTH_VERIFY", new DEPTH_VERIFY_HIP(verify[0], verify[1], verify[2], verify[3]));
  return cluster;
}

static FRAME_RESIDENT_3D_HIP* createResidentPipeline(MopedPipeline& pipeline, const Scene& s) {
  FRAME_RESIDENT_3D_HIP* alg = new FRAME_RESIDENT_3D_HIP(s.fill_scale, false, 128, "SIFT", s.patch, s.density1, 0.6, 0.75, 0.65, 0.8,
                                                         150, 50, s.density2, 0.1, 7, 2, 1, -1, -1, 1024, 4, 5, 6, 8, 0.5, 6, 4096.,
                                                         2, 1024, 4, 6, 8, 5, 8, 8192., 1e-4);
  pipeline.addAlg("DEPTHFILL", alg);
  return alg;
}

static int model_index(const vector<SP_Model>& models, const SP_Model& m) {
  for (size_t i = 0; i < models.size(); ++i)
    if (models[i].get() == m.get()) return (int)i;
  return -1;
}

static void print_frame(const char* step, const FrameData& fd, const Scene& s, const vector<SP_Model>& models) {
  std::printf("STEP %s\n", step);
  for (size_t m = 0; m < fd.matches.size(); ++m)
    for (size_t k = 0; k < fd.matches[m].size(); ++k) {
      const FrameData::Match& x = fd.matches[m][k];
      int q = -1;
      for (int i = 0; i < s.Q && q < 0; ++i)
        if (s.uv[2 * i] == x.coord2D[0] && s.uv[2 * i + 1] == x.coord2D[1]) q = i;
      std::printf("MATCH %zu %d %a %a %a %a %a\n", m, q, x.coord2D[0], x.coord2D[1], x.coord3D[0], x.coord3D[1], x.coord3D[2]);
    }
  if (std::strcmp(step, "DEPTHPROP") == 0 || std::strcmp(step, "DEPTHFILL") == 0)
    for (size_t m = 0; m < fd.matches.size(); ++m)
      for (size_t k = 0; k < fd.matches[m].size(); ++k) {
        const depthInformation& d = fd.matches[m][k].depthData;
        std::printf("DEPTH %zu %zu %d %a %a %a %a %a\n", m, k, d.depthValid ? 1 : 0, d.coord3D[0], d.coord3D[1], d.coord3D[2], d.depth,
                    d.fillDistance);
      }
  for (size_t m = 0; m < fd.clusters.size(); ++m)
    for (size_t c = 0; c < fd.clusters[m].size(); ++c) {
      std::printf("CLUSTER %zu %zu", m, c);
      for (FrameData::Cluster::const_iterator it = fd.clusters[m][c].begin(); it != fd.clusters[m][c].end(); ++it) std::printf(" %d", *it);
      std::printf("\n");
    }
  for (list<SP_Object>::const_iterator o = fd.objects->begin(); o != fd.objects->end(); ++o)
    std::printf("OBJ %d %a %a %a %a %a %a %a %a\n", model_index(models, (*o)->model), (*o)->pose.translation[0],
                (*o)->pose.translation[1], (*o)->pose.translation[2], (*o)->pose.rotation[0], (*o)->pose.rotation[1],
                (*o)->pose.rotation[2], (*o)->pose.rotation[3], (*o)->score);
}

int main(int argc, char** argv) {
  bool resident = false, level_fill = false, linkage_rowmax = false;
  int loop = 1;
  const char* maps_out = 0;
  double wms[5];
  bool cluster_wms = false;
  double verify[4];
  bool depth_verify = false;
  int a = 1;
  for (; a < argc && argv[a][0] == '-'; ++a) {
    if (std::string(argv[a]) == "--resident") resident = true;
    else if (std::string(argv[a]) == "--level-fill") level_fill = true;
    else if (std::string(argv[a]) == "--linkage-rowmax") linkage_rowmax = true;
    else if (std::string(argv[a]) == "--loop" && a + 1 < argc) loop = std::atoi(argv[++a]);
    else if (std::string(argv[a]) == "--maps-out" && a + 1 < argc) maps_out = argv[++a];
    else if (std::string(argv[a]) == "--cluster-wms" && a + 5 < argc) {
      cluster_wms = true;
      for (int k = 0; k < 5; ++k) wms[k] = std::atof(argv[++a]);
    }
    else if (std::string(argv[a]) == "--depth-verify" && a + 4 < argc) {
      depth_verify = true;
      for (int k = 0; k < 4; ++k) verify[k] = std::atof(argv[++a]);
    }
    else { a = argc; break; }   // an option nobody knows, or one without its value
  }
  if (a + 1 != argc || loop < 1) {
    std::fprintf(stderr, "usage: %s [--resident] [--loop N] [--maps-out file] [--level-fill] [--linkage-rowmax] [--cluster-wms R M MinPts MaxIter HWD] [--depth-verify FD MM MD DF] scene.bin\n", argv[0]);
    return 2;
  }
  if (cluster_wms && (linkage_rowmax || wms[2] < 0 || wms[3] < 0)) {
    std::fprintf(stderr, "--cluster-wms: without --linkage-rowmax, MinPts and MaxIter >= 0\n");
    return 2;
  }
  Scene s;
  if (!load(argv[a], s)) {
    std::fprintf(stderr, "%s: not a scene file of dump_kinect\n", argv[a]);
    return 2;
  }
  if (resident && !s.has_image) {
    std::fprintf(stderr, "--resident needs a scene with an image (FEAT runs on the device)\n");
    return 2;
  }
  MopedPipeline pipeline;
  FRAME_RESIDENT_3D_HIP* res = 0;
  CLUSTER_LINKAGE_HIP* cluster = 0;
  if (resident) res = createResidentPipeline(pipeline, s);
  else cluster = createPipeline(pipeline, s, level_fill, cluster_wms ? wms : 0, depth_verify ? verify : 0);
  list<MopedAlg*> all = pipeline.getAlgs();
  map<string, string> config;
  for (list<MopedAlg*>::iterator it = all.begin(); it != all.end(); ++it) {
    if (!(*it)->isCapable()) {
      std::fprintf(stderr, "step %s: no gfx950 device / HIP library -- not capable\n", (*it)->_stepName.c_str());
      return 3;
    }
    (*it)->modelsUpdated(s.models);
    (*it)->getConfig(config);
  }
  if (res) {
    config["DEPTHFILL:0:FRAME_RESIDENT_3D_HIP/MaxKeypoints"] = toString(s.max_keypoints);
    if (level_fill) config["DEPTHFILL:0:FRAME_RESIDENT_3D_HIP/LevelFill"] = "1";
    if (linkage_rowmax) config["DEPTHFILL:0:FRAME_RESIDENT_3D_HIP/LinkageRowMaxima"] = "1";
    if (cluster_wms) {
      static const char* const keys[5] = {"Radius", "Merge", "MinPts", "MaxIterations", "HalfWeightDistance"};
      config["DEPTHFILL:0:FRAME_RESIDENT_3D_HIP/ClusterWeighted"] = "1";
      for (int k = 0; k < 5; ++k)
        config[std::string("DEPTHFILL:0:FRAME_RESIDENT_3D_HIP/ClusterWeighted") + keys[k]] = toString(k == 2 || k == 3 ? (double)(int)wms[k] : wms[k]);
    }
    if (depth_verify) {
      static const char* const vkeys[4] = {"VerifyFeatureDistance", "VerifyMaxMultiplier", "VerifyMaxDistance", "VerifyDepthFraction"};
      config["DEPTHFILL:0:FRAME_RESIDENT_3D_HIP/DepthVerify"] = "1";
      for (int k = 0; k < 4; ++k) config[std::string("DEPTHFILL:0:FRAME_RESIDENT_3D_HIP/") + vkeys[k]] = toString(verify[k]);
    }
    res->setConfig(config);
  }
  if (cluster && linkage_rowmax) {
    config["CLUSTER:0:CLUSTER_LINKAGE_HIP/RowMaxima"] = "1";
    cluster->setConfig(config);
  }
  std::printf("CONFIG_KEYS %zu\n", config.size());

  list<SP_Object> objects;
  double total = 0;
  for (int rep = 0; rep < loop; ++rep) {
    const bool last = rep == loop - 1;
    objects.clear();
    FrameData frameData;
    frameData.objects = &objects;
    // FrameData::images as moped3d.cpp builds them: the gray image, the depth map, (a map that arrives filled: its distance map)
    frameData.images.push_back(make_image(s, IMAGE_TYPE_GRAY_IMAGE, "camera", s.gray.empty() ? 0 : &s.gray[0],
                                          s.gray.empty() ? (size_t)s.w * s.h : s.gray.size()));
    frameData.images.push_back(make_image(s, IMAGE_TYPE_DEPTH_MAP, "depth", &s.depth[0], s.depth.size() * sizeof(float)));
    if (s.has_distance)
      frameData.images.push_back(make_image(s, IMAGE_TYPE_PROB_MAP, "depth.distance", &s.distance[0], s.distance.size() * sizeof(float)));
    if (s.Q > 0) {
      vector<FrameData::DetectedFeature>& feats = frameData.detectedFeatures["SIFT"];
      feats.resize(s.Q);
      for (int i = 0; i < s.Q; ++i) {
        feats[i].imageIdx = 0;
        feats[i].coord2D.init(s.uv[2 * i], s.uv[2 * i + 1]);
        feats[i].descriptor.assign(s.qd.begin() + (size_t)i * 128, s.qd.begin() + (size_t)(i + 1) * 128);
      }
    }
    list<MopedAlg*> algs = pipeline.getAlgs(true);
    for (list<MopedAlg*>::iterator it = algs.begin(); it != algs.end(); ++it) {
      struct timespec t0, t1;
      clock_gettime(CLOCK_REALTIME, &t0);
      (*it)->process(frameData);
      clock_gettime(CLOCK_REALTIME, &t1);
      if (rep > 0 || loop == 1) total += (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
      if (last) {
        std::printf("FEATURES %zu\n", frameData.detectedFeatures["SIFT"].size());
        print_frame((*it)->_stepName.c_str(), frameData, s, s.models);
      }
    }
    if (last && maps_out) {
      FILE* f = std::fopen(maps_out, "wb");
      if (!f) { std::perror(maps_out); return 2; }
      for (size_t i = 0; i < frameData.images.size(); ++i)
        if (frameData.images[i]->imageType != IMAGE_TYPE_GRAY_IMAGE)
          std::fwrite(&frameData.images[i]->data[0], 1, frameData.images[i]->data.size(), f);
      std::fclose(f);
    }
  }
  if (res) {
    const vector<float>& t = res->table();
    for (size_t m = 0; 4 * m + 3 < t.size(); ++m) std::printf("CONTROL %zu %a %a %a %a\n", m, t[4 * m], t[4 * m + 1], t[4 * m + 2], t[4 * m + 3]);
    std::printf("COUNTS %d %d %d %d\n", res->counts()[0], res->counts()[1], res->counts()[2], res->counts()[3]);
  } else {
    for (list<MopedAlg*>::iterator it = all.begin(); it != all.end(); ++it)
      if (MATCH_ADAPTIVE_BRUTE_HIP* mt = dynamic_cast<MATCH_ADAPTIVE_BRUTE_HIP*>(*it)) {
        const vector<float>& t = mt->table();
        for (size_t m = 0; 4 * m + 3 < t.size(); ++m) std::printf("CONTROL %zu %a %a %a %a\n", m, t[4 * m], t[4 * m + 1], t[4 * m + 2], t[4 * m + 3]);
      }
  }
  std::printf("DEPTH_MAP_UPLOADS %lu FRAMES %d\n", HipDepthMaps::get().uploads, loop);
  const int timed = loop > 1 ? loop - 1 : 1;
  std::printf("FPS %.2f\n", total > 0 ? timed / total : 0.0);
  return 0;
}
