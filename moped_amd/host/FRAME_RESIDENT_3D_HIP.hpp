// FRAME_RESIDENT_3D_HIP -- moped3d only: ONE step for a Kinect frame's whole hot path, what DEPTHFILL, SIFT, DEPTHFILTER,
// MATCH_SIFT, DEPTHFILTER2, DEPTHPROP, CLUSTER, POSE, FILTER, POSE2 and FILTER2 of moped3d's pipeline
// (moped3d/libmoped/src/config.hpp:39-49) do one after the other, in one call of the C ABI (mh_frame_run_kinect_host):
// the gray image and the depth map go up once, the chain of kernels runs stream-ordered on the device, the objects come
// back -- what FRAME_RESIDENT_HIP is to moped2.  A maintainer who does not need the intermediate lists on the host
// replaces those addAlg lines by
//     pipeline.addAlg( "DEPTHFILL", new FRAME_RESIDENT_3D_HIP( 8, false,  128, "SIFT",  64, 0.05,
//                                                              0.6, 0.75, 0.65, 0.8, 150, 50,  0.01,
//                                                              0.1, 7, 2, 1, -1, -1,
//                                                              1024, 4, 5, 6, 8, 0.5,  6, 4096., 2,
//                                                              1024, 4, 6, 8, 5,       8, 8192., 1e-4 ) );
// (the reference constructors' arguments in pipeline order: DEPTH_FILL_EXACT's two; the descriptor; DEPTHFILTER's PatchSize
// and Density; MATCH_ADAPTIVE's six; DEPTHFILTER2's Density -- one PatchSize serves both filters, as in config.hpp;
// CLUSTER_LINKAGE's Cutoff, MinPts, Use3DFilter, LinkageType, Sigma2D, Sigma3D; POSE's NHypotheses and the reference's
// four + Alpha; FILTER's three; POSE2's five; FILTER2's three) and keeps the step-by-step plugins for pipelines that read
// lists in between.  Update() is MATCH_ADAPTIVE_BRUTE_HIP's (HipAdaptiveModels): database upload + control points, which
// become the ratio table of mh_frame_set_depth_rules.  Seeds as FRAME_RESIDENT_HIP's.
// Contract kept: reads the frame's gray image, depth map (filled in place, its ".distance" map appended to
// frameData.images as DEPTH_FILL_EXACT_CPU::process does; FillScale 0: the maps arrive filled, an existing ".distance"
// map is read); appends the frame's final objects {model, pose, score} to *frameData.objects in FILTER2's list order;
// fills frameData.matches (per model, ascending feature order: imageIdx, coord2D, coord3D, depthData) from the device's
// lists; frameData.clusters is sized to models->size() and left empty, like FRAME_RESIDENT_HIP's (the clusters never
// leave the device; counts() says how many there were).  detectedFeatures stays as it was: the keypoints are made and
// consumed on the device.  capable = false without a gfx950 device, as for every HIP step.
#pragma once
#include "MATCH_ADAPTIVE_BRUTE_HIP.hpp"

namespace MopedNS {

class FRAME_RESIDENT_3D_HIP : public MopedAlg {
  int FillScale;
  bool Bilinear;
  int DescriptorSize;
  string DescriptorType;
  int PatchSize;
  Float Density1, Density2;
  HipAdaptiveModels am;
  mh_linkage_params lk;
  mh_frame_params prm;
  Float Alpha;
  int Kind;
  int MaxKeypoints, DoubleImSize;   // config keys: keypoint capacity of the frame (2048), libsiftfast's DoubleImSize (1)
  int IncrementalModels;
  int LevelFill;   // config key: the frame's DEPTHFILL in MH_DEPTH_FILL_LEVELS mode (FillScale 4, 2, 1; 1280 x 960 frames)
  int LinkageRowMaxima;   // config key: the frame's CLUSTER in MH_LINKAGE_ROWMAX mode (match lists of up to 4096 per model)
  // config keys: the frame's CLUSTER as CLUSTER_WEIGHTED_MEAN_SHIFT_CPU instead of the linkage class (ClusterWeighted 1) with
  // that class's Radius, Merge, MinPts, MaxIterations, halfWeightDistance (mh_frame_set_cluster_wms); clusters[model] is
  // then filled too (the clusters may overlap)
  int ClusterWeighted;
  mh_wms_params wp;
  // config keys: DEPTH_VERIFY_CPU behind FILTER2 (DepthVerify 1) with that class's FeatureDistance, MaxMultiplier,
  // MaxDistance, DepthFraction (mh_frame_set_depth_verify): the objects the reference's step would erase are not delivered
  int DepthVerify;
  mh_depth_verify_params vp;
  unsigned long frameCounter;
  int32_t lastCounts[4];

  void Update(FrameData& frameData) {
    if (am.update(models, DescriptorType, IncrementalModels, frameData)) configUpdated = false;
  }

 public:
  FRAME_RESIDENT_3D_HIP(int FillScale, bool Bilinear, int DescriptorSize, string DescriptorType,                  // DEPTHFILL, SIFT
                        int PatchSize, Float Density1,                                                             // DEPTHFILTER
                        Float MinRatioMin, Float MinRatioMax, Float MaxRatioMin, Float MaxRatioMax, Float DimensionPeak,
                        Float DimensionFade,                                                                       // MATCH_SIFT
                        Float Density2,                                                                            // DEPTHFILTER2
                        Float Cutoff, int MinPts, int Use3DFilter, int LinkageType, Float Sigma2D, Float Sigma3D,  // CLUSTER
                        int NHyp1, int MaxObj1, int NPtsAlign1, int MinNPts1, Float ErrorThreshold1, Float Alpha,  // POSE
                        int MinPoints1, Float FeatureDistance1, Float MinScore1,                                   // FILTER
                        int NHyp2, int MaxObj2, int NPtsAlign2, int MinNPts2, Float ErrorThreshold2,               // POSE2
                        int MinPoints2, Float FeatureDistance2, Float MinScore2)                                   // FILTER2
      : FillScale(FillScale), Bilinear(Bilinear), DescriptorSize(DescriptorSize), DescriptorType(DescriptorType),
        PatchSize(PatchSize), Density1(Density1), Density2(Density2),
        am(MinRatioMin, MinRatioMax, MaxRatioMin, MaxRatioMax, DimensionPeak, DimensionFade), Alpha(Alpha),
        Kind(MH_DEPTH_BACKPROJECTION), MaxKeypoints(2048), DoubleImSize(1), IncrementalModels(0), LevelFill(0), LinkageRowMaxima(0), ClusterWeighted(0), DepthVerify(0), frameCounter(0) {
    vp.feature_distance = 64.f;
    vp.max_multiplier = 3.f;
    vp.max_distance = 2.f;
    vp.depth_fraction = 0.1f;
    wp.radius = 0.1f;
    wp.merge = 0.02f;
    wp.min_pts = 7;
    wp.max_iter = 100;
    wp.half_weight_distance = 10.f;
    lk.cutoff = (float)Cutoff;
    lk.min_pts = MinPts;
    lk.use3d_filter = Use3DFilter;
    lk.sigma2d = (float)Sigma2D;
    lk.sigma3d = (float)Sigma3D;
    lk.linkage_type = LinkageType;
    mh_frame_default_params(&prm);
    hipStageParams(prm, 1, NHyp1, MaxObj1, NPtsAlign1, MinNPts1, ErrorThreshold1, MinPoints1, FeatureDistance1, MinScore1);
    hipStageParams(prm, 2, NHyp2, MaxObj2, NPtsAlign2, MinNPts2, ErrorThreshold2, MinPoints2, FeatureDistance2, MinScore2);
    prm.run_stage2 = 1;
    for (int j = 0; j < 4; ++j) lastCounts[j] = 0;
    capable = (DescriptorSize == MH_DESC_DIM) && PatchSize > 0 && LinkageType >= 0 && LinkageType <= 2 && FillScale >= -1 &&
              HipSession::get() != 0;
  }

  const vector<float>& table() const { return am.controlPoints; }
  // the last frame's accepted matches, clusters, objects after POSE, objects after FILTER2 (mh_frame_fetch's counts)
  const int32_t* counts() const { return lastCounts; }

  void getConfig(map<string, string>& config) const {
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "DescriptorType", DescriptorType);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "DescriptorSize", DescriptorSize);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "scaleFactor", FillScale);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "PatchSize", PatchSize);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "Density", Density1);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "Density2", Density2);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "Cutoff", lk.cutoff);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "MinPts", lk.min_pts);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "NHypotheses", prm.pose1.n_hypotheses);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "NHypotheses2", prm.pose2.n_hypotheses);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "MaxKeypoints", MaxKeypoints);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "DoubleImSize", DoubleImSize);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "LevelFill", LevelFill);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "LinkageRowMaxima", LinkageRowMaxima);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeighted", ClusterWeighted);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeightedRadius", wp.radius);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeightedMerge", wp.merge);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeightedMinPts", wp.min_pts);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeightedMaxIterations", wp.max_iter);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeightedHalfWeightDistance", wp.half_weight_distance);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "DepthVerify", DepthVerify);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "VerifyFeatureDistance", vp.feature_distance);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "VerifyMaxMultiplier", vp.max_multiplier);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "VerifyMaxDistance", vp.max_distance);
    hipGetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "VerifyDepthFraction", vp.depth_fraction);
  }
  void setConfig(map<string, string>& config) {
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "Density", Density1);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "Density2", Density2);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "MaxKeypoints", MaxKeypoints);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "DoubleImSize", DoubleImSize);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "IncrementalModels", IncrementalModels);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "LevelFill", LevelFill);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "LinkageRowMaxima", LinkageRowMaxima);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeighted", ClusterWeighted);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeightedRadius", wp.radius);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeightedMerge", wp.merge);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeightedMinPts", wp.min_pts);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeightedMaxIterations", wp.max_iter);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "ClusterWeightedHalfWeightDistance", wp.half_weight_distance);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "DepthVerify", DepthVerify);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "VerifyFeatureDistance", vp.feature_distance);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "VerifyMaxMultiplier", vp.max_multiplier);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "VerifyMaxDistance", vp.max_distance);
    hipSetConfig(config, _stepName, _alg, "FRAME_RESIDENT_3D_HIP", "VerifyDepthFraction", vp.depth_fraction);
  }

  void process(FrameData& frameData) {
    if (configUpdated) Update(frameData);
    ++frameCounter;
    if (am.skipCalculation) return;
    Image* gray = 0;   // the FIRST gray image of the frame
    Image *depthmap, *distanceMap;
    int grayIdx = -1;
    for (size_t i = 0; i < frameData.images.size() && !gray; ++i)
      if (frameData.images[i]->imageType == IMAGE_TYPE_GRAY_IMAGE) { gray = frameData.images[i].get(); grayIdx = (int)i; }
    if (!hipFindDepthMaps(frameData, false, depthmap, distanceMap) || !gray) return;
    const int w = gray->width, h = gray->height;
    const size_t px = (size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0);
    if (px == 0 || depthmap->width != w || depthmap->height != h || gray->data.size() < px ||
        depthmap->data.size() < px * 4 * sizeof(Float)) {
      std::clog << "[moped_hip] FRAME_RESIDENT_3D_HIP: the gray image and the depth map must have one size: frame skipped" << std::endl;
      return;
    }
    if (distanceMap && distanceMap->data.size() < px * sizeof(Float)) distanceMap = 0;
    const bool fill = FillScale != 0;
    SP_Image filled;
    if (fill) {   // DEPTH_FILL_EXACT_CPU::process appends the map's distance map to the frame
      filled = SP_Image(new Image);
      filled->imageType = IMAGE_TYPE_PROB_MAP;
      filled->width = w;
      filled->height = h;
      filled->name = depthmap->name + ".distance";
      filled->data.resize(px * sizeof(Float));
      distanceMap = filled.get();
    }
    mh_ctx* ctx = HipSession::get();
    HipHandover::get().drop();
    HipDepthMaps::get().drop();
    // the rules and the clusterer of this pipeline (the session's context is shared with whatever else the host runs)
    float K[4];
    for (int j = 0; j < 4; ++j) K[j] = depthmap->intrinsicLinearCalibration[j];
    mh_depth_rules rules;
    rules.patch_size = PatchSize;
    rules.feature_density = (float)Density1;
    rules.match_density = (float)Density2;
    rules.ratio_table = am.controlPoints.empty() ? 0 : &am.controlPoints[0];
    rules.n_models = (int32_t)models->size();
    rules.maximum_depth = 4.0f;   // MATCH_ADAPTIVE_FLANN_CPU.hpp:107-109
    rules.default_depth = 1.0f;
    rules.cauchy_scale = 0.1f;
    if (mh_frame_set_depth_rules(ctx, &rules, K) != MH_OK) { HipSession::warn("mh_frame_set_depth_rules"); return; }
    if (mh_frame_set_cluster_linkage(ctx, &lk) != MH_OK) { HipSession::warn("mh_frame_set_cluster_linkage"); return; }
    // (set after the linkage class: the one set last is on)
    if (ClusterWeighted && mh_frame_set_cluster_wms(ctx, &wp) != MH_OK) { HipSession::warn("mh_frame_set_cluster_wms"); return; }
    const mh_cam cam = hipCamOf(*gray);
    const mh_cam depthCam = hipCamOf(*depthmap);
    if (DepthVerify && mh_frame_set_depth_verify(ctx, &vp, &depthCam) != MH_OK) { HipSession::warn("mh_frame_set_depth_verify"); return; }
    vector<mh_object> out(256);
    int32_t n = 0;
    int32_t* const counts = lastCounts;
    for (int j = 0; j < 4; ++j) counts[j] = 0;
    int fillModeBefore = MH_DEPTH_FILL_REPLAY;   // the session's context is shared: its mode is put back afterwards
    mh_depth_fill_get_mode(ctx, &fillModeBefore);
    if (LevelFill) mh_depth_fill_set_mode(ctx, MH_DEPTH_FILL_LEVELS);
    int linkageModeBefore = MH_LINKAGE_SCAN;
    mh_linkage_get_mode(ctx, &linkageModeBefore);
    if (LinkageRowMaxima) mh_linkage_set_mode(ctx, MH_LINKAGE_ROWMAX);
    int rc = mh_frame_run_kinect_host(ctx, &gray->data[0], (float*)&depthmap->data[0],
                                      distanceMap ? (float*)&distanceMap->data[0] : 0, w, h, DoubleImSize, MaxKeypoints, &cam,
                                      &prm, FillScale, Bilinear ? 1 : 0, Kind, (float)Alpha,
                                      Kind == MH_DEPTH_BACKPROJECTION ? 0.1f : 25.f,
                                      (uint64_t)frameCounter * 2654435761ul + _alg, &out[0], (int)out.size(), &n, counts);
    if (rc == MH_OK && n > (int)out.size()) {   // more objects than the first guess: the frame's results are still there
      out.resize(n);
      rc = mh_frame_fetch(ctx, &out[0], (int)out.size(), &n, counts);
    }
    // the context goes back to a plain one: another mh_frame_* user of the session must not inherit this pipeline's front end
    struct Restore {
      mh_ctx* ctx;
      int fillMode, linkageMode;
      ~Restore() {
        mh_frame_set_depth_rules(ctx, 0, 0);
        mh_frame_set_cluster_linkage(ctx, 0);
        mh_frame_set_cluster_wms(ctx, 0);
        mh_frame_set_depth_verify(ctx, 0, 0);
        mh_frame_set_depth_image(ctx, 0, 0, 0, 0, 0, 0.5f, 0.1f);
        mh_depth_fill_set_mode(ctx, fillMode);
        mh_linkage_set_mode(ctx, linkageMode);
      }
    } restore = {ctx, fillModeBefore, linkageModeBefore};
    if (rc != MH_OK) { HipSession::warn("mh_frame_run_kinect_host"); return; }
    if (fill) frameData.images.push_back(filled);
    // frameData.matches as the steps up to DEPTHPROP leave it, from the device's lists
    frameData.matches.clear();
    frameData.matches.resize(models->size());
    frameData.clusters.clear();
    frameData.clusters.resize(models->size());
    const int M = counts[0] > 0 ? counts[0] : 0;
    if (M > 0) {
      vector<int32_t> mq(M), mm(M);
      vector<mh_corr> pts(M);
      vector<mh_depth_info> info(M);
      vector<float> uv(2 * (size_t)M);
      int32_t nm = 0, np = 0;
      if (mh_frame_fetch_matches(ctx, &mq[0], &mm[0], M, &nm) != MH_OK || mh_frame_fetch_match_points(ctx, &pts[0], M, &np) != MH_OK ||
          nm != M || np != M) {
        HipSession::warn("mh_frame_fetch_matches");
      } else {
        for (int k = 0; k < M; ++k) { uv[2 * k] = pts[k].u; uv[2 * k + 1] = pts[k].v; }
        const bool have = mh_depth_prop(ctx, 0, 0, 0, 0, &uv[0], M, &info[0]) == MH_OK;   // (the context still holds the maps)
        if (!have) HipSession::warn("mh_depth_prop");
        for (int k = 0; k < M; ++k) {
          if (mm[k] < 0 || mm[k] >= (int)models->size()) continue;
          FrameData::Match mt;
          mt.imageIdx = grayIdx;
          mt.coord2D.init(pts[k].u, pts[k].v);
          mt.coord3D.init(pts[k].x, pts[k].y, pts[k].z);
          mt.depthData.depthValid = have && info[k].depth_valid != 0;
          mt.depthData.coord3D.init(have ? info[k].coord3d[0] : 0.f, have ? info[k].coord3d[1] : 0.f, have ? info[k].coord3d[2] : 0.f);
          mt.depthData.depth = have ? info[k].depth : 0.f;
          mt.depthData.fillDistance = have ? info[k].fill_distance : -1.f;
          frameData.matches[mm[k]].push_back(mt);
        }
      }
    }
    // the weighted mean shift's clusters: member indices inside the model's match list, as the CLUSTER step leaves them
    if (ClusterWeighted && M > 0 && counts[1] > 0) {
      vector<int32_t> cm(counts[1]), co((size_t)counts[1] + 1), mem((size_t)MH_WMS_MEMBER_FACTOR * M);
      int32_t nc = 0;
      if (mh_frame_debug_fetch_clusters_slot(ctx, 0, &cm[0], &co[0], &mem[0], counts[1], (int)mem.size(), &nc) != MH_OK) {
        HipSession::warn("mh_frame_debug_fetch_clusters_slot");
      } else {
        for (int k = 0; k < nc; ++k) {
          if (cm[k] < 0 || cm[k] >= (int)models->size()) continue;
          frameData.clusters[cm[k]].resize(frameData.clusters[cm[k]].size() + 1);
          FrameData::Cluster& cl = frameData.clusters[cm[k]].back();
          for (int j = co[k]; j < co[k + 1]; ++j) cl.push_back(mem[j]);
        }
      }
    }
    for (int o = 0; o < n && o < (int)out.size(); ++o)
      if (out[o].model >= 0 && out[o].model < (int)models->size())
        hipAppendObject(frameData, (*models)[out[o].model], out[o].pose, out[o].score);
  }
};

}  // namespace MopedNS
