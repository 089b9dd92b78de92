// FILTER_PROJECTION_DEPTH_HIP -- moped3d only: drop-in for FILTER_PROJECTION_DEPTH_CPU
// (moped3d/libmoped/src/filter/FILTER_PROJECTION_DEPTH_CPU.hpp), same seven constructor arguments in the same order:
//     pipeline.addAlg( "FILTER2", new FILTER_PROJECTION_DEPTH_HIP( 8, 8192., 64., 1e-4, 0.1, 300, 0.1 ) );
//     pipeline.addAlg( "FILTER2", new FILTER_PROJECTION_HIP( 8, 8192., 1e-4 ) );   // takes the slot when a frame has no depth map
// FILTER_PROJECTION plus a test of every object's pose against the frame's depth map (:207-270): a sample of the model's
// own points is projected into the depth camera, and where the sensor measured a depth behind a point the object pays
// the Cauchy "incorrect score" IS; object->score = score - IS, MinScore is applied to that, keypoint ownership still
// goes by the projection score.  The whole step is one call, mh_filter_depth (include/moped_hip.h).
//
// TestPoints (:94-116) are chosen here, on the first process() and again whenever the model list has changed (the
// reference never re-selects: a model added later is tested with no points, one replaced with the old one's): all
// keypoints of the model over its descriptor types in map order when there are at most TestSampleSize, else the
// reference's randSample (:78-92) on the process's rand().  Every instance keeps its own sample and uploads it with
// every process(): the device context is shared by all HIP steps of the pipeline, so another instance of this class
// (FILTER beside FILTER2) or an edit of the resident DB by MATCH may have replaced or outdated what is there.
// A frame without a depth map (the reference dereferences a null image there): the step says so and declares itself
// not capable, the next algorithm registered under the slot takes over from the next frame on, this frame's objects
// stay as they are.  A depth map without its ".distance" map (the reference would crash as well): every pixel counts
// as measured.  Frames whose matches refer to several images are left to the step behind it in the same way.
#pragma once
#include <algorithm>
#include <utility>

#include "hip_frame3d.hpp"

namespace MopedNS {

class FILTER_PROJECTION_DEPTH_HIP : public MopedAlg {
  int MinPoints;
  Float FeatureDistance;
  Float PlausibleSqDistance;
  Float MinScore;
  Float DepthFraction;
  int TestSampleSize;
  Float MinKeypointFraction;

  // the test points as they were uploaded, and what they were chosen for
  vector<float> testXyz;
  vector<int32_t> testOff;
  vector<const Model*> chosenFor;
  vector<size_t> chosenCount;

  static size_t keypointCount(const Model& model) {
    size_t n = 0;
    for (map<string, vector<Model::IP> >::const_iterator it = model.IPs.begin(); it != model.IPs.end(); ++it) n += it->second.size();
    return n;
  }

  // randSample (:78-92): the population's indices prefixed with (Float) rand(), sorted; the first nSamples of them
  static void randSample(vector<int>& samples, int population, int nSamples) {
    vector<std::pair<Float, int> > randomSamples;
    for (int i = 0; i < population; i++) randomSamples.push_back(std::make_pair((Float)rand(), i));
    std::sort(randomSamples.begin(), randomSamples.end());
    for (int i = 0; i < nSamples && i < population; i++) samples.push_back(randomSamples[i].second);
  }

  bool modelsChanged() const {
    if (chosenFor.size() != models->size()) return true;
    for (size_t m = 0; m < models->size(); ++m)
      if (chosenFor[m] != (*models)[m].get() || chosenCount[m] != keypointCount(*(*models)[m])) return true;
    return false;
  }

  // selectTestPoints (:94-116)
  void selectTestPoints() {
    testXyz.clear();
    testOff.assign(1, 0);
    chosenFor.clear();
    chosenCount.clear();
    for (int modelNum = 0; modelNum < (int)models->size(); modelNum++) {
      const Model& model = *(*models)[modelNum];
      vector<const Model::IP*> keypoints;
      for (map<string, vector<Model::IP> >::const_iterator it = model.IPs.begin(); it != model.IPs.end(); ++it)
        for (size_t k = 0; k < it->second.size(); ++k) keypoints.push_back(&it->second[k]);
      vector<int> chosen;
      if ((int)keypoints.size() > TestSampleSize)
        randSample(chosen, (int)keypoints.size(), TestSampleSize);
      else
        for (int k = 0; k < (int)keypoints.size(); ++k) chosen.push_back(k);
      for (size_t k = 0; k < chosen.size(); ++k)
        for (int j = 0; j < 3; ++j) testXyz.push_back(keypoints[chosen[k]]->coord3D[j]);
      testOff.push_back((int32_t)(testXyz.size() / 3));
      chosenFor.push_back(&model);
      chosenCount.push_back(keypoints.size());
    }
  }

  // This instance's points onto the device, on EVERY process(): the context is the session's, shared by every HIP step
  // of the pipeline -- a FILTER and a FILTER2 instance of this class each hold their own sample (their own rand() draws,
  // perhaps another TestSampleSize) and each upload replaces the other's, and MATCH's edits of the resident DB make
  // whatever is there stale.  A few KB beside the depth map that crosses with them.
  bool uploadTestPoints(mh_ctx* ctx) {
    if (mh_filter_depth_set_points(ctx, testXyz.empty() ? 0 : &testXyz[0], &testOff[0], (int)testOff.size() - 1) != MH_OK) {
      HipSession::warn("mh_filter_depth_set_points");
      return false;
    }
    return true;
  }

 public:
  FILTER_PROJECTION_DEPTH_HIP(int MinPoints, Float FeatureDistance, Float PlausibleSqDistance, Float MinScore,
                              Float DepthFraction, int TestSampleSize, Float MinKeypointFraction)
      : MinPoints(MinPoints), FeatureDistance(FeatureDistance), PlausibleSqDistance(PlausibleSqDistance), MinScore(MinScore),
        DepthFraction(DepthFraction), TestSampleSize(TestSampleSize), MinKeypointFraction(MinKeypointFraction) {
    capable = HipSession::get() != 0;
  }

  void getConfig(map<string, string>& config) const {   // the keys the reference publishes (:118-127)
    hipGetConfig(config, _stepName, _alg, "FILTER_PROJECTION_DEPTH_HIP", "MinPoints", MinPoints);
    hipGetConfig(config, _stepName, _alg, "FILTER_PROJECTION_DEPTH_HIP", "FeatureDistance", FeatureDistance);
    hipGetConfig(config, _stepName, _alg, "FILTER_PROJECTION_DEPTH_HIP", "MinScore", MinScore);
    hipGetConfig(config, _stepName, _alg, "FILTER_PROJECTION_DEPTH_HIP", "PlausibleSqDistance", PlausibleSqDistance);
    hipGetConfig(config, _stepName, _alg, "FILTER_PROJECTION_DEPTH_HIP", "DepthFraction", DepthFraction);
    hipGetConfig(config, _stepName, _alg, "FILTER_PROJECTION_DEPTH_HIP", "TestSampleSize", TestSampleSize);
  }
  void setConfig(map<string, string>&) {}

  void process(FrameData& frameData) {
    mh_ctx* ctx = HipSession::get();
    if (models->empty()) return;
    if (modelsChanged()) selectTestPoints();          // :142-144

    vector<vector<FrameData::Match> >& matches = frameData.matches;
    if (matches.size() < models->size()) return;      // the reference's sanity check (:150-152)

    // the depth map and its fill-distance image (:155-173)
    Image *depthmap, *distanceMap;
    if (!hipFindDepthMaps(frameData, false, depthmap, distanceMap) || depthmap->width <= 0 || depthmap->height <= 0 ||
        depthmap->data.size() < (size_t)depthmap->width * depthmap->height * 4 * sizeof(Float)) {
      std::clog << "[moped_hip] FILTER_PROJECTION_DEPTH_HIP: the frame has no depth map: the step is not capable" << std::endl;
      capable = false;
      return;
    }
    if (distanceMap && distanceMap->data.size() < (size_t)depthmap->width * depthmap->height * sizeof(Float)) distanceMap = 0;

    const int nm = (int)models->size();
    const HipCameraTable table(frameData);
    if (!table.ok) return;
    if (table.cams.size() > 1) {
      std::clog << "[moped_hip] FILTER_PROJECTION_DEPTH_HIP: matches from several images: the step is not capable" << std::endl;
      capable = false;
      return;
    }
    HipHandover::get().drop();
    HipDepthMaps::get().drop();   // (this step sets the context's map itself and clears it behind itself)
    if (!uploadTestPoints(ctx)) return;
    if (mh_frame_set_depth_image_host(ctx, (const float*)&depthmap->data[0], distanceMap ? (const float*)&distanceMap->data[0] : 0,
                                      depthmap->width, depthmap->height, MH_DEPTH_BACKPROJECTION, 0.5f, 0.1f) != MH_OK) {
      HipSession::warn("mh_frame_set_depth_image_host");
      return;
    }
    const mh_cam depthCam = hipCamOf(*depthmap);

    vector<mh_corr> corr;
    vector<int32_t> off(nm + 1, 0);
    for (int m = 0; m < nm; ++m) {
      for (size_t k = 0; k < matches[m].size(); ++k) {
        mh_corr c;
        c.u = matches[m][k].coord2D[0]; c.v = matches[m][k].coord2D[1];
        c.x = matches[m][k].coord3D[0]; c.y = matches[m][k].coord3D[1]; c.z = matches[m][k].coord3D[2];
        corr.push_back(c);
      }
      off[m + 1] = (int32_t)corr.size();
    }
    // objects in (model, list) order -- the order the reference's double loop visits them (:182-184)
    vector<list<SP_Object>::iterator> its;
    vector<int32_t> objModel;
    vector<float> objPose;
    for (int m = 0; m < nm; ++m)
      for (list<SP_Object>::iterator it = frameData.objects->begin(); it != frameData.objects->end(); ++it)
        if ((*it)->model->name == (*models)[m]->name) {
          its.push_back(it);
          objModel.push_back(m);
          for (int i = 0; i < 4; ++i) objPose.push_back((*it)->pose.rotation[i]);
          for (int i = 0; i < 3; ++i) objPose.push_back((*it)->pose.translation[i]);
        }
    const int nobj = (int)its.size();
    frameData.clusters.clear();
    frameData.clusters.resize(nm);
    if (nobj == 0) return;
    mh_cam cam = depthCam;                              // (no match anywhere: no image is referred to; the camera is not read)
    if (!table.cams.empty()) cam = table.cams[0];
    const mh_filter_depth_params prm = {PlausibleSqDistance, DepthFraction, MinKeypointFraction};
    vector<float> score(nobj);
    vector<uint8_t> keep(nobj);
    vector<int32_t> order(nobj), members(corr.size() + 1), cloff(nobj + 1);
    mh_corr none;
    int32_t kept = 0;
    const int rc = mh_filter_depth(ctx, corr.empty() ? &none : &corr[0], &off[0], nm, &objModel[0], &objPose[0], nobj, &cam,
                                   MinPoints, FeatureDistance, MinScore, &depthCam, &prm, &score[0], &keep[0], &order[0],
                                   &members[0], &cloff[0], &kept, 0, 0, 0);
    if (rc != MH_OK) HipSession::warn("mh_filter_depth");
    // the session's context goes back to "no depth map": a later mh_frame_* user of it (FRAME_RESIDENT_HIP) must not
    // inherit a map and residual settings it never asked for
    mh_frame_set_depth_image_host(ctx, 0, 0, 0, 0, 0, 0.5f, 0.1f);
    if (rc != MH_OK) return;
    for (int o = 0; o < nobj; ++o) (*its[o])->score = score[o];
    for (int k = 0; k < kept; ++k) {
      const int o = order[k];
      FrameData::Cluster cl;
      for (int j = cloff[k]; j < cloff[k + 1]; ++j) cl.push_back(members[j]);
      frameData.clusters[objModel[o]].push_back(cl);
    }
    for (int o = 0; o < nobj; ++o)
      if (!keep[o]) frameData.objects->erase(its[o]);
  }
};

}  // namespace MopedNS
