// DEPTH_VERIFY_HIP -- moped3d only: drop-in for DEPTH_VERIFY_CPU
// (moped3d/libmoped/src/depthVerify/DEPTH_VERIFY_CPU.hpp), same four constructor arguments in the same order:
//     pipeline.addAlg( "DEPTH_VERIFY", new DEPTH_VERIFY_HIP( 64., 3., 2., 0.1 ) );
// The reference's check of every object that left FILTER2 against the Kinect map (:86-208): a quality score QS over all
// matches of the object's model, an "incorrect score" IS over all keypoints of the model projected into the depth camera,
// the object erased if IS > QS.  The whole step is one call, mh_depth_verify (include/moped_hip.h): objects, matches and
// the maps go over, nine words per object come back, the model's keypoints never leave the device.
//
// The keypoints are the rows of the RESIDENT database: the one the MATCH step of the pipeline uploaded for its
// DescriptorType (HipModelTable, hip_session.hpp -- MATCH_BRUTE_HIP, MATCH_ADAPTIVE_BRUTE_HIP and FRAME_RESIDENT_3D_HIP all
// leave it on the session's context), one slice per model in model order.  The reference walks the keypoints of every
// descriptor type; with one type per model the two agree.  Without a resident database for models->size() models the
// call is refused, the step says so and leaves the objects as they are.
// A frame without a depth map (the reference dereferences a null image there): the step says so and declares itself not
// capable.  A depth map without its ".distance" map (the reference would crash as well): no distance test.  Frames
// whose matches refer to several images are left alone in the same way.  Objects whose model is not in the list are
// skipped, as the reference skips them (:138-140).
#pragma once
#include "hip_frame3d.hpp"

namespace MopedNS {

class DEPTH_VERIFY_HIP : public MopedAlg {
  Float FeatureDistance;
  Float MaxMultiplier;
  Float MaxDistance;
  Float DepthFraction;

 public:
  DEPTH_VERIFY_HIP(Float FeatureDistance, Float MaxMultiplier, Float MaxDistance, Float DepthFraction)
      : FeatureDistance(FeatureDistance), MaxMultiplier(MaxMultiplier), MaxDistance(MaxDistance), DepthFraction(DepthFraction) {
    capable = HipSession::get() != 0;
  }

  void getConfig(map<string, string>& config) const {   // the keys the reference publishes (:68-75)
    hipGetConfig(config, _stepName, _alg, "DEPTH_VERIFY_HIP", "FeatureDistance", FeatureDistance);
    hipGetConfig(config, _stepName, _alg, "DEPTH_VERIFY_HIP", "MaxMultiplier", MaxMultiplier);
    hipGetConfig(config, _stepName, _alg, "DEPTH_VERIFY_HIP", "MaxDistance", MaxDistance);
    hipGetConfig(config, _stepName, _alg, "DEPTH_VERIFY_HIP", "DepthFraction", DepthFraction);
  }
  void setConfig(map<string, string>& config) {          // (:77-84)
    hipSetConfig(config, _stepName, _alg, "DEPTH_VERIFY_HIP", "FeatureDistance", FeatureDistance);
    hipSetConfig(config, _stepName, _alg, "DEPTH_VERIFY_HIP", "MaxMultiplier", MaxMultiplier);
    hipSetConfig(config, _stepName, _alg, "DEPTH_VERIFY_HIP", "MaxDistance", MaxDistance);
    hipSetConfig(config, _stepName, _alg, "DEPTH_VERIFY_HIP", "DepthFraction", DepthFraction);
  }

  // the verdicts of the last process(), one record per object that was examined, in list order
  vector<mh_verify_record> lastRecords;

  void process(FrameData& frameData) {
    mh_ctx* ctx = HipSession::get();
    lastRecords.clear();
    if (models->empty() || !frameData.objects) return;
    vector<vector<FrameData::Match> >& matches = frameData.matches;
    if (matches.size() < models->size()) return;      // the reference's sanity check (:93-95)

    // the depth map and its fill-distance image (:98-116)
    Image *depthmap, *distanceMap;
    if (!hipFindDepthMaps(frameData, false, depthmap, distanceMap) || depthmap->width <= 0 || depthmap->height <= 0 ||
        depthmap->data.size() < (size_t)depthmap->width * depthmap->height * 4 * sizeof(Float)) {
      std::clog << "[moped_hip] DEPTH_VERIFY_HIP: the frame has no depth map: the step is not capable" << std::endl;
      capable = false;
      return;
    }
    if (distanceMap && distanceMap->data.size() < (size_t)depthmap->width * depthmap->height * sizeof(Float)) distanceMap = 0;

    const int nm = (int)models->size();
    const HipCameraTable table(frameData);
    if (!table.ok) return;
    if (table.cams.size() > 1) {
      std::clog << "[moped_hip] DEPTH_VERIFY_HIP: matches from several images: the step is not capable" << std::endl;
      capable = false;
      return;
    }
    // the objects in list order (:118), each with its model's index (:123-127)
    vector<list<SP_Object>::iterator> its;
    vector<int32_t> objModel;
    vector<float> objPose;
    for (list<SP_Object>::iterator it = frameData.objects->begin(); it != frameData.objects->end(); ++it) {
      int modelNum = -1;
      for (int m = 0; m < nm; ++m)
        if ((*it)->model->name == (*models)[m]->name) modelNum = m;   // (the reference keeps the last of that name too)
      if (modelNum == -1) continue;                                   // :138-140
      its.push_back(it);
      objModel.push_back(modelNum);
      for (int i = 0; i < 4; ++i) objPose.push_back((*it)->pose.rotation[i]);
      for (int i = 0; i < 3; ++i) objPose.push_back((*it)->pose.translation[i]);
    }
    const int nobj = (int)its.size();
    if (nobj == 0) return;

    HipHandover::get().drop();
    HipDepthMaps::get().drop();   // (this step sets the context's map itself and clears it behind itself)
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
    mh_cam cam = depthCam;                              // (no match anywhere: no image is referred to; the camera is not read)
    if (!table.cams.empty()) cam = table.cams[0];
    const mh_depth_verify_params prm = {FeatureDistance, MaxMultiplier, MaxDistance, DepthFraction};
    lastRecords.resize(nobj);
    mh_corr none;
    const int rc = mh_depth_verify(ctx, corr.empty() ? &none : &corr[0], &off[0], nm, &objModel[0], &objPose[0], nobj, &cam,
                                   &depthCam, &prm, &lastRecords[0]);
    if (rc != MH_OK) HipSession::warn("mh_depth_verify");
    // the session's context goes back to "no depth map": a later mh_frame_* user of it must not inherit one
    mh_frame_set_depth_image_host(ctx, 0, 0, 0, 0, 0, 0.5f, 0.1f);
    if (rc != MH_OK) {
      lastRecords.clear();
      return;
    }
    for (int o = 0; o < nobj; ++o)
      if (!lastRecords[o].keep) frameData.objects->erase(its[o]);   // :204-206
  }
};

}  // namespace MopedNS
