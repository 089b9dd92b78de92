// DEPTHFILTER_HIP -- moped3d only: drop-in for DEPTHFILTER_CPU
// (moped3d/libmoped/src/depthfilter/DEPTHFILTER_CPU.hpp, config.hpp:41,43):
//     pipeline.addAlg( "DEPTHFILTER",  new DEPTHFILTER_HIP( 64, 0.05, 1 ) );
//     pipeline.addAlg( "DEPTHFILTER",  new DEPTHFILTER_CPU( 64, 0.05, 1 ) );   // fallback
//     pipeline.addAlg( "DEPTHFILTER2", new DEPTHFILTER_HIP( 64, 0.01, 2 ) );
//     pipeline.addAlg( "DEPTHFILTER2", new DEPTHFILTER_CPU( 64, 0.01, 2 ) );   // fallback
// Same constructor arguments: PatchSize, Density, ToFilter.  ToFilter = 1 rewrites detectedFeatures["SIFT"] (:180-214),
// ToFilter = 2 every matches[model] (:215-251): the entries whose patch density (of the features / of that model's
// matches, per square metre of scene surface at the patch's minimum depth, dilated 3x3) exceeds Density * 100 * 100
// stay, in their order.  The patch map and the verdicts come from the device (mh_depth_filter); the frame's depth map is
// uploaded once for the frame's depth steps (HipDepthMaps).  Coordinates outside the map count for the nearest patch (the
// reference indexes out of bounds there).
#pragma once
#include "hip_frame3d.hpp"

namespace MopedNS {

class DEPTHFILTER_HIP : public MopedAlg {
  int PatchSize;
  Float Density;
  int ToFilter;

 public:
  DEPTHFILTER_HIP(int PatchSize, Float Density, int ToFilter) : PatchSize(PatchSize), Density(Density), ToFilter(ToFilter) {
    capable = PatchSize > 0 && HipSession::get() != 0;
  }

  void getConfig(map<string, string>& config) const {
    hipGetConfig(config, _stepName, _alg, "DEPTHFILTER_HIP", "PatchSize", PatchSize);
    hipGetConfig(config, _stepName, _alg, "DEPTHFILTER_HIP", "Density", Density);
    hipGetConfig(config, _stepName, _alg, "DEPTHFILTER_HIP", "ToFilter", ToFilter);
  }
  void setConfig(map<string, string>&) {}

  void process(FrameData& frameData) {
    if (frameData.images.size() < 2) return;   // :117-119
    if (ToFilter != 1 && ToFilter != 2) return;
    // the LAST depth map of the frame (:122-127 has no break); its distance map is not read here, it rides along for
    // the frame's later depth steps
    Image *depthmap, *distanceMap;
    if (!hipFindDepthMaps(frameData, false, depthmap, distanceMap)) return;
    // the step's lists: one group (the features) or one per model (its matches)
    vector<float> uv;
    vector<int32_t> off(1, 0);
    vector<FrameData::DetectedFeature>* feats = 0;
    if (ToFilter == 1) {
      feats = &frameData.detectedFeatures["SIFT"];
      for (size_t i = 0; i < feats->size(); ++i) {
        uv.push_back((*feats)[i].coord2D[0]);
        uv.push_back((*feats)[i].coord2D[1]);
      }
      off.push_back((int32_t)feats->size());
    } else {
      for (size_t m = 0; m < frameData.matches.size(); ++m) {
        const vector<FrameData::Match>& mm = frameData.matches[m];
        for (size_t k = 0; k < mm.size(); ++k) {
          uv.push_back(mm[k].coord2D[0]);
          uv.push_back(mm[k].coord2D[1]);
        }
        off.push_back((int32_t)(uv.size() / 2));
      }
    }
    const int n = (int)(uv.size() / 2), groups = (int)off.size() - 1;
    if (n == 0) return;
    mh_ctx* ctx = HipSession::get();
    if (!HipDepthMaps::get().ensure(ctx, depthmap, distanceMap)) {
      HipSession::warn("mh_frame_set_depth_image_host");
      return;
    }
    float K[4];
    for (int j = 0; j < 4; ++j) K[j] = depthmap->intrinsicLinearCalibration[j];
    vector<uint8_t> keep(n);
    if (mh_depth_filter(ctx, 0, 0, 0, K, PatchSize, (float)Density, &uv[0], &off[0], groups, &keep[0]) != MH_OK) {
      HipSession::warn("mh_depth_filter");
      return;
    }
    if (ToFilter == 1) {
      vector<FrameData::DetectedFeature> kept;   // newCorresp (:198-213)
      for (int i = 0; i < n; ++i)
        if (keep[i]) kept.push_back((*feats)[i]);
      feats->swap(kept);
    } else {
      for (int m = 0; m < groups; ++m) {
        vector<FrameData::Match>& mm = frameData.matches[m];
        vector<FrameData::Match> kept;             // newMatches (:232-248)
        for (size_t k = 0; k < mm.size(); ++k)
          if (keep[off[m] + k]) kept.push_back(mm[k]);
        mm.swap(kept);
      }
    }
  }
};

}  // namespace MopedNS
