// DEPTHMAP_PROP_HIP -- moped3d only: drop-in for DEPTHMAP_PROP_CPU
// (moped3d/libmoped/src/depthprop/DEPTHMAP_PROP_CPU.hpp, config.hpp:44):
//     pipeline.addAlg( "DEPTHPROP", new DEPTHMAP_PROP_HIP() );
//     pipeline.addAlg( "DEPTHPROP", new DEPTHMAP_PROP_CPU() );   // fallback
// Fills Match::depthData (src/util.hpp:73-84) of every match from the pixel ((int) u, (int) v) of the frame's depth map:
// coord3D, depth, depthValid, and fillDistance from the map's ".distance" map or -1 (:98-113, 119-132).  The lookups run
// on the device copy of the map the frame's depth steps share (mh_depth_prop; HipDepthMaps), one call for all models.
#pragma once
#include "hip_frame3d.hpp"

namespace MopedNS {

class DEPTHMAP_PROP_HIP : public MopedAlg {
 public:
  DEPTHMAP_PROP_HIP() { capable = HipSession::get() != 0; }

  void getConfig(map<string, string>&) const {}
  void setConfig(map<string, string>&) {}

  void process(FrameData& frameData) {
    if (frameData.images.size() < 2) return;   // :54-58
    Image* gray = 0;
    Image *depthmap, *distanceMap;
    for (size_t i = 0; i < frameData.images.size(); ++i)   // the last of each kind (:62-72)
      if (frameData.images[i]->imageType == IMAGE_TYPE_GRAY_IMAGE) gray = frameData.images[i].get();
    if (!hipFindDepthMaps(frameData, false, depthmap, distanceMap) || !gray) return;   // :75-77
    if (gray->width != depthmap->width || gray->height != depthmap->height) return;   // :80-83
    vector<float> uv;
    for (size_t m = 0; m < frameData.matches.size(); ++m)
      for (size_t k = 0; k < frameData.matches[m].size(); ++k) {
        uv.push_back(frameData.matches[m][k].coord2D[0]);
        uv.push_back(frameData.matches[m][k].coord2D[1]);
      }
    const int n = (int)(uv.size() / 2);
    if (n == 0) return;
    mh_ctx* ctx = HipSession::get();
    if (!HipDepthMaps::get().ensure(ctx, depthmap, distanceMap)) {
      HipSession::warn("mh_frame_set_depth_image_host");
      return;
    }
    vector<mh_depth_info> info(n);
    if (mh_depth_prop(ctx, 0, 0, 0, 0, &uv[0], n, &info[0]) != MH_OK) {
      HipSession::warn("mh_depth_prop");
      return;
    }
    size_t x = 0;
    for (size_t m = 0; m < frameData.matches.size(); ++m)
      for (size_t k = 0; k < frameData.matches[m].size(); ++k, ++x) {
        depthInformation& d = frameData.matches[m][k].depthData;
        d.depthValid = info[x].depth_valid != 0;
        d.coord3D.init(info[x].coord3d[0], info[x].coord3d[1], info[x].coord3d[2]);
        d.depth = info[x].depth;
        d.fillDistance = info[x].fill_distance;
      }
  }
};

}  // namespace MopedNS
