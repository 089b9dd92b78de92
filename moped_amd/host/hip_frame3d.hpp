// moped3d only (Image::imageType): what the depth steps look up in a FrameData before they call the C ABI.
// C++98-clean and free of HIP headers, like hip_session.hpp.
#pragma once
#include "hip_session.hpp"

namespace MopedNS {

// The frame's depth map and its fill-distance map, the IMAGE_TYPE_PROB_MAP image named "<depth map's name>.distance"
// (the first of that name; NULL if there is none).  firstDepthMap: CLUSTER_LINKAGE_CPU's loop stops at the first depth
// map (CLUSTER_LINKAGE_CPU.hpp:577-593), every other reference step keeps the LAST one (DEPTHFILTER_CPU.hpp:122-127
// has no break).  false: the frame has no depth map.
inline bool hipFindDepthMaps(FrameData& frameData, bool firstDepthMap, Image*& depthmap, Image*& distanceMap) {
  depthmap = 0;
  distanceMap = 0;
  for (size_t i = 0; i < frameData.images.size(); ++i)
    if (frameData.images[i]->imageType == IMAGE_TYPE_DEPTH_MAP) {
      depthmap = frameData.images[i].get();
      if (firstDepthMap) break;
    }
  if (!depthmap) return false;
  for (size_t i = 0; i < frameData.images.size(); ++i)
    if (frameData.images[i]->imageType == IMAGE_TYPE_PROB_MAP && frameData.images[i]->name == depthmap->name + ".distance") {
      distanceMap = frameData.images[i].get();
      break;
    }
  return true;
}

}  // namespace MopedNS
