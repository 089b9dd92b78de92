// createPlanarModelsFromImages_HIP -- Moped::createPlanarModelsFromImages (src/moped.cpp:196-236) with the pipeline's
// front on the device: FEAT of all images as ONE batch (mh_sift_extract_batch_dev), ONE selection launch that turns every
// keypoint into a model point at (u scale, v scale, 0) in detectedFeatures order (mh_planar_rows_dev's batch form), then
// the tree of moped.cpp:211-233 built on the host -- one <Model name=image->name> per image with one <Points> child and
// one <Point p3d desc_type desc> per keypoint, numbers through toString (moped.hpp:359-360).  Same signature and result
// shape as the reference's call, the session in front:
//     vector<shared_ptr<sXML> > xmls = createPlanarModelsFromImages_HIP(HipSession::get(), images, scale);
//     xmls[i]->print(file);            // samples/createModels/createModels.cpp:121-126
// Differences: the images of one call have one size and there are at most MH_MAX_BATCH of them; no UNDISTORTED_IMAGE step
// runs (the reference runs whatever its pipeline holds); the descriptors are FEAT's, not renormalised by a MATCH step
// (include/moped_hip.h, mh_models_write_xml).  On an error the result is EMPTY (the reference cannot fail) and the reason
// goes to std::clog.  C++98-clean; the buffers are page-locked blocks of mh_host_alloc, which the device addresses.
#pragma once
#include "hip_session.hpp"

namespace MopedNS {

inline vector<shared_ptr<sXML> > createPlanarModelsFromImages_HIP(mh_ctx* session, vector<SP_Image>& images, Float scale,
                                                                  int doubleImSize = 1, int capacity = 8192,
                                                                  const string& descType = "SIFT") {
  vector<shared_ptr<sXML> > xmls;
  const int n = (int)images.size();
  if (!session || n <= 0 || n > MH_MAX_BATCH || capacity <= 0) {
    std::clog << "[moped_hip] createPlanarModelsFromImages_HIP: no session, or not 1.." << MH_MAX_BATCH << " images" << std::endl;
    return xmls;
  }
  const int w = images[0]->width, h = images[0]->height;
  for (int i = 0; i < n; ++i)
    if (images[i]->width != w || images[i]->height != h || w <= 0 || h <= 0 || images[i]->data.size() < (size_t)w * h) {
      std::clog << "[moped_hip] createPlanarModelsFromImages_HIP: the images of one call have one size" << std::endl;
      return xmls;
    }
  const size_t px = ((size_t)w * h + 15) / 16 * 16, rows = (size_t)n * capacity;
  // one block: images | FEAT's desc, xy | kept desc, xyz | boxes | counts, kept counts
  const size_t o_desc = n * px, o_xy = o_desc + rows * MH_DESC_DIM * 4, o_kd = (o_xy + rows * 2 * 4 + 15) / 16 * 16,
               o_kx = o_kd + rows * MH_DESC_DIM * 4, o_box = (o_kx + rows * 3 * 4 + 15) / 16 * 16, o_cnt = o_box + (size_t)n * 6 * 4,
               bytes = o_cnt + 2 * (size_t)n * 4;
  void* block = 0;
  if (mh_host_alloc(session, bytes, &block) != MH_OK) {
    std::clog << "[moped_hip] createPlanarModelsFromImages_HIP: " << mh_last_error(session) << std::endl;
    return xmls;
  }
  unsigned char* b = (unsigned char*)block;
  const uint8_t* gray[MH_MAX_BATCH];
  for (int i = 0; i < n; ++i) {
    std::memcpy(b + i * px, &images[i]->data[0], (size_t)w * h);
    gray[i] = b + i * px;
  }
  float* desc = (float*)(b + o_desc);
  float* xy = (float*)(b + o_xy);
  float* kd = (float*)(b + o_kd);
  float* kx = (float*)(b + o_kx);
  int32_t* counts = (int32_t*)(b + o_cnt);
  mh_planar_spec spec;
  std::memset(&spec, 0, sizeof spec);   // form 0, every keypoint, no limit
  spec.scale = scale;
  int rc = mh_sift_extract_batch_dev(session, gray, n, w, h, doubleImSize, desc, xy, capacity, counts);
  if (rc == MH_OK)
    rc = mh_planar_rows_batch_dev(session, desc, xy, counts, n, capacity, &spec, kd, kx, capacity, counts + n, (float*)(b + o_box));
  if (rc == MH_OK) rc = mh_synchronize(session);
  if (rc != MH_OK) {
    std::clog << "[moped_hip] createPlanarModelsFromImages_HIP: " << mh_last_error(session) << std::endl;
    mh_host_free(session, block);
    return xmls;
  }
  for (int i = 0; i < n; ++i) {   // moped.cpp:211-233
    xmls.push_back(shared_ptr<sXML>(new sXML));
    sXML& x = *xmls.back();
    x.name = "Model";
    x["name"] = images[i]->name;
    x.children.resize(1);
    x.children[0].name = "Points";
    const int kept = counts[n + i];
    x.children[0].children.resize(kept);
    for (int k = 0; k < kept; ++k) {
      sXML& point = x.children[0].children[k];
      const float* p = kx + ((size_t)i * capacity + k) * 3;
      const float* d = kd + ((size_t)i * capacity + k) * MH_DESC_DIM;
      point.name = "Point";
      point["p3d"] = toString(p[0]) + " " + toString(p[1]) + " 0";
      point["desc_type"] = descType;
      string& s = point["desc"];
      for (int j = 0; j < MH_DESC_DIM; ++j) s += string(j ? " " : "") + toString(d[j]);
    }
  }
  mh_host_free(session, block);
  return xmls;
}

}  // namespace MopedNS
