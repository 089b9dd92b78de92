// Object::getObjectHull (include/moped.hpp:266-287; moped3d: :402-422) for all objects of a frame in one device call:
// what MopedBench's outputObjectCH (moped3d/libmoped/src/MopedBench.cpp:153-174) asks object after object, and what
// the display steps draw.  The models' points are the ones resident on the device (the rows the MATCH step's Update()
// uploaded: one descriptor type), so the host keeps no copy and projects nothing.
// C++98-clean and free of HIP headers, like the step headers; include it after <moped.hpp> (or moped_types.hpp).
//
//   std::vector<std::list<Pt<2> > > hulls;
//   if (getObjectHulls_HIP(HipSession::get(), models, *frameData.objects, *image, hulls)) ...   // hulls[i]: i-th object
//
// Departures from the CPU function: points behind the camera (z < 0.001) are left out instead of
// entering the chain as (FLT_MAX, FLT_MAX); the hull is over the resident descriptor type's points.
#pragma once
#include <moped_hip.h>

#include <list>
#include <vector>

#include "hip_session.hpp"

namespace MopedNS {

// false: a call failed (HipSession::warn said why) or an object's model is not in `models`; hulls is then empty.
// models: the list the database was uploaded from (index = model index on the device).  behind (optional): per object,
// the model points that lay behind the camera.
inline bool getObjectHulls_HIP(mh_ctx* ctx, const std::vector<SP_Model>& models, const std::list<SP_Object>& objects,
                               const Image& image, std::vector<std::list<Pt<2> > >& hulls,
                               std::vector<int>* behind = 0, int maxVertices = 128) {
  hulls.clear();
  if (behind) behind->clear();
  if (!ctx) return false;
  const size_t n = objects.size();
  if (n == 0) return true;
  std::vector<int32_t> model(n), count(n), nBehind(n);
  std::vector<float> pose(7 * n);
  size_t o = 0;
  for (std::list<SP_Object>::const_iterator it = objects.begin(); it != objects.end(); ++it, ++o) {
    size_t m = 0;
    while (m < models.size() && models[m].get() != (*it)->model.get()) ++m;
    if (m == models.size()) return false;
    model[o] = (int32_t)m;
    for (int i = 0; i < 4; ++i) pose[7 * o + i] = (float)(*it)->pose.rotation[i];
    for (int i = 0; i < 3; ++i) pose[7 * o + 4 + i] = (float)(*it)->pose.translation[i];
  }
  const mh_cam cam = hipCamOf(image);
  std::vector<float> xy;
  for (int round = 0; round < 2; ++round) {   // (a hull with more vertices than maxVertices: once more, with room for the largest)
    xy.assign(2 * n * (size_t)maxVertices, 0.f);
    if (mh_object_hulls(ctx, &model[0], &pose[0], (int)n, &cam, maxVertices, &xy[0], &count[0], &nBehind[0], 0) != MH_OK) {
      HipSession::warn("mh_object_hulls");
      return false;
    }
    int most = 0;
    for (size_t i = 0; i < n; ++i)
      if (count[i] > most) most = count[i];
    if (most <= maxVertices) break;
    maxVertices = most;
  }
  hulls.resize(n);
  for (size_t i = 0; i < n; ++i)
    for (int v = 0; v < count[i] && v < maxVertices; ++v) {
      Pt<2> p;
      p.init(xy[2 * (i * (size_t)maxVertices + v)], xy[2 * (i * (size_t)maxVertices + v) + 1]);
      hulls[i].push_back(p);
    }
  if (behind) behind->assign(nBehind.begin(), nBehind.end());
  return true;
}

}  // namespace MopedNS
