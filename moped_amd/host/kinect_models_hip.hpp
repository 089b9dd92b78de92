// createModelFromKinectViews_HIP -- a 3-D model taught from Kinect views, beside createPlanarModelsFromImages_HIP
// (planar_models_hip.hpp).  The reference has no such call: its models come from an offline reconstruction.  A Kinect
// host has what that reconstruction produces for every keypoint it sees -- the measured 3-D point, in the depth map
// moped3d's node builds (moped3d.cpp:259-276: [h][w][4] floats x, y, z, valid; the depth camera at the origin) -- so a
// view = gray image + depth map + the object's pose in that view (X_cam = R X_model + t, as MOPED reports poses) is
// enough: every keypoint on a measured pixel becomes a model point at inverseTransform(pose, point).
//
//     SP_Model m = createModelFromKinectViews_HIP(HipSession::get(), "mug", images, depthmaps, poses, &index);
//
// The FIRST view becomes a new model at the end of the session's resident store (mh_db_splice_view, MH_DB_INSERT), every
// further view is appended to it (mh_db_append_view) without the keypoints the model holds already: those MATCH accepts
// at mergeRatio whose nearest row is a row of this model within mergeDist of the keypoint's point.  Frames of the
// session see the model from the next enqueue on.  The result holds the rows as the store got them (descriptors as FEAT
// made them, IPs[descType]) and their bounding box; mh_models_add_rows + mh_models_write_xml save it as a .moped.xml.
// All views have one size and their maps the images' size; an optional distance map per view (DEPTHFILL's) with
// spec.max_fill_distance keeps only points near a measurement.  On an error the result is an EMPTY pointer and the
// reason goes to std::clog; views spliced before the error stay in the store.  C++98-clean; the images travel through a
// page-locked block of mh_host_alloc, which the device addresses.
#pragma once
#include "hip_session.hpp"

namespace MopedNS {

inline SP_Model createModelFromKinectViews_HIP(mh_ctx* session, const string& name, vector<SP_Image>& images,
                                               vector<SP_Image>& depthmaps, vector<Pose>& poses, int* modelIndex = 0,
                                               Float mergeRatio = 0.8f, Float mergeDist = 0.002f,
                                               const mh_view_spec* rules = 0, vector<SP_Image>* distancemaps = 0,
                                               int doubleImSize = 1, int capacity = 8192, const string& descType = "SIFT") {
  SP_Model none;
  const size_t n = images.size();
  if (!session || n == 0 || depthmaps.size() != n || poses.size() != n || (distancemaps && distancemaps->size() != n) ||
      capacity <= 0) {
    std::clog << "[moped_hip] createModelFromKinectViews_HIP: no session, no view, or not one depth map and pose per image" << std::endl;
    return none;
  }
  const int w = images[0]->width, h = images[0]->height;
  const size_t px = (size_t)w * h;
  for (size_t i = 0; i < n; ++i)
    if (w <= 0 || h <= 0 || images[i]->width != w || images[i]->height != h || images[i]->data.size() < px ||
        depthmaps[i]->width != w || depthmaps[i]->height != h || depthmaps[i]->data.size() < px * 16 ||
        (distancemaps && ((*distancemaps)[i]->width != w || (*distancemaps)[i]->height != h || (*distancemaps)[i]->data.size() < px * 4))) {
      std::clog << "[moped_hip] createModelFromKinectViews_HIP: the views of one call have one size, the maps the images'" << std::endl;
      return none;
    }
  // one block, reused view after view: depth map | distance map | gray image
  const size_t o_fill = px * 16, o_gray = o_fill + px * 4;
  void* block = 0;
  if (mh_host_alloc(session, o_gray + px, &block) != MH_OK) {
    std::clog << "[moped_hip] createModelFromKinectViews_HIP: " << mh_last_error(session) << std::endl;
    return none;
  }
  unsigned char* b = (unsigned char*)block;
  mh_view_spec spec;
  if (rules) spec = *rules;
  else {
    std::memset(&spec, 0, sizeof spec);   // every keypoint with a measured point, no limit
    spec.max_fill_distance = -1.f;
  }
  spec.merge_ratio = mergeRatio;
  spec.merge_dist = mergeDist;
  int model = 0, rc = mh_db_size(session, 0, &model);   // the new model goes behind the last
  SP_Model out(new Model);
  out->name = name;
  vector<Model::IP>& ips = out->IPs[descType];
  vector<float> desc((size_t)capacity * MH_DESC_DIM), xyz((size_t)capacity * 3);
  float bbox[6] = {0, 0, 0, 0, 0, 0};
  for (size_t i = 0; rc == MH_OK && i < n; ++i) {
    std::memcpy(b, &depthmaps[i]->data[0], px * 16);
    if (distancemaps) std::memcpy(b + o_fill, &(*distancemaps)[i]->data[0], px * 4);
    std::memcpy(b + o_gray, &images[i]->data[0], px);
    mh_view view;
    std::memset(&view, 0, sizeof view);
    view.depth_xyzn_dev = b;
    view.fill_distance_dev = distancemaps ? (const float*)(b + o_fill) : 0;
    for (int j = 0; j < 4; ++j) view.pose[j] = poses[i].rotation[j];
    for (int j = 0; j < 3; ++j) view.pose[4 + j] = poses[i].translation[j];
    for (int j = 0; j < 4; ++j) view.K[j] = images[i]->intrinsicLinearCalibration[j];
    int32_t kept = 0;
    rc = i == 0 ? mh_db_splice_view(session, MH_DB_INSERT, model, b + o_gray, &view, w, h, doubleImSize, capacity, &spec, &kept, bbox,
                                    0, &desc[0], &xyz[0], capacity)
                : mh_db_append_view(session, model, b + o_gray, &view, w, h, doubleImSize, capacity, &spec, &kept, bbox, 0, &desc[0],
                                    &xyz[0], capacity);
    if (rc == MH_ERR_CAPACITY) {   // the edit is made, from the first `capacity` keypoints of the list
      std::clog << "[moped_hip] createModelFromKinectViews_HIP: " << mh_last_error(session) << std::endl;
      rc = MH_OK;
    }
    for (int k = 0; rc == MH_OK && k < kept; ++k) {
      ips.push_back(Model::IP());
      Model::IP& ip = ips.back();
      ip.coord3D.init(xyz[(size_t)k * 3], xyz[(size_t)k * 3 + 1], xyz[(size_t)k * 3 + 2]);
      ip.descriptor.assign(desc.begin() + (size_t)k * MH_DESC_DIM, desc.begin() + (size_t)(k + 1) * MH_DESC_DIM);
    }
  }
  if (rc != MH_OK) std::clog << "[moped_hip] createModelFromKinectViews_HIP: " << mh_last_error(session) << std::endl;
  mh_host_free(session, block);
  if (rc != MH_OK) return none;
  out->boundingBox[0].init(bbox[0], bbox[1], bbox[2]);   // the whole model's, after the last view
  out->boundingBox[1].init(bbox[3], bbox[4], bbox[5]);
  if (modelIndex) *modelIndex = model;
  return out;
}

// createMergedModelFromKinectViews_HIP -- the same teaching, but a keypoint the model holds already is not thrown away: it
// is folded into the row it re-observes (mh_db_merge_view), as MOPED's own model builder gives every model point one
// descriptor from all its observations and counts them (moped-modeling-py MopedModeling.py:863-894, nviews at :915).  The
// first view goes in through mh_db_splice_view, every further one through mh_db_merge_view; then, with minViews > 1, the
// rows fewer than minViews views saw -- sensor noise, background inside the box, a highlight -- are dropped
// (mh_db_keep_rows).  The result holds the mirror rows after patching and pruning: raw descriptors (FEAT's bits, or the
// un-normalised sums of merged rows), so that mh_models_add_rows + mh_models_write_xml save what the store holds.
// *views (optional) gets the view count of every row of the result.  Errors as createModelFromKinectViews_HIP.
inline SP_Model createMergedModelFromKinectViews_HIP(mh_ctx* session, const string& name, vector<SP_Image>& images,
                                                     vector<SP_Image>& depthmaps, vector<Pose>& poses, int minViews,
                                                     int* modelIndex = 0, vector<int>* views = 0, Float mergeRatio = 0.8f,
                                                     Float mergeDist = 0.002f, const mh_view_spec* rules = 0,
                                                     vector<SP_Image>* distancemaps = 0, int doubleImSize = 1,
                                                     int capacity = 8192, const string& descType = "SIFT") {
  SP_Model none;
  const char* who = "[moped_hip] createMergedModelFromKinectViews_HIP: ";
  const size_t n = images.size();
  if (!session || n == 0 || depthmaps.size() != n || poses.size() != n || (distancemaps && distancemaps->size() != n) ||
      capacity <= 0) {
    std::clog << who << "no session, no view, or not one depth map and pose per image" << std::endl;
    return none;
  }
  const int w = images[0]->width, h = images[0]->height;
  const size_t px = (size_t)w * h;
  for (size_t i = 0; i < n; ++i)
    if (w <= 0 || h <= 0 || images[i]->width != w || images[i]->height != h || images[i]->data.size() < px ||
        depthmaps[i]->width != w || depthmaps[i]->height != h || depthmaps[i]->data.size() < px * 16 ||
        (distancemaps && ((*distancemaps)[i]->width != w || (*distancemaps)[i]->height != h || (*distancemaps)[i]->data.size() < px * 4))) {
      std::clog << who << "the views of one call have one size, the maps the images'" << std::endl;
      return none;
    }
  // one block, reused view after view: depth map | distance map | gray image
  const size_t o_fill = px * 16, o_gray = o_fill + px * 4;
  void* block = 0;
  if (mh_host_alloc(session, o_gray + px, &block) != MH_OK) {
    std::clog << who << mh_last_error(session) << std::endl;
    return none;
  }
  unsigned char* b = (unsigned char*)block;
  mh_view_spec spec;
  if (rules) spec = *rules;
  else {
    std::memset(&spec, 0, sizeof spec);   // every keypoint with a measured point, no limit
    spec.max_fill_distance = -1.f;
  }
  spec.merge_ratio = mergeRatio;
  spec.merge_dist = mergeDist;
  int model = 0, rc = mh_db_size(session, 0, &model);   // the new model goes behind the last
  // the mirror of the model's raw rows and their view counts
  vector<float> mdesc, mxyz;
  vector<int32_t> count;
  vector<float> desc((size_t)capacity * MH_DESC_DIM), xyz((size_t)capacity * 3);
  vector<float> gdesc, gxyz;   // the merged rows of one view
  vector<int32_t> gidx, vout;
  float bbox[6] = {0, 0, 0, 0, 0, 0};
  for (size_t i = 0; rc == MH_OK && i < n; ++i) {
    std::memcpy(b, &depthmaps[i]->data[0], px * 16);
    if (distancemaps) std::memcpy(b + o_fill, &(*distancemaps)[i]->data[0], px * 4);
    std::memcpy(b + o_gray, &images[i]->data[0], px);
    mh_view view;
    std::memset(&view, 0, sizeof view);
    view.depth_xyzn_dev = b;
    view.fill_distance_dev = distancemaps ? (const float*)(b + o_fill) : 0;
    for (int j = 0; j < 4; ++j) view.pose[j] = poses[i].rotation[j];
    for (int j = 0; j < 3; ++j) view.pose[4 + j] = poses[i].translation[j];
    for (int j = 0; j < 4; ++j) view.K[j] = images[i]->intrinsicLinearCalibration[j];
    int32_t kept = 0, merged = 0;
    const size_t rows = count.size();
    if (i == 0) {
      rc = mh_db_splice_view(session, MH_DB_INSERT, model, b + o_gray, &view, w, h, doubleImSize, capacity, &spec, &kept, bbox, 0,
                             &desc[0], &xyz[0], capacity);
    } else {
      const size_t gcap = rows < (size_t)capacity ? rows : (size_t)capacity;
      gidx.resize(gcap + 1);
      gdesc.resize((gcap + 1) * MH_DESC_DIM);
      gxyz.resize((gcap + 1) * 3);
      vout.resize(rows + (size_t)capacity);
      rc = mh_db_merge_view(session, model, b + o_gray, &view, w, h, doubleImSize, capacity, &spec, rows ? &count[0] : 0, (int)rows,
                            &kept, &merged, bbox, 0, &desc[0], &xyz[0], capacity, &gidx[0], &gdesc[0], &gxyz[0], (int)gcap,
                            &vout[0], (int)vout.size());
    }
    if (rc == MH_ERR_CAPACITY) {   // the edit is made, from the first `capacity` keypoints of the list
      std::clog << who << mh_last_error(session) << std::endl;
      rc = MH_OK;
    }
    if (rc != MH_OK) break;
    for (int k = 0; k < merged; ++k) {   // the rows the view re-observed
      const size_t r = (size_t)gidx[k];
      std::memcpy(&mdesc[r * MH_DESC_DIM], &gdesc[(size_t)k * MH_DESC_DIM], MH_DESC_DIM * sizeof(float));
      std::memcpy(&mxyz[r * 3], &gxyz[(size_t)k * 3], 3 * sizeof(float));
    }
    if (i > 0) count.assign(vout.begin(), vout.begin() + rows);
    mdesc.insert(mdesc.end(), desc.begin(), desc.begin() + (size_t)kept * MH_DESC_DIM);
    mxyz.insert(mxyz.end(), xyz.begin(), xyz.begin() + (size_t)kept * 3);
    count.insert(count.end(), (size_t)kept, 1);
  }
  if (rc == MH_OK && minViews > 1) {
    vector<uint8_t> keep(count.size() + 1);
    size_t at = 0;
    for (size_t r = 0; r < count.size(); ++r) {
      keep[r] = count[r] >= minViews ? 1 : 0;
      if (!keep[r]) continue;
      if (at != r) {
        std::memmove(&mdesc[at * MH_DESC_DIM], &mdesc[r * MH_DESC_DIM], MH_DESC_DIM * sizeof(float));
        std::memmove(&mxyz[at * 3], &mxyz[r * 3], 3 * sizeof(float));
        count[at] = count[r];
      }
      ++at;
    }
    int32_t left = 0;
    rc = mh_db_keep_rows(session, model, &keep[0], (int)count.size(), &left, bbox);
    if (rc == MH_OK && (size_t)left != at) {
      std::clog << who << "mh_db_keep_rows kept " << left << " rows, the mirror " << at << std::endl;
      rc = MH_ERR_ARG;
    }
    count.resize(at);
    mdesc.resize(at * MH_DESC_DIM);
    mxyz.resize(at * 3);
  } else if (rc != MH_OK) {
    std::clog << who << mh_last_error(session) << std::endl;
  }
  mh_host_free(session, block);
  if (rc != MH_OK) return none;
  SP_Model out(new Model);
  out->name = name;
  vector<Model::IP>& ips = out->IPs[descType];
  ips.resize(count.size());
  for (size_t k = 0; k < count.size(); ++k) {
    ips[k].coord3D.init(mxyz[k * 3], mxyz[k * 3 + 1], mxyz[k * 3 + 2]);
    ips[k].descriptor.assign(mdesc.begin() + k * MH_DESC_DIM, mdesc.begin() + (k + 1) * MH_DESC_DIM);
  }
  out->boundingBox[0].init(bbox[0], bbox[1], bbox[2]);   // the whole model's, after the last edit
  out->boundingBox[1].init(bbox[3], bbox[4], bbox[5]);
  if (modelIndex) *modelIndex = model;
  if (views) views->assign(count.begin(), count.end());
  return out;
}

}  // namespace MopedNS
