// One mh_ctx shared by the HIP steps of a pipeline (the steps run strictly one
// after another on the caller's thread, src/moped.cpp:184-191).  C++98-clean and
// free of HIP headers so it compiles inside libmoped with its own flags
// (-std=gnu++98, libmoped/Makefile:44-47); the GPU lives behind the C ABI.
// Beside the session, the glue between FrameData and the C ABI that more than one step needs lives here, once:
//   HipHandover, HipDepthMaps   what consecutive steps of a frame leave on the device for each other
//   HipResidentModels           edits of the resident database (IncrementalModels)
//   HipModelTable               Update() of every MATCH-like step: pack, normalise, write back, upload
//   hipCamOf, HipCameraTable    an Image as mh_cam; the cameras a frame's matches or features refer to
//   hipAppendObject             a result record as an Object of the frame
//   HipPinnedBlock              the page-locked block a step packs a frame's features into
//   hipStageParams              one POSE + FILTER stage of mh_frame_params
//   hipGetConfig, hipSetConfig  the reference's config keys
// (moped3d's depth-map lookup needs Image::imageType and is in hip_frame3d.hpp.)
#pragma once
#include <moped_hip.h>

#include <cstdlib>
#include <iostream>
#include <list>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace MopedNS {

class HipSession {
 public:
  // NULL when no gfx950 device / library problem: the step then sets capable=false
  // and MopedStep::getAlg() falls through to the next algorithm of the same step
  // (src/util.hpp:151-159).
  static mh_ctx* get(int device = 0) {
    static HipSession s(device);
    return s.ctx_;
  }
  static void warn(const char* where) {
    mh_ctx* c = get();
    std::clog << "[moped_hip] " << where << ": " << (c ? mh_last_error(c) : "no context") << std::endl;
  }

 private:
  explicit HipSession(int device) : ctx_(0) {
    if (mh_create(device, &ctx_) != MH_OK) ctx_ = 0;
  }
  ~HipSession() {
    if (ctx_) mh_destroy(ctx_);
  }
  mh_ctx* ctx_;
};

// The hand-over between consecutive HIP steps of one frame (mh_step_*, include/moped_hip.h): a HIP step that finds
// FrameData as the HIP step before it left it -- same frame object, and the lists it is about to read hash to what that
// step wrote -- runs on the device-resident copy instead of uploading them again.  Anything else (a CPU step in between
// that touched the lists, a frame with several cameras, lists that were not empty before MATCH, MH_STEP_HANDOVER=0)
// takes the upload path of the slot, which is always valid; so does a refusal by the library (the context's frame
// arrays were used by another call).  One instance per process, like the context.
struct HipHandover {
  int stage;                 // -1: nothing resident; 0 MATCH .. 5 FILTER2 = the last slot that ran on the resident frame
  const void* frame;         // the FrameData it belongs to
  unsigned long long matchesTag, clustersTag, objectsTag;
  unsigned long taken;       // steps that ran on the resident frame so far (tests, moped_hip_test)

  static HipHandover& get() {
    static HipHandover h;
    return h;
  }
  static bool enabled() {
    static const int on = (std::getenv("MH_STEP_HANDOVER") && std::getenv("MH_STEP_HANDOVER")[0] == '0') ? 0 : 1;
    return on != 0;
  }
  void drop() { stage = -1; frame = 0; }

  // FNV-1a over the bytes a step reads
  static unsigned long long mix(unsigned long long h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
  }
  static unsigned long long tagMatches(const FrameData& fd) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t m = 0; m < fd.matches.size(); ++m) {
      const size_t n = fd.matches[m].size();
      h = mix(h, &n, sizeof n);
      for (size_t k = 0; k < n; ++k) {
        const FrameData::Match& x = fd.matches[m][k];
        const float v[5] = {(float)x.coord2D[0], (float)x.coord2D[1], (float)x.coord3D[0], (float)x.coord3D[1], (float)x.coord3D[2]};
        h = mix(h, &x.imageIdx, sizeof x.imageIdx);
        h = mix(h, v, sizeof v);
      }
    }
    return h;
  }
  static unsigned long long tagClusters(const FrameData& fd) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t m = 0; m < fd.clusters.size(); ++m) {
      const size_t n = fd.clusters[m].size();
      h = mix(h, &n, sizeof n);
      for (size_t c = 0; c < n; ++c) {
        const size_t sz = fd.clusters[m][c].size();
        h = mix(h, &sz, sizeof sz);
        for (FrameData::Cluster::const_iterator it = fd.clusters[m][c].begin(); it != fd.clusters[m][c].end(); ++it) h = mix(h, &*it, sizeof(int));
      }
    }
    return h;
  }
  static unsigned long long tagObjects(const FrameData& fd) {
    unsigned long long h = 1469598103934665603ull;
    for (list<SP_Object>::const_iterator it = fd.objects->begin(); it != fd.objects->end(); ++it) {
      const void* model = (*it)->model.get();
      float v[7];
      for (int i = 0; i < 4; ++i) v[i] = (float)(*it)->pose.rotation[i];
      for (int i = 0; i < 3; ++i) v[4 + i] = (float)(*it)->pose.translation[i];
      h = mix(h, &model, sizeof model);
      h = mix(h, v, sizeof v);
    }
    return h;
  }
  bool at(int wanted, const FrameData& fd) const { return enabled() && stage == wanted && frame == (const void*)&fd; }

 private:
  HipHandover() : stage(-1), frame(0), matchesTag(0), clustersTag(0), objectsTag(0), taken(0) {}
};

// Opt-in (config key IncrementalModels = 1 of MATCH_BRUTE_HIP, MATCH_ADAPTIVE_BRUTE_HIP, FRAME_RESIDENT_HIP): Update()
// compares `models` with what is resident on the device -- SP_Model pointer and descriptor count per index -- and, if the
// difference is a run of appends, one removal, or replaces, edits the resident database (mh_db_splice) instead of
// packing, normalising and uploading every model again.  Only the changed models' descriptors are normalised and
// written back (the reference normalises every model on every Update, MATCH_ANN_CPU.hpp:94).  One instance per process,
// like the context whose store it describes.
struct HipResidentModels {
  std::vector<const void*> ptr;   // the SP_Model each resident model came from
  std::vector<size_t> count;      // ... and its descriptor count
  std::string type;               // DescriptorType the rows were taken from
  bool valid;                     // the store holds exactly these models, normalised
  unsigned long fullUploads, splices;   // (tests, db_edit_step_test)

  static HipResidentModels& get() {
    static HipResidentModels r;
    return r;
  }
  static bool same(const SP_Model& m, const std::string& type, const void* p, size_t n) {
    std::map<std::string, std::vector<Model::IP> >::const_iterator it = m->IPs.find(type);
    return m.get() == p && (it == m->IPs.end() ? 0 : it->second.size()) == n;
  }
  // what the full path leaves resident
  void record(const std::vector<SP_Model>& models, const std::string& t) {
    ptr.resize(models.size());
    count.resize(models.size());
    for (size_t m = 0; m < models.size(); ++m) {
      ptr[m] = models[m].get();
      count[m] = models[m]->IPs[t].size();
    }
    type = t;
    valid = true;
    ++fullUploads;
  }
  // one model's rows: normalised on the device, written back, spliced in
  bool splice(mh_ctx* ctx, int op, int index, Model* model, const std::string& t) {
    if (op == MH_DB_REMOVE) return mh_db_splice(ctx, op, index, 0, 0, 0, 0, 0) == MH_OK;
    std::vector<Model::IP>& ips = model->IPs[t];
    const size_t n = ips.size();
    std::vector<float> desc(n * MH_DESC_DIM + 1), xyz(n * 3 + 1);
    for (size_t f = 0; f < n; ++f) {
      for (int i = 0; i < MH_DESC_DIM; ++i) desc[f * MH_DESC_DIM + i] = ips[f].descriptor[i];
      for (int i = 0; i < 3; ++i) xyz[f * 3 + i] = ips[f].coord3D[i];
    }
    if (n > 0 && mh_normalize(ctx, &desc[0], (int)n) != MH_OK) return false;
    for (size_t f = 0; f < n; ++f)
      for (int i = 0; i < MH_DESC_DIM; ++i) ips[f].descriptor[i] = desc[f * MH_DESC_DIM + i];
    return mh_db_splice(ctx, op, index, &desc[0], &xyz[0], (int)n, 0, 0) == MH_OK;
  }
  // true: the store now holds `models` (nothing to do counts); false: not a difference this serves, or a call failed --
  // the caller takes the full path, which is always valid
  bool update(mh_ctx* ctx, std::vector<SP_Model>& models, const std::string& t) {
    if (!valid || t != type) return false;
    const size_t had = ptr.size(), now = models.size();
    valid = false;   // until every edit below has succeeded
    if (now + 1 == had) {   // one removal
      size_t k = 0;
      while (k < now && same(models[k], t, ptr[k], count[k])) ++k;
      for (size_t i = k; i < now; ++i)
        if (!same(models[i], t, ptr[i + 1], count[i + 1])) return false;
      if (!splice(ctx, MH_DB_REMOVE, (int)k, 0, t)) return false;
      ptr.erase(ptr.begin() + k);
      count.erase(count.begin() + k);
      ++splices;
    } else if (now >= had) {   // replaces, or a run of appends behind unchanged models
      if (now > had)
        for (size_t i = 0; i < had; ++i)
          if (!same(models[i], t, ptr[i], count[i])) return false;
      for (size_t i = 0; i < now; ++i) {
        if (i < had && same(models[i], t, ptr[i], count[i])) continue;
        if (!splice(ctx, i < had ? MH_DB_REPLACE : MH_DB_INSERT, (int)i, models[i].get(), t)) return false;
        if (i < had) {
          ptr[i] = models[i].get();
          count[i] = models[i]->IPs[t].size();
        } else {
          ptr.push_back(models[i].get());
          count.push_back(models[i]->IPs[t].size());
        }
        ++splices;
      }
    } else {
      return false;
    }
    valid = true;
    return true;
  }

 private:
  HipResidentModels() : valid(false), fullUploads(0), splices(0) {}
};

// What Update() of a MATCH step leaves behind (MATCH_ANN_CPU.hpp:72-109), for MATCH_BRUTE_HIP, FRAME_RESIDENT_HIP and
// moped3d's HipAdaptiveModels alike: every model's descriptors normalised IN PLACE (:94) and resident on the device --
// uploaded, or edited when IncrementalModels is set and the difference is one HipResidentModels serves -- and the
// row -> model / row -> model point tables of the upload path.
struct HipModelTable {
  bool skipCalculation;   // true: one row or none (the reference's rule, :102), or the last update() failed
  std::vector<int> correspModel;
  std::vector<Pt<3>*> correspFeat;

  HipModelTable() : skipCalculation(true) {}

  // false: a call failed and was reported; skipCalculation stays true, the caller leaves configUpdated set and the next
  // frame tries again
  bool update(mh_ctx* ctx, std::vector<SP_Model>& models, const std::string& DescriptorType, int IncrementalModels) {
    skipCalculation = true;
    size_t n = 0;
    for (size_t m = 0; m < models.size(); ++m) n += models[m]->IPs[DescriptorType].size();
    correspModel.resize(n);
    correspFeat.resize(n);
    size_t x = 0;
    for (size_t m = 0; m < models.size(); ++m) {
      std::vector<Model::IP>& ips = models[m]->IPs[DescriptorType];
      for (size_t f = 0; f < ips.size(); ++f, ++x) {
        correspModel[x] = (int)m;
        correspFeat[x] = &ips[f].coord3D;
      }
    }
    if (IncrementalModels && HipResidentModels::get().update(ctx, models, DescriptorType)) {
      skipCalculation = n <= 1;
      return true;
    }
    if (n <= 1) return true;
    std::vector<float> desc(n * MH_DESC_DIM), xyz(n * 3);
    std::vector<int32_t> owner(n);
    x = 0;
    for (size_t m = 0; m < models.size(); ++m) {
      std::vector<Model::IP>& ips = models[m]->IPs[DescriptorType];
      for (size_t f = 0; f < ips.size(); ++f, ++x) {
        owner[x] = (int32_t)m;
        for (int i = 0; i < MH_DESC_DIM; ++i) desc[x * MH_DESC_DIM + i] = ips[f].descriptor[i];
        for (int i = 0; i < 3; ++i) xyz[x * 3 + i] = ips[f].coord3D[i];
      }
    }
    // normalised on the device (bit-identical to norm(), :54-57) and written back, as Update() does to the models (:94)
    if (mh_normalize(ctx, &desc[0], (int)n) != MH_OK) { HipSession::warn("mh_normalize"); return false; }
    x = 0;
    for (size_t m = 0; m < models.size(); ++m) {
      std::vector<Model::IP>& ips = models[m]->IPs[DescriptorType];
      for (size_t f = 0; f < ips.size(); ++f, ++x)
        for (int i = 0; i < MH_DESC_DIM; ++i) ips[f].descriptor[i] = desc[x * MH_DESC_DIM + i];
    }
    if (mh_db_upload(ctx, &desc[0], &owner[0], &xyz[0], (int)n, (int)models.size(), 0) != MH_OK) {
      HipSession::warn("mh_db_upload");
      return false;
    }
    skipCalculation = false;
    if (IncrementalModels) HipResidentModels::get().record(models, DescriptorType);
    return true;
  }
};

// An Image's camera as the C ABI takes it
inline mh_cam hipCamOf(const Image& im) {
  mh_cam c;
  for (int j = 0; j < 4; ++j) c.K[j] = im.intrinsicLinearCalibration[j];
  for (int j = 0; j < 4; ++j) c.cam[j] = im.cameraPose.rotation[j];
  for (int j = 0; j < 3; ++j) c.cam[4 + j] = im.cameraPose.translation[j];
  return c;
}

// The cameras of a frame for the *_images entry points.  The reference projects every match through
// *frameData.images[match.imageIdx] whatever else the image list holds (FILTER_PROJECTION_CPU.hpp:100-104,
// POSE_RANSAC_LM_DIFF_REPROJECTION_CPU.hpp:228-237) -- a moped3d frame carries its depth and distance maps as
// further Images that no match points to -- so the table holds the images the matches REFER to, renumbered in
// image order (which keeps CLUSTER's and FILTER's per-image ordering), and `local` maps imageIdx to that number.
struct HipCameraTable {
  std::vector<mh_cam> cams;
  std::vector<int> local;  // imageIdx -> index into cams, -1 = nothing refers to it
  bool ok;                 // false: cams is empty (an imageIdx outside FrameData::images) or longer than MH_MAX_IMAGES

  // from the frame's matches; says itself why a step is skipped
  explicit HipCameraTable(const FrameData& frameData) : local(frameData.images.size(), -1), ok(true) {
    for (size_t m = 0; m < frameData.matches.size(); ++m) mark(frameData.matches[m]);
    finish(frameData);
    if (!ok)
      std::clog << "[moped_hip] frame refers to an image outside FrameData::images or to more than " << MH_MAX_IMAGES
                << " images: step skipped" << std::endl;
  }
  // from any list whose elements have .imageIdx (FRAME_RESIDENT_HIP: the features); silent, the step words its own message
  template <typename List>
  HipCameraTable(const FrameData& frameData, const List& refs) : local(frameData.images.size(), -1), ok(true) {
    mark(refs);
    finish(frameData);
  }

 private:
  template <typename List>
  void mark(const List& refs) {
    for (size_t k = 0; k < refs.size() && ok; ++k) {
      const int i = refs[k].imageIdx;
      if (i < 0 || i >= (int)local.size()) ok = false;
      else local[i] = 0;
    }
  }
  void finish(const FrameData& frameData) {
    for (size_t i = 0; i < local.size() && ok; ++i) {
      if (local[i] < 0) continue;
      local[i] = (int)cams.size();
      cams.push_back(hipCamOf(*frameData.images[i]));
    }
    if ((int)cams.size() > MH_MAX_IMAGES) ok = false;
  }
};

// One result record {model, pose (qx, qy, qz, qw, tx, ty, tz), score} as an Object at the end of *frameData.objects
inline void hipAppendObject(FrameData& frameData, const SP_Model& model, const float pose[7], Float score) {
  SP_Object obj(new Object);
  frameData.objects->push_back(obj);
  obj->pose.rotation.init(pose[0], pose[1], pose[2], pose[3]);
  obj->pose.translation.init(pose[4], pose[5], pose[6]);
  obj->model = model;
  obj->score = score;
}

// The page-locked block (mh_host_alloc) a step packs a frame's descriptors / keypoints / image indices into, grown when a
// frame needs more.  Freed with the context it came from: the session's, which outlives every step (a step's constructor
// is what first calls HipSession::get()).
class HipPinnedBlock {
 public:
  HipPinnedBlock() : ctx_(0), block_(0), bytes_(0) {}
  ~HipPinnedBlock() {
    if (block_) mh_host_free(ctx_, block_);
  }
  // false: no block (the allocation failed); else data() holds at least `need` bytes
  bool ensure(mh_ctx* ctx, size_t need) {
    if (need <= bytes_) return true;
    if (block_) mh_host_free(ctx_, block_);
    block_ = 0;
    bytes_ = 0;
    const size_t want = need + need / 4;
    if (mh_host_alloc(ctx, want, &block_) != MH_OK) { block_ = 0; return false; }
    ctx_ = ctx;
    bytes_ = want;
    return true;
  }
  void* data() const { return block_; }
  size_t bytes() const { return bytes_; }

 private:
  HipPinnedBlock(const HipPinnedBlock&);
  HipPinnedBlock& operator=(const HipPinnedBlock&);
  mh_ctx* ctx_;
  void* block_;
  size_t bytes_;
};

// POSE + FILTER (stage 1) or POSE2 + FILTER2 (stage 2) of a frame, from the reference constructors' arguments
inline void hipStageParams(mh_frame_params& prm, int stage, int NHypotheses, int MaxObjectsPerCluster, int NPtsAlign,
                           int MinNPtsObject, Float ErrorThreshold, int MinPoints, Float FeatureDistance, Float MinScore) {
  mh_pose_params& pose = stage == 1 ? prm.pose1 : prm.pose2;
  pose.n_hypotheses = NHypotheses;
  pose.max_objects_per_cluster = MaxObjectsPerCluster;
  pose.n_pts_align = NPtsAlign;
  pose.min_n_pts_object = MinNPtsObject;
  pose.error_threshold = (float)ErrorThreshold;
  (stage == 1 ? prm.f1_min_points : prm.f2_min_points) = MinPoints;
  (stage == 1 ? prm.f1_feature_distance : prm.f2_feature_distance) = (float)FeatureDistance;
  (stage == 1 ? prm.f1_min_score : prm.f2_min_score) = (float)MinScore;
}

// The frame's depth map on the device, shared by moped3d's steps of one frame (DEPTHFILTER_HIP, DEPTHFILTER2,
// DEPTHMAP_PROP_HIP, CLUSTER_LINKAGE_HIP): the first of them that finds another map than the context holds uploads it
// (mh_frame_set_depth_image_host: 4.9 MB + 1.2 MB for 640x480), the others pass NULL and read that copy -- the map
// crosses PCIe once per frame instead of once per step.  "The same map" = the same Image objects with the same buffers,
// sizes and a sample of 4096 words of each (a sensor's next frame differs in nearly every pixel; a step that rewrites
// the map in place -- DEPTH_FILL_EXACT_HIP -- or hands the context another one calls drop()).  One instance per process.
struct HipDepthMaps {
  unsigned long long tag;
  bool valid;
  unsigned long uploads;   // (tests, moped3d_hip_test)

  static HipDepthMaps& get() {
    static HipDepthMaps d;
    return d;
  }
  void drop() { valid = false; }
  static unsigned long long sample(unsigned long long h, const Image* im) {
    const void* p = im;
    const unsigned char* data = im->data.empty() ? 0 : &im->data[0];
    const size_t words = im->data.size() / 4, step = words / 4096 + 1;
    h = HipHandover::mix(h, &p, sizeof p);
    h = HipHandover::mix(h, &data, sizeof data);
    h = HipHandover::mix(h, &im->width, sizeof im->width);
    h = HipHandover::mix(h, &im->height, sizeof im->height);
    h = HipHandover::mix(h, &words, sizeof words);
    for (size_t i = 0; i < words; i += step) h = HipHandover::mix(h, data + 4 * i, 4);
    return h;
  }
  // true: the context holds depthmap (and distanceMap, or none) as its frame map
  bool ensure(mh_ctx* ctx, const Image* depthmap, const Image* distanceMap) {
    const size_t px = (size_t)(depthmap->width > 0 ? depthmap->width : 0) * (size_t)(depthmap->height > 0 ? depthmap->height : 0);
    if (px == 0 || depthmap->data.size() < px * 4 * sizeof(float)) return false;
    if (distanceMap && distanceMap->data.size() < px * sizeof(float)) distanceMap = 0;
    unsigned long long t = sample(1469598103934665603ull, depthmap);
    if (distanceMap) t = sample(t, distanceMap);
    if (valid && t == tag) return true;
    valid = false;
    if (mh_frame_set_depth_image_host(ctx, (const float*)&depthmap->data[0], distanceMap ? (const float*)&distanceMap->data[0] : 0,
                                      depthmap->width, depthmap->height, MH_DEPTH_BACKPROJECTION, 0.5f, 0.1f) != MH_OK)
      return false;
    tag = t;
    valid = true;
    ++uploads;
    return true;
  }

 private:
  HipDepthMaps() : tag(0), valid(false), uploads(0) {}
};

// Same key layout as GET_CONFIG: "<STEP>:<algIdx>:<HeaderBasename>/<var>" (src/util.hpp:62)
template <typename T>
inline void hipGetConfig(std::map<std::string, std::string>& config, const std::string& step, int alg,
                         const char* header, const char* var, const T& value) {
  config[step + ":" + toString(alg) + ":" + header + "/" + var] = toString(value);
}

// The counterpart for setConfig: takes `value` from the key hipGetConfig writes; true if it was there and parsed.
// (The reference's SET_CONFIG builds its key with another substring length than GET_CONFIG, src/util.hpp:62-63, so a
// value set through Moped::setConfig never reaches a CPU step -- SURVEY F5; the HIP steps honour the key they publish.)
template <typename T>
inline bool hipSetConfig(std::map<std::string, std::string>& config, const std::string& step, int alg, const char* header,
                         const char* var, T& value) {
  std::map<std::string, std::string>::iterator it = config.find(step + ":" + toString(alg) + ":" + header + "/" + var);
  if (it == config.end() || it->second.empty()) return false;
  std::istringstream in(it->second);
  T v;
  if (!(in >> v)) return false;
  value = v;
  return true;
}

}  // namespace MopedNS
