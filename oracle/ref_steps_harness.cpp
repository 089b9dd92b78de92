// oracle/ref_steps_harness.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// C-ABI wrapper over four of the reference's STEP classes, each driven through its own
// process():
//
//   -DREF_STEPS_MOPED2   (oracle/_ref/libmoped_ref_steps2.so)
//       moped2/libmoped/src/cluster/CLUSTER_MEAN_SHIFT_CPU.hpp
//       moped2/libmoped/src/filter/FILTER_PROJECTION_CPU.hpp
//   -DREF_STEPS_MOPED3D  (oracle/_ref/libmoped_ref_steps3d.so)
//       moped3d/libmoped/src/depthfilter/DEPTHFILTER_CPU.hpp
//       moped3d/libmoped/src/depthprop/DEPTHMAP_PROP_CPU.hpp
//       moped3d/libmoped/src/cluster/CLUSTER_MEAN_SHIFT_CPU.hpp   (2-D and use3D)
//
// The step headers include nothing but <math.h>; what they need beside the tree's
// include/moped.hpp is src/util.hpp, and THAT file is what pulls OpenCV in.  This file defines
// its own minimal stand-ins for the names util.hpp would provide -- only the members the four
// classes touch -- and then includes the reference's headers where they lie (build_ref.sh
// passes the -I paths).  Nothing of the reference is copied here; the two trees define the
// same names in MopedNS, hence two translation units and two libraries.
//
// Not buildable this way: CLUSTER_LINKAGE_CPU and DEPTH_FILL_EXACT_CPU (IplImage),
// MATCH_ADAPTIVE_FLANN_CPU (cv::flann).
//
// Build flags as for libmoped_ref.so (see build_ref.sh): -O2, no fast-math, -std=gnu++98,
// -fno-delete-null-pointer-checks (project() tests the address of a reference), -fopenmp.

#if !defined(REF_STEPS_MOPED2) && !defined(REF_STEPS_MOPED3D)
#error "define REF_STEPS_MOPED2 or REF_STEPS_MOPED3D"
#endif

#include <moped.hpp>

#include <cstdio>
#include <cstring>
#include <list>
#include <map>
#include <string>
#include <vector>

// ---- stand-ins for util.hpp ------------------------------------------------------------------

// the classes' configuration plumbing: not exercised, the constructors take the values
#define GET_CONFIG(varName) ((void)0)
#define SET_CONFIG(varName) ((void)0)

// foreach(i, c): the body runs once per element of c with `i` a reference to it.  Four nested
// for statements so that `continue` goes on with the next element and `break` leaves the whole
// construct: the innermost runs the body once and marks the element finished in its increment,
// which a `break` skips; the one around it turns an unfinished element into "stop".
#define RS_LOOP_BODY(i, itname, c)                                                                        \
  for (int i##_state = 0; i##_state < 2; i##_state = (i##_state == 0 ? (i##_stop = 1, 2) : 2))            \
    for (__typeof__(*(c).begin())& i = *itname; i##_state == 0; i##_state = 1)

#define foreach(i, c)                                                                                     \
  for (int i##_stop = 0; !i##_stop; i##_stop = 1)                                                         \
    for (__typeof__((c).begin()) i##_pos = (c).begin(); !i##_stop && i##_pos != (c).end(); ++i##_pos)     \
      RS_LOOP_BODY(i, i##_pos, c)

// eforeach(i, it, c): the same with the iterator `it` visible in the body.  A body that assigns
// `it` (it = c.erase(it)) continues at the new `it`; otherwise `it` advances by one.
#define eforeach(i, it, c)                                                                                \
  for (int i##_stop = 0; !i##_stop; i##_stop = 1)                                                         \
    for (__typeof__((c).begin()) it = (c).begin(), i##_was = it; !i##_stop && it != (c).end();            \
         (it == i##_was ? (void)++it : (void)0), i##_was = it)                                            \
      RS_LOOP_BODY(i, it, c)

namespace MopedNS {

struct depthInformation {
  bool depthValid;
  Pt<3> coord3D;
  Float depth;
  Float fillDistance;
};

struct FrameData {
  struct DetectedFeature {
    int imageIdx;
    Pt<2> coord2D;
    vector<float> descriptor;
  };
  struct Match {
    int imageIdx;
    Pt<2> coord2D;
    Pt<3> coord3D;
    depthInformation depthData;
  };
  typedef list<int> Cluster;

  vector<SP_Image> images;
  map<string, vector<DetectedFeature> > detectedFeatures;
  vector<vector<Match> > matches;
  vector<vector<Cluster> > clusters;
  vector<vector<Cluster> > oldClusters;
  list<SP_Object>* objects;
};

class MopedAlg {
 public:
  vector<SP_Model>* models;
  bool configUpdated;
  string _stepName;

  MopedAlg() : models(NULL), configUpdated(true) {}
  virtual ~MopedAlg() {}
  virtual void modelsUpdated(vector<SP_Model>& _models) {
    models = &_models;
    configUpdated = true;
  }
  virtual void process(FrameData& frameData) = 0;
};

}  // namespace MopedNS

// ---- the reference's classes, where they lie ---------------------------------------------------
#ifdef REF_STEPS_MOPED2
#include <cluster/CLUSTER_MEAN_SHIFT_CPU.hpp>
#include <filter/FILTER_PROJECTION_CPU.hpp>
#else
#include <cluster/CLUSTER_MEAN_SHIFT_CPU.hpp>
#include <depthfilter/DEPTHFILTER_CPU.hpp>
#include <depthprop/DEPTHMAP_PROP_CPU.hpp>
#endif

using namespace MopedNS;

namespace {

void make_models(std::vector<SP_Model>& models, int n) {
  for (int m = 0; m < n; m++) {
    SP_Model mod(new Model);
    char nm[32];
    snprintf(nm, sizeof nm, "model%06d", m);
    mod->name = nm;
    models.push_back(mod);
  }
}

const float K_NONE[4] = {1.f, 1.f, 0.f, 0.f};
const float CAM_NONE[7] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};

SP_Image make_camera(int w, int h, const float K[4], const float cam[7]) {
  SP_Image img(new Image);
  img->name = "gray";
  img->width = w;
  img->height = h;
  img->intrinsicLinearCalibration.init(K[0], K[1], K[2], K[3]);
  img->intrinsicNonlinearCalibration.init(0.f, 0.f, 0.f, 0.f);
  img->cameraPose.rotation.init(cam[0], cam[1], cam[2], cam[3]);
  img->cameraPose.translation.init(cam[4], cam[5], cam[6]);
  img->TM.init(img->cameraPose);  // as MopedPimpl::processImages does before the steps run
  return img;
}

#ifdef REF_STEPS_MOPED3D
SP_Image make_float_image(Image_Type type, const char* name, const float* px, int w, int h, int floats_per_px,
                          const float K[4]) {
  SP_Image img = make_camera(w, h, K, CAM_NONE);
  img->imageType = type;
  img->name = name;
  img->data.resize((size_t)w * h * floats_per_px * sizeof(float));
  memcpy(&img->data[0], px, img->data.size());
  return img;
}
#endif

}  // namespace

extern "C" {

// 2: built from moped2's tree, 3: from moped3d's
int ref_steps_tree(void) {
#ifdef REF_STEPS_MOPED2
  return 2;
#else
  return 3;
#endif
}

// CLUSTER_MEAN_SHIFT_CPU::process.  pts: n x dim (dim 2: Match::coord2D; dim 3, moped3d only: use3D over
// depthData.coord3D).  Matches of model m are the rows [model_off[m], model_off[m+1]), image_of names each row's
// image.  Out: the clusters in the order process() leaves them -- model after model, inside a model frameData.clusters[model]
// -- as member lists (indices into the MODEL's matches, list order): cluster c = members[cl_off[c] .. cl_off[c+1]),
// cl_model[c] its model.  Returns the number of clusters, -1 for a dim this build does not have.
int ref_meanshift_step(const float* pts, int dim, const int* image_of, const int* model_off, int n_models, int n_images,
                       float radius, float merge, int min_pts, int max_iter, int* members, int* cl_off, int* cl_model) {
#ifdef REF_STEPS_MOPED2
  if (dim != 2) return -1;
  CLUSTER_MEAN_SHIFT_CPU alg(radius, merge, (unsigned)min_pts, (unsigned)max_iter);
#else
  if (dim != 2 && dim != 3) return -1;
  CLUSTER_MEAN_SHIFT_CPU alg(radius, merge, (unsigned)min_pts, (unsigned)max_iter, dim == 3);
#endif
  std::vector<SP_Model> models;
  make_models(models, n_models);
  alg.modelsUpdated(models);
  alg._stepName = "CLUSTER";
  FrameData fd;
  fd.objects = NULL;
  for (int i = 0; i < n_images; i++) fd.images.push_back(make_camera(640, 480, K_NONE, CAM_NONE));
  fd.matches.resize(n_models);
  for (int m = 0; m < n_models; m++)
    for (int i = model_off[m]; i < model_off[m + 1]; i++) {
      FrameData::Match mt;
      mt.imageIdx = image_of[i];
      mt.coord2D.init(pts[(size_t)dim * i], pts[(size_t)dim * i + 1]);
      mt.coord3D.init(0.f, 0.f, 0.f);
      mt.depthData.depthValid = true;
      mt.depthData.depth = 0.f;
      mt.depthData.fillDistance = -1.f;
      if (dim == 3)
        mt.depthData.coord3D.init(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
      else
        mt.depthData.coord3D.init(0.f, 0.f, 0.f);
      fd.matches[m].push_back(mt);
    }
  alg.process(fd);
  int nc = 0, pos = 0;
  cl_off[0] = 0;
  for (int m = 0; m < (int)fd.clusters.size(); m++)
    for (size_t c = 0; c < fd.clusters[m].size(); c++) {
      for (std::list<int>::const_iterator it = fd.clusters[m][c].begin(); it != fd.clusters[m][c].end(); ++it) members[pos++] = *it;
      cl_model[nc] = m;
      cl_off[++nc] = pos;
    }
  return nc;
}

#ifdef REF_STEPS_MOPED2

// FILTER_PROJECTION_CPU::process.  Matches of model m: rows [model_off[m], model_off[m+1]) of uv / image_of / xyz;
// objects in list order with their model and pose (qx,qy,qz,qw,tx,ty,tz); images with K and camera pose.
// Out: score[n_obj] = Object::score as process() left it (erased objects too), keep[n_obj], and for the survivors in the
// order process() pushes their clusters -- model after model, list order inside a model -- order[k] = the object's
// index, its rewritten cluster = members[cl_off[k] .. cl_off[k+1]) (indices into the model's matches).  Returns the
// number of survivors.
int ref_filter_step(const float* uv, const int* image_of, const float* xyz, const int* model_off, int n_models,
                    const int* obj_model, const float* obj_pose, int n_obj, const float* Ks, const float* cams,
                    int n_images, int min_points, float feature_distance, float min_score, float* score,
                    unsigned char* keep, int* order, int* members, int* cl_off) {
  FILTER_PROJECTION_CPU alg(min_points, feature_distance, min_score);
  std::vector<SP_Model> models;
  make_models(models, n_models);
  alg.modelsUpdated(models);
  alg._stepName = "FILTER";
  FrameData fd;
  for (int i = 0; i < n_images; i++) fd.images.push_back(make_camera(640, 480, Ks + 4 * i, cams + 7 * i));
  fd.matches.resize(n_models);
  for (int m = 0; m < n_models; m++)
    for (int i = model_off[m]; i < model_off[m + 1]; i++) {
      FrameData::Match mt;
      mt.imageIdx = image_of ? image_of[i] : 0;
      mt.coord2D.init(uv[2 * (size_t)i], uv[2 * (size_t)i + 1]);
      mt.coord3D.init(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
      fd.matches[m].push_back(mt);
    }
  std::list<SP_Object> objects;
  std::vector<SP_Object> all;   // keeps the erased ones alive: their scores are read back
  for (int o = 0; o < n_obj; o++) {
    SP_Object ob(new Object);
    ob->model = models[obj_model[o]];
    ob->pose.rotation.init(obj_pose[7 * o], obj_pose[7 * o + 1], obj_pose[7 * o + 2], obj_pose[7 * o + 3]);
    ob->pose.translation.init(obj_pose[7 * o + 4], obj_pose[7 * o + 5], obj_pose[7 * o + 6]);
    ob->score = 0;
    objects.push_back(ob);
    all.push_back(ob);
  }
  fd.objects = &objects;
  alg.process(fd);
  std::map<const Object*, int> index;
  for (int o = 0; o < n_obj; o++) {
    index[all[o].get()] = o;
    score[o] = all[o]->score;
    keep[o] = 0;
  }
  int k = 0, pos = 0;
  cl_off[0] = 0;
  for (int m = 0; m < n_models; m++) {
    size_t c = 0;
    for (std::list<SP_Object>::const_iterator it = objects.begin(); it != objects.end(); ++it) {
      if ((*it)->model.get() != models[m].get()) continue;
      const int o = index[it->get()];
      keep[o] = 1;
      order[k] = o;
      if (m >= (int)fd.clusters.size() || c >= fd.clusters[m].size()) return -2;   // a survivor without a cluster
      const FrameData::Cluster& cl = fd.clusters[m][c++];
      for (std::list<int>::const_iterator j = cl.begin(); j != cl.end(); ++j) members[pos++] = *j;
      cl_off[++k] = pos;
    }
    if (m < (int)fd.clusters.size() && c != fd.clusters[m].size()) return -3;      // a cluster without a survivor
  }
  return k;
}

#else  // REF_STEPS_MOPED3D

// DEPTHFILTER_CPU::process.  depth_xyzn: h x w x 4 floats (x, y, z, norm); to_filter 1: the n points are ONE list of
// "SIFT" features (n_groups / group_off ignored); to_filter 2: group g = matches[g] = rows [group_off[g],
// group_off[g+1]).  Every feature / match carries its row in imageIdx; keep_out[i] = 1 for the rows that are still
// there afterwards.  Coordinates must lie inside the map (the class indexes its patch arrays without a check).
int ref_depthfilter(const float* depth_xyzn, int w, int h, const float K[4], int patch, float density, int to_filter,
                    const float* uv, const int* group_off, int n_groups, int n, unsigned char* keep_out) {
  DEPTHFILTER_CPU alg(patch, density, to_filter);
  FrameData fd;
  fd.objects = NULL;
  fd.images.push_back(make_camera(w, h, K, CAM_NONE));
  fd.images.push_back(make_float_image(IMAGE_TYPE_DEPTH_MAP, "depth", depth_xyzn, w, h, 4, K));
  for (int i = 0; i < n; i++) keep_out[i] = 0;
  if (to_filter == 1) {
    std::vector<FrameData::DetectedFeature>& f = fd.detectedFeatures["SIFT"];
    f.resize(n);
    for (int i = 0; i < n; i++) {
      f[i].imageIdx = i;
      f[i].coord2D.init(uv[2 * (size_t)i], uv[2 * (size_t)i + 1]);
    }
    alg.process(fd);
    std::vector<FrameData::DetectedFeature>& g = fd.detectedFeatures["SIFT"];
    for (size_t i = 0; i < g.size(); i++) keep_out[g[i].imageIdx] = 1;
  } else if (to_filter == 2) {
    fd.matches.resize(n_groups);
    for (int m = 0; m < n_groups; m++)
      for (int i = group_off[m]; i < group_off[m + 1]; i++) {
        FrameData::Match mt;
        mt.imageIdx = i;
        mt.coord2D.init(uv[2 * (size_t)i], uv[2 * (size_t)i + 1]);
        mt.coord3D.init(0.f, 0.f, 0.f);
        fd.matches[m].push_back(mt);
      }
    alg.process(fd);
    for (size_t m = 0; m < fd.matches.size(); m++)
      for (size_t i = 0; i < fd.matches[m].size(); i++) keep_out[fd.matches[m][i].imageIdx] = 1;
  } else {
    return -1;
  }
  return 0;
}

// DEPTHMAP_PROP_CPU::process over n matches at uv.  fill_or_null: h x w floats, handed over as the PROB_MAP the class
// looks for (named <depth map's name>.distance), or NULL = no such image.  Out per match: depthData.coord3D, .depth,
// .fillDistance, and (optional) .depthValid.  Coordinates must lie inside the map.
int ref_depthmap_prop(const float* depth_xyzn, const float* fill_or_null, int w, int h, const float* uv, int n,
                      float* coord3d_out, float* depth_out, float* fill_distance_out, unsigned char* valid_out_or_null) {
  DEPTHMAP_PROP_CPU alg;
  FrameData fd;
  fd.objects = NULL;
  fd.images.push_back(make_camera(w, h, K_NONE, CAM_NONE));
  fd.images.push_back(make_float_image(IMAGE_TYPE_DEPTH_MAP, "depth", depth_xyzn, w, h, 4, K_NONE));
  if (fill_or_null) fd.images.push_back(make_float_image(IMAGE_TYPE_PROB_MAP, "depth.distance", fill_or_null, w, h, 1, K_NONE));
  fd.matches.resize(1);
  fd.matches[0].resize(n);
  for (int i = 0; i < n; i++) {
    FrameData::Match& mt = fd.matches[0][i];
    mt.imageIdx = 0;
    mt.coord2D.init(uv[2 * (size_t)i], uv[2 * (size_t)i + 1]);
    mt.coord3D.init(0.f, 0.f, 0.f);
    mt.depthData.depthValid = false;
    mt.depthData.coord3D.init(-7.f, -7.f, -7.f);   // (a process() that returns early is seen)
    mt.depthData.depth = -7.f;
    mt.depthData.fillDistance = -7.f;
  }
  alg.process(fd);
  for (int i = 0; i < n; i++) {
    const depthInformation& d = fd.matches[0][i].depthData;
    for (int k = 0; k < 3; k++) coord3d_out[3 * (size_t)i + k] = d.coord3D[k];
    depth_out[i] = d.depth;
    fill_distance_out[i] = d.fillDistance;
    if (valid_out_or_null) valid_out_or_null[i] = d.depthValid ? 1 : 0;
  }
  return 0;
}

#endif

}  // extern "C"
