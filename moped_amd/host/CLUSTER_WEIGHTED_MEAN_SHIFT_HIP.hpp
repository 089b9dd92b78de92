// CLUSTER_WEIGHTED_MEAN_SHIFT_HIP -- moped3d only: drop-in for CLUSTER_WEIGHTED_MEAN_SHIFT_CPU
// (moped3d/libmoped/src/cluster/CLUSTER_WEIGHTED_MEAN_SHIFT_CPU.hpp, one of the CLUSTER classes config.hpp:21-25 includes):
//     pipeline.addAlg( "CLUSTER", new CLUSTER_WEIGHTED_MEAN_SHIFT_HIP( 0.1, 0.02, 7, 100, 10 ) );
//     pipeline.addAlg( "CLUSTER", new CLUSTER_WEIGHTED_MEAN_SHIFT_CPU( 0.1, 0.02, 7, 100, 10 ) );   // fallback
// Same five constructor arguments (Radius, Merge, MinPts, MaxIterations, halfWeightDistance) and config keys.
// Reads matches[model] (imageIdx, depthData.coord3D, depthData.fillDistance) -- what DEPTHMAP_PROP left, no map of its
// own; writes clusters[model]: per image, in image order, the reference's clusters in its order, member indices =
// positions in THAT image's list of the model's matches, descending (:188-206).  The clusters may overlap.  Sets
// oldClusters when the step is named "CLUSTER" (:207).  A (model, image) list of more than 2048 matches is more than
// the device takes: the step then warns and leaves the frame without clusters.
#pragma once
#include "hip_frame3d.hpp"

namespace MopedNS {

class CLUSTER_WEIGHTED_MEAN_SHIFT_HIP : public MopedAlg {
  Float Radius;
  Float Merge;
  int MinPts;
  int MaxIterations;
  Float halfWeightDistance;

 public:
  CLUSTER_WEIGHTED_MEAN_SHIFT_HIP(Float Radius, Float Merge, unsigned int MinPts, unsigned int MaxIterations,
                                  Float halfWeightDistance)
      : Radius(Radius), Merge(Merge), MinPts(MinPts), MaxIterations(MaxIterations), halfWeightDistance(halfWeightDistance) {
    // (a negative or NaN Radius / Merge / halfWeightDistance is the CPU step's to make sense of)
    capable = Radius >= 0 && Merge >= 0 && halfWeightDistance >= 0 && this->MaxIterations >= 0 && HipSession::get() != 0;
  }

  void getConfig(map<string, string>& config) const {
    hipGetConfig(config, _stepName, _alg, "CLUSTER_WEIGHTED_MEAN_SHIFT_HIP", "Radius", Radius);
    hipGetConfig(config, _stepName, _alg, "CLUSTER_WEIGHTED_MEAN_SHIFT_HIP", "Merge", Merge);
    hipGetConfig(config, _stepName, _alg, "CLUSTER_WEIGHTED_MEAN_SHIFT_HIP", "MinPts", MinPts);
    hipGetConfig(config, _stepName, _alg, "CLUSTER_WEIGHTED_MEAN_SHIFT_HIP", "MaxIterations", MaxIterations);
    hipGetConfig(config, _stepName, _alg, "CLUSTER_WEIGHTED_MEAN_SHIFT_HIP", "halfWeightDistance", halfWeightDistance);
  }

  void process(FrameData& frameData) {
    frameData.clusters.resize(models->size());
    mh_ctx* ctx = HipSession::get();
    // one problem per (model, image), in that order: the points process() hands to WeighedMeanShift (:195-204)
    const int n_models = (int)frameData.matches.size(), n_images = (int)frameData.images.size();
    vector<float> xyz, fill;
    vector<int32_t> off(1, 0);
    for (int model = 0; model < n_models; ++model) {
      const vector<FrameData::Match>& mm = frameData.matches[model];
      for (int i = 0; i < n_images; ++i) {
        for (int k = 0; k < (int)mm.size(); ++k) {
          if (mm[k].imageIdx != i) continue;
          xyz.push_back(mm[k].depthData.coord3D[0]);
          xyz.push_back(mm[k].depthData.coord3D[1]);
          xyz.push_back(mm[k].depthData.coord3D[2]);
          fill.push_back(mm[k].depthData.fillDistance);
        }
        off.push_back((int32_t)fill.size());
      }
    }
    const int n_problems = (int)off.size() - 1, total = off[n_problems];
    if (total > 0) {
      mh_wms_params prm;
      prm.radius = Radius;
      prm.merge = Merge;
      prm.min_pts = MinPts;
      prm.max_iter = MaxIterations;
      prm.half_weight_distance = halfWeightDistance;
      // room for four memberships per match; a scene with more overlap says what it needs and is asked again
      vector<int32_t> ncl(n_problems), cl_off((size_t)total + 1), members(4 * (size_t)total);
      int64_t needed[2] = {0, 0};
      int rc = mh_cluster_wms(ctx, &xyz[0], &fill[0], &off[0], n_problems, &prm, &ncl[0], &cl_off[0], (int)cl_off.size() - 1,
                              &members[0], (int)members.size(), needed);
      if (rc == MH_ERR_CAPACITY && needed[0] < 0x7fffffff && needed[1] < 0x7fffffff) {
        cl_off.resize((size_t)needed[0] + 1);
        members.resize((size_t)needed[1] + 1);
        rc = mh_cluster_wms(ctx, &xyz[0], &fill[0], &off[0], n_problems, &prm, &ncl[0], &cl_off[0], (int)cl_off.size() - 1,
                            &members[0], (int)members.size(), needed);
      }
      if (rc != MH_OK) {
        HipSession::warn("mh_cluster_wms");
      } else {
        int k = 0;
        for (int p = 0; p < n_problems; ++p) {
          vector<FrameData::Cluster>& out = frameData.clusters[p / n_images];   // all images of a model append to its list
          for (int c = 0; c < ncl[p]; ++c, ++k) {
            out.resize(out.size() + 1);
            FrameData::Cluster& cl = out.back();
            for (int j = cl_off[k]; j < cl_off[k + 1]; ++j) cl.push_back(members[j]);
          }
        }
      }
    }
    if (_stepName == "CLUSTER") frameData.oldClusters = frameData.clusters;
  }
};

}  // namespace MopedNS
