// CLUSTER_LINKAGE_HIP -- moped3d only: drop-in for CLUSTER_LINKAGE_CPU
// (moped3d/libmoped/src/cluster/CLUSTER_LINKAGE_CPU.hpp, config.hpp:45):
//     pipeline.addAlg( "CLUSTER", new CLUSTER_LINKAGE_HIP( 0.1, 7, 2, 1, 0.0, 1, -1, -1 ) );
//     pipeline.addAlg( "CLUSTER", new CLUSTER_LINKAGE_CPU( 0.1, 7, 2, 1, 0.0, 1, -1, -1 ) );   // fallback
// Same constructor arguments (WeightGamma and Alpha are unused by the reference as well: its
// adaptiveWeightSum call passes 0.5 and 25, :697).  LinkageType 0 (minimum), 1 (average: the shipped
// configuration) and 2 (maximum) as the reference's update loop has them (:506-526).
// One key of its own: RowMaxima (default 0; 1 = MH_LINKAGE_ROWMAX for this step's call -- the same clusters, match
// lists of up to 4096 per model where the default refuses more than 1024; the session's mode is put back afterwards).
// Reads matches[model] (coord2D, coord3D, depthData.coord3D), the depth map and its ".distance"
// map (:577-593); writes clusters[model] in the reference's cluster and member order; sets
// oldClusters when the step is named "CLUSTER" (:703).
#pragma once
#include "hip_frame3d.hpp"

namespace MopedNS {

class CLUSTER_LINKAGE_HIP : public MopedAlg {
  Float Cutoff;
  int MinPts;
  int Use3DFilter;
  Float WeightGamma;
  Float Alpha;
  int LinkageType;
  Float Sigma2D;
  Float Sigma3D;
  int RowMaxima;   // 0 / 1 (a config value)

 public:
  CLUSTER_LINKAGE_HIP(Float Cutoff, int MinPts, int Use3DFilter, Float WeightGamma, Float Alpha, int LinkageType,
                      Float Sigma2D, Float Sigma3D)
      : Cutoff(Cutoff), MinPts(MinPts), Use3DFilter(Use3DFilter), WeightGamma(WeightGamma), Alpha(Alpha),
        LinkageType(LinkageType), Sigma2D(Sigma2D), Sigma3D(Sigma3D), RowMaxima(0) {
    capable = LinkageType >= 0 && LinkageType <= 2 && HipSession::get() != 0;
  }

  void getConfig(map<string, string>& config) const {
    hipGetConfig(config, _stepName, _alg, "CLUSTER_LINKAGE_HIP", "Cutoff", Cutoff);
    hipGetConfig(config, _stepName, _alg, "CLUSTER_LINKAGE_HIP", "MinPts", MinPts);
    hipGetConfig(config, _stepName, _alg, "CLUSTER_LINKAGE_HIP", "Use3DFilter", Use3DFilter);
    hipGetConfig(config, _stepName, _alg, "CLUSTER_LINKAGE_HIP", "WeightGamma", WeightGamma);
    hipGetConfig(config, _stepName, _alg, "CLUSTER_LINKAGE_HIP", "Alpha", Alpha);
    hipGetConfig(config, _stepName, _alg, "CLUSTER_LINKAGE_HIP", "LinkageType", LinkageType);
    hipGetConfig(config, _stepName, _alg, "CLUSTER_LINKAGE_HIP", "RowMaxima", RowMaxima);
  }
  void setConfig(map<string, string>& config) {
    hipSetConfig(config, _stepName, _alg, "CLUSTER_LINKAGE_HIP", "RowMaxima", RowMaxima);
  }

  void process(FrameData& frameData) {
    frameData.clusters.resize(models->size());
    mh_ctx* ctx = HipSession::get();
    Image *depthmap, *distanceMap;   // the FIRST depth map of the frame: the reference's loop breaks (:577-593)
    if (!hipFindDepthMaps(frameData, true, depthmap, distanceMap)) return;
    // (uploaded by this step only if no depth step of this frame has done so: HipDepthMaps, hip_session.hpp)
    if (!HipDepthMaps::get().ensure(ctx, depthmap, distanceMap)) {
      HipSession::warn("mh_frame_set_depth_image_host");
      return;
    }
    // every model's matches in ONE call
    vector<mh_corr> corr;
    vector<mh_depth> depth;
    vector<int32_t> off(1, 0);
    for (int model = 0; model < (int)frameData.matches.size(); ++model) {
      const vector<FrameData::Match>& mm = frameData.matches[model];
      for (int k = 0; k < (int)mm.size(); ++k) {
        mh_corr c;
        c.u = mm[k].coord2D[0]; c.v = mm[k].coord2D[1];
        c.x = mm[k].coord3D[0]; c.y = mm[k].coord3D[1]; c.z = mm[k].coord3D[2];
        mh_depth d;
        d.wx = mm[k].depthData.coord3D[0]; d.wy = mm[k].depthData.coord3D[1]; d.wz = mm[k].depthData.coord3D[2];
        d.w = 1.f;
        corr.push_back(c);
        depth.push_back(d);
      }
      off.push_back((int32_t)corr.size());
    }
    const int n_problems = (int)frameData.matches.size(), total = off[n_problems];
    if (total > 0) {
      mh_linkage_params prm;
      prm.cutoff = Cutoff;
      prm.min_pts = MinPts;
      prm.use3d_filter = Use3DFilter;
      prm.sigma2d = Sigma2D;
      prm.sigma3d = Sigma3D;
      prm.linkage_type = LinkageType;
      vector<int32_t> label(total), order(total), ncl(n_problems);
      // the session's context is shared: the mode is this step's for its own call only
      struct Mode {
        mh_ctx* ctx;
        bool on;
        int before;   // what another user of the session left: put back afterwards
        Mode(mh_ctx* c, bool o) : ctx(c), on(o), before(MH_LINKAGE_SCAN) {
          if (on && mh_linkage_get_mode(ctx, &before) == MH_OK) mh_linkage_set_mode(ctx, MH_LINKAGE_ROWMAX);
        }
        ~Mode() { if (on) mh_linkage_set_mode(ctx, before); }
      } mode(ctx, RowMaxima != 0);
      if (mh_cluster_linkage(ctx, &corr[0], &depth[0], &off[0], n_problems, &prm, &label[0], &order[0], &ncl[0]) != MH_OK) {
        HipSession::warn("mh_cluster_linkage");
      } else {
        for (int p = 0; p < n_problems; ++p) {
          const int b = off[p], n = off[p + 1] - b;
          int pos = 0;
          for (int c = 0; c < ncl[p]; ++c) {
            frameData.clusters[p].resize(frameData.clusters[p].size() + 1);
            FrameData::Cluster& cl = frameData.clusters[p].back();
            while (pos < n && order[b + pos] >= 0 && label[b + order[b + pos]] == c) cl.push_back(order[b + pos++]);
          }
        }
      }
    }
    if (_stepName == "CLUSTER") frameData.oldClusters = frameData.clusters;
  }
};

}  // namespace MopedNS
