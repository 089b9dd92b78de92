// getObjectHulls_HIP (object_hulls_hip.hpp) from a scene file, hulls out in the line format of MopedBench's
// outputObjectCH (moped3d/libmoped/src/MopedBench.cpp:164-172):  <step>:OBJHULL:<model name>:<x>;<y>:<x>;<y>...
// (tests/test_gpu_object_hulls_host.py writes the scene and compares the lines with the Python path).
//
//   object_hulls_test <scene file> [digits] [loops]  digits: the stream's precision (default 6, as MopedBench prints)
//
// loops > 0: the same hulls again by a plain host loop on one thread (hostHull below: project, std::sort, a vector as the
// chain's stack), compared vertex by vertex with the device's, and both timed over `loops` rounds -- the lines
// "TIMING host ..." / "TIMING device ..." on stderr (scripts/bench_object_hulls.py reads them).
//
// scene file, whitespace-separated:   K fx fy cx cy | CAM qx qy qz qw tx ty tz | MODEL name n  x y z ... |
//                                     OBJECT model-index qx qy qz qw tx ty tz
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "moped_types.hpp"
#include "object_hulls_hip.hpp"

using namespace MopedNS;

namespace {

struct P2 {
  float x, y;
  bool operator<(const P2& o) const { return x != o.x ? x < o.x : y < o.y; }
};

// one direction of the chain over seq[first], seq[first + step] ...: pop while the turn is not strictly convex
void halfChain(const std::vector<P2>& seq, int first, int last, int step, std::vector<P2>& st) {
  st.clear();
  for (int i = first; i != last + step; i += step) {
    const P2 q = seq[i];
    while (st.size() >= 2) {
      const P2 &a = st[st.size() - 2], &b = st[st.size() - 1];
      const float det = (a.x - b.x) * (q.y - b.y) - (q.x - b.x) * (a.y - b.y);
      if (det <= 0) st.pop_back();
      else break;
    }
    st.push_back(q);
  }
}

// the hull of one object on the host: the model's points through the pose and the camera (points with z < 0.001 left
// out, as the device leaves them out), sorted, chained forward and back; vertices in the device's order
void hostHull(const Model& model, const Pose& pose, const Image& image, std::vector<P2>& pts, std::vector<P2>& fwd,
              std::vector<P2>& bwd, std::vector<P2>& hull) {
  const mh_cam cam = hipCamOf(image);
  float R[2][9];
  const float* q[2] = {&pose.rotation[0], cam.cam};
  for (int k = 0; k < 2; ++k) {
    const float x = q[k][0], y = q[k][1], z = q[k][2], w = q[k][3];
    const float r[9] = {1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
                        2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                        2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y};
    for (int i = 0; i < 9; ++i) R[k][i] = r[i];
  }
  const std::vector<Model::IP>& ips = model.IPs.find("SIFT")->second;
  pts.clear();
  for (size_t i = 0; i < ips.size(); ++i) {
    const float X = ips[i].coord3D[0], Y = ips[i].coord3D[1], Z = ips[i].coord3D[2];
    const float wx = X * R[0][0] + Y * R[0][1] + Z * R[0][2] + pose.translation[0] - cam.cam[4];
    const float wy = X * R[0][3] + Y * R[0][4] + Z * R[0][5] + pose.translation[1] - cam.cam[5];
    const float wz = X * R[0][6] + Y * R[0][7] + Z * R[0][8] + pose.translation[2] - cam.cam[6];
    const float cx = wx * R[1][0] + wy * R[1][3] + wz * R[1][6];
    const float cy = wx * R[1][1] + wy * R[1][4] + wz * R[1][7];
    const float cz = wx * R[1][2] + wy * R[1][5] + wz * R[1][8];
    if (cz < 0.001) continue;
    const P2 p = {cx / cz * cam.K[0] + cam.K[2], cy / cz * cam.K[1] + cam.K[3]};
    pts.push_back(p);
  }
  hull.clear();
  if (pts.size() < 2) return;
  std::sort(pts.begin(), pts.end());
  const int n = (int)pts.size();
  halfChain(pts, 0, n - 1, 1, fwd);
  halfChain(pts, n - 1, 0, -1, bwd);
  for (int i = (int)bwd.size() - 2; i >= 0; --i) hull.push_back(bwd[i]);
  for (int i = (int)fwd.size() - 2; i >= 0; --i) hull.push_back(fwd[i]);
}

double nowSeconds() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: object_hulls_test <scene file> [digits]" << std::endl;
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::cerr << "cannot read " << argv[1] << std::endl;
    return 2;
  }
  if (argc > 2) std::cout.precision(std::atoi(argv[2]));
  Image image;
  image.width = 640;
  image.height = 480;
  image.intrinsicLinearCalibration.init(0.f, 0.f, 0.f, 0.f);
  image.cameraPose.rotation.init(0.f, 0.f, 0.f, 1.f);
  image.cameraPose.translation.init(0.f, 0.f, 0.f);
  std::vector<SP_Model> models;
  std::list<SP_Object> objects;
  std::string word;
  while (in >> word) {
    if (word == "K") {
      for (int i = 0; i < 4; ++i) in >> image.intrinsicLinearCalibration[i];
    } else if (word == "CAM") {
      for (int i = 0; i < 4; ++i) in >> image.cameraPose.rotation[i];
      for (int i = 0; i < 3; ++i) in >> image.cameraPose.translation[i];
    } else if (word == "MODEL") {
      SP_Model m(new Model);
      size_t n = 0;
      in >> m->name >> n;
      std::vector<Model::IP>& ips = m->IPs["SIFT"];
      ips.resize(n);
      for (size_t i = 0; i < n; ++i) {
        in >> ips[i].coord3D[0] >> ips[i].coord3D[1] >> ips[i].coord3D[2];
        ips[i].descriptor.assign(MH_DESC_DIM, 0.f);
        ips[i].descriptor[(i + models.size()) % MH_DESC_DIM] = 1.f;   // (unit rows: the hull does not read them)
      }
      models.push_back(m);
    } else if (word == "OBJECT") {
      size_t m = 0;
      SP_Object o(new Object);
      in >> m;
      for (int i = 0; i < 4; ++i) in >> o->pose.rotation[i];
      for (int i = 0; i < 3; ++i) in >> o->pose.translation[i];
      if (!in || m >= models.size()) {
        std::cerr << "bad OBJECT record" << std::endl;
        return 2;
      }
      o->model = models[m];
      o->score = 0;
      objects.push_back(o);
    } else {
      std::cerr << "unknown record " << word << std::endl;
      return 2;
    }
  }
  mh_ctx* ctx = HipSession::get();
  if (!ctx) {
    std::cerr << "no gfx950 device" << std::endl;
    return 3;
  }
  HipModelTable table;   // Update() of a MATCH step: the models' rows to the device
  if (!table.update(ctx, models, "SIFT", 0) || table.skipCalculation) {
    std::cerr << "model upload failed: " << mh_last_error(ctx) << std::endl;
    return 3;
  }
  std::vector<std::list<Pt<2> > > hulls;
  std::vector<int> behind;
  if (!getObjectHulls_HIP(ctx, models, objects, image, hulls, &behind, 16)) {   // (16: the larger hulls take the second round)
    std::cerr << "getObjectHulls_HIP failed" << std::endl;
    return 4;
  }
  size_t i = 0;
  for (std::list<SP_Object>::const_iterator it = objects.begin(); it != objects.end(); ++it, ++i) {
    std::cout << "HULLS:OBJHULL:" << (*it)->model->name;
    for (std::list<Pt<2> >::const_iterator p = hulls[i].begin(); p != hulls[i].end(); ++p) std::cout << ":" << (*p)[0] << ";" << (*p)[1];
    std::cout << std::endl;
    std::cerr << "behind " << behind[i] << std::endl;
  }
  const int loops = argc > 3 ? std::atoi(argv[3]) : 0;
  if (loops > 0) {
    std::vector<P2> pts, fwd, bwd, hull;
    std::vector<std::vector<P2> > hostHulls;
    const double t0 = nowSeconds();
    for (int r = 0; r < loops; ++r) {
      hostHulls.clear();
      for (std::list<SP_Object>::const_iterator it = objects.begin(); it != objects.end(); ++it) {
        hostHull(*(*it)->model, (*it)->pose, image, pts, fwd, bwd, hull);
        hostHulls.push_back(hull);
      }
    }
    const double t1 = nowSeconds();
    for (int r = 0; r < loops; ++r)
      if (!getObjectHulls_HIP(ctx, models, objects, image, hulls, 0, 64)) return 4;
    const double t2 = nowSeconds();
    size_t differing = 0, vertices = 0;
    for (size_t o = 0; o < hulls.size(); ++o) {
      vertices += hulls[o].size();
      bool same = hulls[o].size() == hostHulls[o].size();
      size_t v = 0;
      for (std::list<Pt<2> >::const_iterator p = hulls[o].begin(); same && p != hulls[o].end(); ++p, ++v)
        same = (*p)[0] == hostHulls[o][v].x && (*p)[1] == hostHulls[o][v].y;
      differing += same ? 0 : 1;
    }
    const double per = 1e6 / ((double)loops * (double)objects.size());
    std::cerr << "TIMING host " << (t1 - t0) * per << " us/hull device " << (t2 - t1) * per << " us/hull objects " << objects.size()
              << " loops " << loops << " vertices/hull " << (double)vertices / (double)hulls.size() << " hulls differing " << differing
              << std::endl;
  }
  return 0;
}
