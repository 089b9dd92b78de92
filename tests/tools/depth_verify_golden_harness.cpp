// Records what the reference's own DEPTH_VERIFY_CPU (moped3d/libmoped/src/depthVerify/DEPTH_VERIFY_CPU.hpp) prints and
// keeps for the cases of a case file.  Test infrastructure of tests/tools/make_depth_verify_golden.py: built against the
// reference headers where they lie (-I <reference>/moped3d/libmoped/include -I <reference>/moped3d/libmoped/src/depthVerify),
// run when the golden is made, never needed by a test.
//
// The class prints, per object, raw QS and IS, the multiplier before the cap, both counts and the adjusted scores to
// std::cerr (:192-202).  Here cerr's buffer is a string stream with precision 9 -- decimals that parse back to the same
// float32 -- and the text of every case goes to the output file behind a line "CASE <c> <n_obj>", followed by a line
// "KEPT <flag per object>" (which objects process() left in frameData.objects, by pointer).
//
//   in : int32 n_cases, then per case
//        float32 prm[4] (FeatureDistance, MaxMultiplier, MaxDistance, DepthFraction); float32 K[4], cam[7] (the image);
//        float32 dK[4], dcam[7] (the depth map); int32 w, h; float32 depth[h][w][4]; float32 fill[h][w];
//        int32 n_models; int32 kp_off[n_models + 1]; float32 kp[..][3]; int32 m_off[n_models + 1]; float32 match[..][5]
//        (u, v, x, y, z); int32 n_obj; int32 obj_model[n_obj]; float32 obj_pose[n_obj][7]
//   out: text
#include <moped.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <vector>

// ---- stand-ins for src/util.hpp: what the class uses of it ----
#define GET_CONFIG(v) (void)0
#define SET_CONFIG(v) (void)0
namespace dv_harness {
// the state of one erase-safe walk: the body may assign `cur` (the list's erase() returns the next element)
template <class It>
struct Walk {
  It cur, seen;
  bool once;
  explicit Walk(It first) : cur(first), seen(first), once(false) {}
  bool more(It last) {
    if (cur == last) return false;
    seen = cur;
    once = true;
    return true;
  }
  void step() {
    if (cur == seen) ++cur;   // (the body did not erase)
  }
};
}  // namespace dv_harness
// for every element `i` of container c, `it` its iterator; the body may do it = c.erase(it), and may `continue`
#define eforeach(i, it, c)                                                                                      \
  for (dv_harness::Walk<typeof((c).begin())> it##_walk((c).begin()); it##_walk.more((c).end()); it##_walk.step()) \
    for (typeof((c).begin())& it = it##_walk.cur; it##_walk.once;)                                                \
      for (typeof(*(c).begin())& i = *it; it##_walk.once; it##_walk.once = false)
namespace MopedNS {
struct FrameData {
  struct Match {
    int imageIdx;
    Pt<2> coord2D;
    Pt<3> coord3D;
  };
  vector<SP_Image> images;
  vector<vector<Match> > matches;
  list<SP_Object>* objects;
};
class MopedAlg {
 public:
  vector<SP_Model>* models;
  bool capable, configUpdated;
  string _stepName;
  int _alg;
  MopedAlg() : models(0), capable(true), configUpdated(true), _alg(0) {}
  virtual ~MopedAlg() {}
  virtual void getConfig(map<string, string>&) const {}
  virtual void setConfig(map<string, string>&) {}
  virtual void process(FrameData&) = 0;
};
}  // namespace MopedNS

#include <DEPTH_VERIFY_CPU.hpp>

template <class T>
static void rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n + 1);
  if (n && fread(&v[0], sizeof(T), n, f) != n) exit(4);
}
static int rd_int(FILE* f) {
  int v = 0;
  if (fread(&v, 4, 1, f) != 1) exit(4);
  return v;
}

int main(int argc, char** argv) {
  using namespace MopedNS;
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  FILE* out = fopen(argv[2], "w");
  if (!out) return 5;
  const int n_cases = rd_int(in);
  std::ostringstream text;
  std::streambuf* const cerr_buf = std::cerr.rdbuf(text.rdbuf());
  std::cerr.precision(9);
  for (int c = 0; c < n_cases; ++c) {
    std::vector<float> prm, K, cam, dK, dcam, depth, fill, kp, match, obj_pose;
    std::vector<int> kp_off, m_off, obj_model;
    rd(in, prm, 4);
    rd(in, K, 4);
    rd(in, cam, 7);
    rd(in, dK, 4);
    rd(in, dcam, 7);
    const int w = rd_int(in), h = rd_int(in);
    rd(in, depth, 4 * (size_t)w * h);
    rd(in, fill, (size_t)w * h);
    const int n_models = rd_int(in);
    rd(in, kp_off, (size_t)n_models + 1);
    rd(in, kp, 3 * (size_t)kp_off[n_models]);
    rd(in, m_off, (size_t)n_models + 1);
    rd(in, match, 5 * (size_t)m_off[n_models]);
    const int n_obj = rd_int(in);
    rd(in, obj_model, n_obj);
    rd(in, obj_pose, 7 * (size_t)n_obj);

    FrameData fd;
    SP_Image gray(new Image(IMAGE_TYPE_GRAY_IMAGE));
    gray->name = "image";
    gray->width = gray->height = 0;
    gray->intrinsicLinearCalibration.init(K[0], K[1], K[2], K[3]);
    for (int k = 0; k < 7; ++k) gray->cameraPose[k] = cam[k];
    gray->TM.init(gray->cameraPose);
    SP_Image dimg(new Image(IMAGE_TYPE_DEPTH_MAP));
    dimg->name = "depth";
    dimg->width = w;
    dimg->height = h;
    dimg->intrinsicLinearCalibration.init(dK[0], dK[1], dK[2], dK[3]);
    for (int k = 0; k < 7; ++k) dimg->cameraPose[k] = dcam[k];
    dimg->TM.init(dimg->cameraPose);
    dimg->data.resize(16 * (size_t)w * h);
    memcpy(&dimg->data[0], &depth[0], 16 * (size_t)w * h);
    SP_Image fimg(new Image(IMAGE_TYPE_PROB_MAP));
    fimg->name = "depth.distance";
    fimg->width = w;
    fimg->height = h;
    fimg->data.resize(4 * (size_t)w * h);
    memcpy(&fimg->data[0], &fill[0], 4 * (size_t)w * h);
    fd.images.push_back(gray);
    fd.images.push_back(dimg);
    fd.images.push_back(fimg);

    std::vector<SP_Model> models;
    fd.matches.resize(n_models);
    for (int m = 0; m < n_models; ++m) {
      SP_Model mod(new Model);
      char name[32];
      snprintf(name, sizeof name, "model%04d", m);
      mod->name = name;
      std::vector<Model::IP>& ips = mod->IPs["SIFT"];
      for (int j = kp_off[m]; j < kp_off[m + 1]; ++j) {
        Model::IP ip;
        ip.coord3D.init(kp[3 * j], kp[3 * j + 1], kp[3 * j + 2]);
        ips.push_back(ip);
      }
      models.push_back(mod);
      for (int i = m_off[m]; i < m_off[m + 1]; ++i) {
        FrameData::Match mt;
        mt.imageIdx = 0;
        mt.coord2D.init(match[5 * i], match[5 * i + 1]);
        mt.coord3D.init(match[5 * i + 2], match[5 * i + 3], match[5 * i + 4]);
        fd.matches[m].push_back(mt);
      }
    }
    list<SP_Object> objects;
    std::vector<Object*> before;
    for (int o = 0; o < n_obj; ++o) {
      SP_Object ob(new Object);
      ob->model = models[obj_model[o]];
      for (int k = 0; k < 7; ++k) ob->pose[k] = obj_pose[7 * o + k];
      ob->score = 0;
      objects.push_back(ob);
      before.push_back(ob.get());
    }
    fd.objects = &objects;

    DEPTH_VERIFY_CPU alg(prm[0], prm[1], prm[2], prm[3]);
    alg.models = &models;
    alg._stepName = "DEPTH_VERIFY";
    text.str("");
    alg.process(fd);
    fprintf(out, "CASE %d %d\n%s", c, n_obj, text.str().c_str());
    fprintf(out, "KEPT");
    for (int o = 0; o < n_obj; ++o) {
      bool kept = false;
      for (list<SP_Object>::iterator it = objects.begin(); it != objects.end(); ++it) kept = kept || it->get() == before[o];
      fprintf(out, " %d", kept ? 1 : 0);
    }
    fprintf(out, "\n");
  }
  std::cerr.rdbuf(cerr_buf);
  fclose(in);
  fclose(out);
  return 0;
}
