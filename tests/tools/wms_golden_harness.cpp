// Records what the reference's own CLUSTER_WEIGHTED_MEAN_SHIFT_CPU (moped3d/libmoped/src/cluster/
// CLUSTER_WEIGHTED_MEAN_SHIFT_CPU.hpp) returns for the cases of a case file.  Test infrastructure of
// tests/tools/make_wms_golden.py: built against the reference headers where they lie (-I <reference>/moped3d/libmoped/include
// -I <reference>/moped3d/libmoped/src/cluster), run when the golden is made, never needed by a test.
//
// Two builds of this file:
//   plain            process() as a pipeline calls it: the clusters of model 0, all images appended.
//   -DWMS_INSTRUMENT the same, and WeighedMeanShift<3> once more per image with its locals observed from outside, the header
//                    itself untouched: `bool` is a stand-in type inside the header whose assignments are seen (active[i], the
//                    `done = true` that opens every iteration), and the block `can` lives in is copied when the function frees
//                    it (replaced global operator new / delete).  The two builds' clusters must agree (the maker checks).
//
//   in : int32 n_cases; float32 prm[n_cases][3] (Radius, Merge, halfWeightDistance); int32 iprm[n_cases][3] (MinPts,
//        MaxIterations, images); int32 off[n_cases + 1]; float32 xyz[total][3]; float32 fill[total]; int32 image[total]
//   out: int32 n_cases; int32 ncl[n_cases]; int32 n_all; int32 cl_off[n_all + 1]; int32 members[cl_off[n_all]]
//        instrumented, behind that: int32 n_problems (cases x images, in order); int32 poff[n_problems + 1]; int32 iterations
//        [n_problems]; float32 weight[poff[n_problems]]; float32 centre[..][3]; int32 active[..] -- by (problem, position)
#include <moped.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

// ---- stand-ins for src/util.hpp: what the class uses of it ----
#define GET_CONFIG(v) (void)0
#define SET_CONFIG(v) (void)0
namespace MopedNS {
struct depthInformation {
  bool depthValid;
  Pt<3> coord3D;
  Float depth;
  Float fillDistance;
};
struct FrameData {
  struct Match {
    int imageIdx;
    Pt<2> coord2D;
    Pt<3> coord3D;
    depthInformation depthData;
  };
  typedef list<int> Cluster;
  vector<SP_Image> images;
  vector<vector<Match> > matches;
  vector<vector<Cluster> > clusters;
  vector<vector<Cluster> > oldClusters;
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

#ifdef WMS_INSTRUMENT
// What the observation relies on, checked at run time where it can be (abort / exit status 6 / the maker's comparison of the
// two builds' clusters): libstdc++'s std::vector allocates exactly n * sizeof(T) in reserve() through the global operator new
// and frees through the global operator delete without touching the block; a function's by-value vector arguments are
// copied (one allocation each) before its body runs; WeighedMeanShift's first assignment to a `bool` is active[0] = true and
// `done` lives on the stack, outside active's block.  Another standard library or a changed header needs these re-read.
static bool g_armed = false;
static int g_n = 0, g_iterations = 0, g_allocs = 0;
static const char* g_active_base = 0;
static std::vector<int> g_active;
static void* g_can = 0;
static std::vector<char> g_can_copy;
struct wms_bool {
  unsigned char v;
  wms_bool() {}
  wms_bool(bool b) : v(b) {}
  operator bool() const { return v != 0; }
  wms_bool& operator=(bool b) {
    v = b;
    if (g_armed) {
      const char* me = reinterpret_cast<const char*>(this);
      if (!g_active_base) g_active_base = me;   // the first assignment of a call is active[0] = true
      if (me >= g_active_base && me < g_active_base + g_n) g_active[me - g_active_base] = b;
      else if (b) ++g_iterations;               // `done = true`: an iteration begins
    }
    return *this;
  }
};
void* operator new(size_t sz) throw(std::bad_alloc) {
  void* p = malloc(sz ? sz : 1);
  if (!p) throw std::bad_alloc();
  // inside an observed call: the two by-value copies, active's block, then can's (n Canopy<3> of 24 bytes)
  if (g_armed && !g_can && ++g_allocs == 4) {
    if (sz != (size_t)g_n * 24) abort();
    g_can = p;
  }
  return p;
}
void operator delete(void* p) throw() {
  if (g_armed && p && p == g_can) {
    g_can_copy.assign((char*)p, (char*)p + (size_t)g_n * 24);
    g_can = 0;
    g_armed = false;   // (nothing of the call is observed after this)
  }
  free(p);
}
#define bool wms_bool
#define class struct   // (the class has no access specifier before its members: default access)
#endif
#include <CLUSTER_WEIGHTED_MEAN_SHIFT_CPU.hpp>
#ifdef WMS_INSTRUMENT
#undef bool
#undef class
#endif

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n + 1);
  return n == 0 || fread(&v[0], sizeof(T), n, f) == n;
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v) {
  if (!v.empty()) fwrite(&v[0], sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
  using namespace MopedNS;
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int n_cases = 0;
  if (fread(&n_cases, 4, 1, in) != 1) return 4;
  std::vector<float> prm, xyz, fill;
  std::vector<int> iprm, off, image;
  if (!rd(in, prm, 3 * (size_t)n_cases) || !rd(in, iprm, 3 * (size_t)n_cases) || !rd(in, off, (size_t)n_cases + 1)) return 4;
  const size_t total = off[n_cases];
  if (!rd(in, xyz, 3 * total) || !rd(in, fill, total) || !rd(in, image, total)) return 4;
  fclose(in);

  std::vector<int> ncl, cl_off(1, 0), members;
  std::vector<int> poff(1, 0), iterations, active;
  std::vector<float> weight, centre;
  std::vector<SP_Model> models(1);
  for (int c = 0; c < n_cases; ++c) {
    CLUSTER_WEIGHTED_MEAN_SHIFT_CPU alg(prm[3 * c], prm[3 * c + 1], (unsigned)iprm[3 * c], (unsigned)iprm[3 * c + 1], prm[3 * c + 2]);
    alg.models = &models;
    alg._stepName = "CLUSTER";
    FrameData fd;
    fd.images.resize(iprm[3 * c + 2]);
    fd.matches.resize(1);
    for (int i = off[c]; i < off[c + 1]; ++i) {
      FrameData::Match m;
      m.imageIdx = image[i];
      m.coord2D.init(0, 0);
      m.coord3D.init(0, 0, 0);
      m.depthData.depthValid = true;
      m.depthData.coord3D.init(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
      m.depthData.depth = xyz[3 * i + 2];
      m.depthData.fillDistance = fill[i];
      fd.matches[0].push_back(m);
    }
    alg.process(fd);
    ncl.push_back((int)fd.clusters[0].size());
    for (size_t k = 0; k < fd.clusters[0].size(); ++k) {
      const FrameData::Cluster& cl = fd.clusters[0][k];
      for (FrameData::Cluster::const_iterator it = cl.begin(); it != cl.end(); ++it) members.push_back(*it);
      cl_off.push_back((int)members.size());
    }
#ifdef WMS_INSTRUMENT
    // the same lists process() builds (:195-201), one observed call per image; its clusters must be process()'s
    std::vector<FrameData::Cluster> again;
    for (int im = 0; im < iprm[3 * c + 2]; ++im) {
      std::vector<Pt<3> > pts;
      std::vector<Float> wts;
      for (size_t k = 0; k < fd.matches[0].size(); ++k) {
        const FrameData::Match& m = fd.matches[0][k];
        if (m.imageIdx != im) continue;
        pts.push_back(m.depthData.coord3D);
        wts.push_back(alg.cauchyWeight(m.depthData.fillDistance, prm[3 * c + 2]));
      }
      const int n = (int)pts.size();
      g_n = n;
      g_iterations = 0;
      g_allocs = 0;
      g_active_base = 0;
      g_active.assign(n, 0);
      g_can = 0;
      g_can_copy.clear();
      again.reserve(again.size() + n + 1);   // (no allocation of ours inside the observed call)
      g_armed = n > 0;
      alg.WeighedMeanShift<3>(again, pts, wts, alg.Radius, alg.Merge, alg.MinPts, alg.MaxIterations);
      if (g_armed) return 6;   // can's block was not seen
      poff.push_back(poff.back() + n);
      iterations.push_back(n > 0 ? g_iterations : 0);
      for (int i = 0; i < n; ++i) {
        float ctr[3];
        memcpy(ctr, &g_can_copy[(size_t)i * 24], 12);
        weight.push_back(wts[i]);
        centre.insert(centre.end(), ctr, ctr + 3);
        active.push_back(g_active[i]);
      }
    }
    if (again.size() != fd.clusters[0].size()) return 7;
    for (size_t k = 0; k < again.size(); ++k)
      if (again[k] != fd.clusters[0][k]) return 7;
#endif
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 5;
  const int n_all = (int)cl_off.size() - 1;
  fwrite(&n_cases, 4, 1, out);
  wr(out, ncl);
  fwrite(&n_all, 4, 1, out);
  wr(out, cl_off);
  wr(out, members);
#ifdef WMS_INSTRUMENT
  const int n_problems = (int)iterations.size();
  fwrite(&n_problems, 4, 1, out);
  wr(out, poff);
  wr(out, iterations);
  wr(out, weight);
  wr(out, centre);
  wr(out, active);
#endif
  fclose(out);
  return 0;
}
