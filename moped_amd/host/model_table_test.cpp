// HipModelTable over HipResidentModels, and HipPinnedBlock (hip_session.hpp) on the CPU, under ASan + UBSan
// (`make model_table_check`): the C-ABI calls they make are defined HERE -- nothing of the library or of ROCm is
// linked -- so that every call is recorded with its arguments, a failure can be injected, and a leak or a double free
// of the page-locked block is a sanitizer report.  Models of 2, 0 and 3 rows, as Update() of a MATCH step sees them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "moped_types.hpp"
#include "hip_session.hpp"

struct mh_ctx {
  int device;
};

namespace {

struct Call {
  char kind;   // N mh_normalize, U mh_db_upload, S mh_db_splice
  int op, index, n, n_models;
};
std::vector<Call> g_calls;
std::vector<int32_t> g_owner;   // of the last upload
std::vector<float> g_xyz, g_desc;
int g_fail_normalize = 0, g_fail_upload = 0, g_fail_splice = 0, g_fail_alloc = 0;   // that many calls fail from here on
long g_allocs = 0, g_frees = 0;
size_t g_last_bytes = 0;
const mh_ctx* g_free_ctx = 0;

bool fails(int& budget) {
  if (budget <= 0) return false;
  --budget;
  return true;
}

// the stand-in's transform: a row scaled to unit L2 length, in float
void unit(float* row) {
  float s = 0.f;
  for (int i = 0; i < MH_DESC_DIM; ++i) s += row[i] * row[i];
  s = std::sqrt(s);
  for (int i = 0; i < MH_DESC_DIM; ++i) row[i] /= s;
}

int g_failed = 0;
void check_at(bool ok, const char* what, int line) {
  if (ok) return;
  std::fprintf(stderr, "model_table_test:%d: %s\n", line, what);
  ++g_failed;
}
#define CHECK(cond) check_at((cond), #cond, __LINE__)

}  // namespace

extern "C" {
int mh_create(int device, mh_ctx** out) {
  *out = new mh_ctx;
  (*out)->device = device;
  return MH_OK;
}
void mh_destroy(mh_ctx* ctx) { delete ctx; }
const char* mh_last_error(const mh_ctx*) { return "injected"; }
int mh_normalize(mh_ctx*, float* desc, int n) {
  const Call c = {'N', -1, -1, n, -1};
  g_calls.push_back(c);
  if (fails(g_fail_normalize)) return MH_ERR_HIP;
  for (int r = 0; r < n; ++r) unit(desc + (size_t)r * MH_DESC_DIM);
  return MH_OK;
}
int mh_db_upload(mh_ctx*, const float* desc, const int32_t* owner, const float* xyz, int N, int n_models, int32_t index_base) {
  const Call c = {'U', -1, (int)index_base, N, n_models};
  g_calls.push_back(c);
  if (fails(g_fail_upload)) return MH_ERR_HIP;
  g_desc.assign(desc, desc + (size_t)N * MH_DESC_DIM);
  g_owner.assign(owner, owner + N);
  g_xyz.assign(xyz, xyz + (size_t)N * 3);
  return MH_OK;
}
int mh_db_splice(mh_ctx*, int op, int model, const float*, const float*, int n_rows, int, int) {
  const Call c = {'S', op, model, n_rows, -1};
  g_calls.push_back(c);
  return fails(g_fail_splice) ? MH_ERR_HIP : MH_OK;
}
int mh_host_alloc(mh_ctx*, size_t bytes, void** out) {
  if (fails(g_fail_alloc)) return MH_ERR_HIP;
  *out = std::malloc(bytes ? bytes : 1);
  g_last_bytes = bytes;
  ++g_allocs;
  return MH_OK;
}
int mh_host_free(mh_ctx* ctx, void* p) {
  g_free_ctx = ctx;
  if (p) ++g_frees;
  std::free(p);
  return MH_OK;
}
}

using namespace MopedNS;

namespace {

const std::string SIFT = "SIFT";

// a model of `rows` keypoints whose descriptors and coordinates are told apart by `tag`
SP_Model makeModel(int tag, int rows) {
  SP_Model m(new Model);
  m->name = "model" + toString(tag);
  std::vector<Model::IP>& ips = m->IPs[SIFT];
  ips.resize(rows);
  for (int f = 0; f < rows; ++f) {
    ips[f].coord3D.init(tag + 0.f, f + 0.f, tag * 10.f + f);
    ips[f].descriptor.resize(MH_DESC_DIM);
    for (int i = 0; i < MH_DESC_DIM; ++i) ips[f].descriptor[i] = (float)(1 + (i * 7 + f * 3 + tag) % 11);
  }
  return m;
}

std::vector<SP_Model> threeModels() {
  std::vector<SP_Model> models;
  models.push_back(makeModel(0, 2));
  models.push_back(makeModel(1, 0));
  models.push_back(makeModel(2, 3));
  return models;
}

// every descriptor of every model, in row order
std::vector<float> rowsOf(std::vector<SP_Model>& models) {
  std::vector<float> all;
  for (size_t m = 0; m < models.size(); ++m) {
    std::vector<Model::IP>& ips = models[m]->IPs[SIFT];
    for (size_t f = 0; f < ips.size(); ++f) all.insert(all.end(), ips[f].descriptor.begin(), ips[f].descriptor.end());
  }
  return all;
}

// correspModel / correspFeat say what the models say
bool tablesAgree(const HipModelTable& t, std::vector<SP_Model>& models) {
  size_t x = 0;
  for (size_t m = 0; m < models.size(); ++m) {
    std::vector<Model::IP>& ips = models[m]->IPs[SIFT];
    for (size_t f = 0; f < ips.size(); ++f, ++x)
      if (x >= t.correspModel.size() || t.correspModel[x] != (int)m || t.correspFeat[x] != &ips[f].coord3D) return false;
  }
  return x == t.correspModel.size() && x == t.correspFeat.size();
}

void forget() {   // the process-wide record of what is resident, as a fresh process has it
  HipResidentModels& r = HipResidentModels::get();
  r.ptr.clear();
  r.count.clear();
  r.type.clear();
  r.valid = false;
  r.fullUploads = r.splices = 0;
  g_calls.clear();
}

size_t count(char kind) {
  size_t n = 0;
  for (size_t i = 0; i < g_calls.size(); ++i) n += g_calls[i].kind == kind;
  return n;
}
const Call* only(char kind) {   // the one call of that kind, or NULL
  const Call* c = 0;
  for (size_t i = 0; i < g_calls.size(); ++i)
    if (g_calls[i].kind == kind) {
      if (c) return 0;
      c = &g_calls[i];
    }
  return c;
}

// a recorded full upload of the three models to start the edits from
void recorded(HipModelTable& t, std::vector<SP_Model>& models, mh_ctx* ctx) {
  forget();
  CHECK(t.update(ctx, models, SIFT, 1) && HipResidentModels::get().valid && HipResidentModels::get().fullUploads == 1);
  g_calls.clear();
}

}  // namespace

int main() {
  mh_ctx* ctx = HipSession::get();
  CHECK(ctx != 0);

  for (int incremental = 0; incremental < 2; ++incremental) {   // the full path, with and without the record for edits
    forget();
    std::vector<SP_Model> models = threeModels();
    std::vector<float> want = rowsOf(models);
    for (size_t r = 0; r < want.size() / MH_DESC_DIM; ++r) unit(&want[r * MH_DESC_DIM]);
    HipModelTable t;
    CHECK(t.skipCalculation);
    CHECK(t.update(ctx, models, SIFT, incremental));
    CHECK(g_calls.size() == 2 && g_calls[0].kind == 'N' && g_calls[0].n == 5);
    CHECK(g_calls.size() == 2 && g_calls[1].kind == 'U' && g_calls[1].n == 5 && g_calls[1].n_models == 3 && g_calls[1].index == 0);
    const int32_t owners[5] = {0, 0, 2, 2, 2};
    CHECK(g_owner == std::vector<int32_t>(owners, owners + 5));
    const float xyz[15] = {0, 0, 0, 0, 1, 1, 2, 0, 20, 2, 1, 21, 2, 2, 22};
    CHECK(g_xyz == std::vector<float>(xyz, xyz + 15));
    CHECK(rowsOf(models) == want && g_desc == want);   // written back into the models, and what went up
    CHECK(tablesAgree(t, models) && t.correspModel.size() == 5);
    CHECK(!t.skipCalculation);
    CHECK(HipResidentModels::get().valid == (incremental != 0) && HipResidentModels::get().fullUploads == (unsigned long)incremental);
  }

  for (int rows = 0; rows < 2; ++rows) {   // too few rows: no device call
    forget();
    std::vector<SP_Model> models;
    models.push_back(makeModel(0, 0));
    models.push_back(makeModel(1, rows));
    const std::vector<float> before = rowsOf(models);
    HipModelTable t;
    t.skipCalculation = false;
    CHECK(t.update(ctx, models, SIFT, rows) && t.skipCalculation && g_calls.empty());
    CHECK(rowsOf(models) == before && tablesAgree(t, models));
  }

  {   // a failing mh_normalize: reported, the models untouched; a failing mh_db_upload; then the next frame's retry
    forget();
    std::vector<SP_Model> models = threeModels();
    const std::vector<float> before = rowsOf(models);
    HipModelTable t;
    g_fail_normalize = 1;
    CHECK(!t.update(ctx, models, SIFT, 1) && t.skipCalculation);
    CHECK(g_calls.size() == 1 && count('N') == 1 && rowsOf(models) == before && !HipResidentModels::get().valid);
    g_calls.clear();
    g_fail_upload = 1;
    CHECK(!t.update(ctx, models, SIFT, 1) && t.skipCalculation);
    CHECK(g_calls.size() == 2 && count('U') == 1 && !HipResidentModels::get().valid && HipResidentModels::get().fullUploads == 0);
    g_calls.clear();
    CHECK(t.update(ctx, models, SIFT, 1) && !t.skipCalculation && count('U') == 1 && HipResidentModels::get().valid);
  }

  {   // an appended model: one INSERT at the new index, its rows normalised, no upload
    std::vector<SP_Model> models = threeModels();
    HipModelTable t;
    recorded(t, models, ctx);
    models.push_back(makeModel(3, 2));
    std::vector<float> want = rowsOf(models);
    for (size_t r = 5; r < 7; ++r) unit(&want[r * MH_DESC_DIM]);   // (the first five are normalised already)
    CHECK(t.update(ctx, models, SIFT, 1) && !t.skipCalculation);
    const Call* s = only('S');
    CHECK(count('U') == 0 && s && s->op == MH_DB_INSERT && s->index == 3 && s->n == 2 && g_calls.size() == 2);
    CHECK(only('N') && only('N')->n == 2 && rowsOf(models) == want);
    CHECK(tablesAgree(t, models) && t.correspModel.size() == 7);
    CHECK(HipResidentModels::get().valid && HipResidentModels::get().splices == 1 && HipResidentModels::get().fullUploads == 1);
  }

  {   // the middle model removed: one REMOVE at index 1, nothing else
    std::vector<SP_Model> models = threeModels();
    HipModelTable t;
    recorded(t, models, ctx);
    models.erase(models.begin() + 1);
    CHECK(t.update(ctx, models, SIFT, 1) && !t.skipCalculation);
    CHECK(g_calls.size() == 1 && g_calls[0].kind == 'S' && g_calls[0].op == MH_DB_REMOVE && g_calls[0].index == 1);
    CHECK(tablesAgree(t, models) && t.correspModel.size() == 5 && t.correspModel[2] == 1);
    CHECK(HipResidentModels::get().valid && HipResidentModels::get().ptr.size() == 2);
  }

  {   // a model replaced in place: one REPLACE at its index
    std::vector<SP_Model> models = threeModels();
    HipModelTable t;
    recorded(t, models, ctx);
    models[2] = makeModel(7, 4);
    CHECK(t.update(ctx, models, SIFT, 1) && !t.skipCalculation);
    const Call* s = only('S');
    CHECK(count('U') == 0 && s && s->op == MH_DB_REPLACE && s->index == 2 && s->n == 4);
    CHECK(tablesAgree(t, models) && t.correspModel.size() == 6);
    CHECK(HipResidentModels::get().valid && HipResidentModels::get().count[2] == 4);
  }

  {   // two removals at once are not served: the full path
    std::vector<SP_Model> models = threeModels();
    models.push_back(makeModel(3, 2));
    HipModelTable t;
    recorded(t, models, ctx);
    models.erase(models.begin(), models.begin() + 2);
    CHECK(t.update(ctx, models, SIFT, 1) && !t.skipCalculation);
    CHECK(count('S') == 0 && only('N') && only('N')->n == 5 && only('U') && only('U')->n == 5 && only('U')->n_models == 2);
    CHECK(HipResidentModels::get().fullUploads == 2 && HipResidentModels::get().valid && HipResidentModels::get().ptr.size() == 2);
    CHECK(tablesAgree(t, models));
  }

  {   // a failing mh_db_splice: the full path takes over and the record is valid again
    std::vector<SP_Model> models = threeModels();
    HipModelTable t;
    recorded(t, models, ctx);
    models.push_back(makeModel(3, 2));
    g_fail_splice = 1;
    CHECK(t.update(ctx, models, SIFT, 1) && !t.skipCalculation);
    CHECK(count('S') == 1 && only('U') && only('U')->n == 7 && only('U')->n_models == 4);
    CHECK(HipResidentModels::get().valid && HipResidentModels::get().fullUploads == 2 && HipResidentModels::get().splices == 0);
    CHECK(HipResidentModels::get().ptr.size() == 4 && tablesAgree(t, models));
  }

  {   // the page-locked block: nothing within the capacity, need + need / 4 on growth, the old block freed once
    mh_ctx other = {1};
    {
      HipPinnedBlock b;
      CHECK(b.data() == 0 && b.bytes() == 0);
      CHECK(b.ensure(ctx, 1000) && g_allocs == 1 && g_frees == 0 && g_last_bytes == 1250 && b.bytes() == 1250 && b.data());
      void* const first = b.data();
      static_cast<char*>(first)[1249] = 1;   // (the whole block is ours)
      CHECK(b.ensure(ctx, 1000) && b.ensure(&other, 1250) && b.ensure(ctx, 1) && g_allocs == 1 && g_frees == 0 && b.data() == first);
      CHECK(b.ensure(ctx, 1251) && g_allocs == 2 && g_frees == 1 && g_last_bytes == 1251 + 1251 / 4 && b.bytes() == g_last_bytes);
      g_fail_alloc = 1;   // a failed allocation: the old block is gone, nothing is held; the next call succeeds
      CHECK(!b.ensure(ctx, 4000) && g_allocs == 2 && g_frees == 2 && b.data() == 0 && b.bytes() == 0);
      CHECK(b.ensure(&other, 16) && g_allocs == 3 && b.bytes() == 20);
      g_free_ctx = 0;
    }
    CHECK(g_allocs == 3 && g_frees == 3 && g_free_ctx == &other);   // freed with the context it was allocated with
    {
      HipPinnedBlock never;   // (never grown: no call)
    }
    CHECK(g_allocs == 3 && g_frees == 3);
  }

  if (g_failed) return 1;
  std::printf("model_table_test: no finding\n");
  return 0;
}
