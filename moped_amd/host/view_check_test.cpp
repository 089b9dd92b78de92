// view_check_test -- the host-only parts of the Kinect-view models (csrc/view_check.h) under ASan + UBSan: every refusal
// of mh_view_rows_dev / mh_db_splice_view's argument check on its own, and mh_db_append's per-model table over every
// model of small stores, against the splice written out by hand.  No GPU, no HIP runtime.  `make view_check_check`.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../csrc/view_check.h"

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static bool says(const char* why, const char* part) { return why && std::strstr(why, part); }

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  alignas(16) static float map[16];
  mh_view_spec ok_spec;
  std::memset(&ok_spec, 0, sizeof ok_spec);
  ok_spec.max_fill_distance = -1.f;
  ok_spec.merge_dist = -1.f;
  mh_view ok_view;
  std::memset(&ok_view, 0, sizeof ok_view);
  ok_view.depth_xyzn_dev = map;
  ok_view.pose[3] = 1.f;
  ok_view.K[0] = ok_view.K[1] = 800.f;

  // ---- the argument check ----
  CHECK(mh::view_call_why(&ok_view, 1, 640, 480, &ok_spec) == nullptr);
  CHECK(says(mh::view_call_why(&ok_view, 1, 640, 480, nullptr), "no mh_view_spec"));
  CHECK(says(mh::view_call_why(nullptr, 1, 640, 480, &ok_spec), "no mh_view"));
  CHECK(says(mh::view_call_why(&ok_view, 0, 640, 480, &ok_spec), "no mh_view"));
  CHECK(says(mh::view_call_why(&ok_view, MH_MAX_BATCH + 1, 640, 480, &ok_spec), "MH_MAX_BATCH"));
  CHECK(says(mh::view_call_why(&ok_view, 1, 0, 480, &ok_spec), "map size"));
  CHECK(says(mh::view_call_why(&ok_view, 1, 640, -1, &ok_spec), "map size"));
  CHECK(says(mh::view_call_why(&ok_view, 1, 65536, 65536, &ok_spec), "map size"));   // w h beyond 2^31 - 1
  for (int k = 0; k < 4; ++k) {
    mh_view_spec s = ok_spec;
    s.roi[k] = nan;
    CHECK(says(mh::view_call_why(&ok_view, 1, 640, 480, &s), "NaN in roi"));
    s.roi[k] = inf;   // an open side
    CHECK(mh::view_call_why(&ok_view, 1, 640, 480, &s) == nullptr);
  }
  for (int k = 0; k < 6; ++k)
    for (int j = 0; j < 3; ++j) {
      mh_view_spec s = ok_spec;
      s.box[k] = j == 0 ? nan : j == 1 ? inf : -inf;
      CHECK(says(mh::view_call_why(&ok_view, 1, 640, 480, &s), "non-finite box"));
    }
  {
    mh_view_spec s = ok_spec;
    s.max_rows = -1;
    CHECK(says(mh::view_call_why(&ok_view, 1, 640, 480, &s), "max_rows < 0"));
    s = ok_spec;
    s.max_fill_distance = nan;
    CHECK(says(mh::view_call_why(&ok_view, 1, 640, 480, &s), "NaN in max_fill_distance"));
    s = ok_spec;
    s.merge_ratio = nan;
    CHECK(says(mh::view_call_why(&ok_view, 1, 640, 480, &s), "merge_ratio"));
    s = ok_spec;
    s.merge_dist = nan;
    CHECK(says(mh::view_call_why(&ok_view, 1, 640, 480, &s), "merge_dist"));
    s = ok_spec;
    s.max_fill_distance = inf;   // "no pixel is too far": allowed
    s.merge_dist = inf;
    CHECK(mh::view_call_why(&ok_view, 1, 640, 480, &s) == nullptr);
  }
  // every view of a batch is looked at, and none behind the count
  std::vector<mh_view> views(MH_MAX_BATCH, ok_view);
  CHECK(mh::view_call_why(&views[0], MH_MAX_BATCH, 640, 480, &ok_spec) == nullptr);
  for (int i = 0; i < MH_MAX_BATCH; ++i) {
    std::vector<mh_view> v(views.begin(), views.begin() + i + 1);   // exactly i + 1 views: a read behind them is ASan's
    v[i].depth_xyzn_dev = nullptr;
    CHECK(says(mh::view_call_why(&v[0], i + 1, 640, 480, &ok_spec), "null depth map"));
    CHECK(i == 0 || mh::view_call_why(&v[0], i, 640, 480, &ok_spec) == nullptr);
    v[i].depth_xyzn_dev = (const char*)map + 4;
    CHECK(says(mh::view_call_why(&v[0], i + 1, 640, 480, &ok_spec), "16-byte aligned"));
    v[i].depth_xyzn_dev = map;
    v[i].fill_distance_dev = (const float*)((const char*)map + 2);
    CHECK(says(mh::view_call_why(&v[0], i + 1, 640, 480, &ok_spec), "4-byte aligned"));
    v[i].fill_distance_dev = map;
    for (int k = 0; k < 7; ++k) {
      const float keep = v[i].pose[k];
      v[i].pose[k] = k & 1 ? nan : inf;
      CHECK(says(mh::view_call_why(&v[0], i + 1, 640, 480, &ok_spec), "non-finite pose"));
      v[i].pose[k] = keep;
    }
    CHECK(mh::view_call_why(&v[0], i + 1, 640, 480, &ok_spec) == nullptr);
    // the gray image's K, read only while undistortion is on
    CHECK(mh::view_undistort_why(&v[0], i + 1) == nullptr);
    v[i].K[1] = 0.f;
    CHECK(says(mh::view_undistort_why(&v[0], i + 1), "fx or fy is 0"));
    v[i].K[1] = nan;
    CHECK(says(mh::view_undistort_why(&v[0], i + 1), "not finite"));
    v[i].K[1] = 800.f;
    v[i].K[3] = 1.f;
    CHECK(i == 0 ? mh::view_undistort_why(&v[0], 1) == nullptr : says(mh::view_undistort_why(&v[0], i + 1), "differ"));
  }
  {
    int32_t idx[1] = {0};
    float f[3] = {0, 0, 0};
    mh_view_dup d = {idx, f, f, idx, f, 10, 0, 2, 7};
    CHECK(mh::view_dup_why(nullptr) == nullptr && mh::view_dup_why(&d) == nullptr);
    mh_view_dup b = d;
    b.xyz_dev = nullptr;
    CHECK(says(mh::view_dup_why(&b), "null array"));
    b = d;
    b.row_end = 11;
    CHECK(says(mh::view_dup_why(&b), "rows outside"));
    b = d;
    b.row_begin = 8;
    CHECK(says(mh::view_dup_why(&b), "rows outside"));
    b = d;
    b.row_begin = -1;
    CHECK(says(mh::view_dup_why(&b), "rows outside"));
    b = d;
    b.n_db_rows = -1;
    CHECK(says(mh::view_dup_why(&b), "rows outside"));
    b = d;
    b.row_begin = b.row_end = b.n_db_rows = 0;   // an empty store
    CHECK(mh::view_dup_why(&b) == nullptr);
  }

  // ---- mh_view_merge_dev's own arrays, mh_db_merge_view's host counts ----
  {
    alignas(16) static float d[8];
    int32_t idx[1] = {0};
    float f[3] = {0, 0, 0};
    const mh_view_dup dup = {idx, f, f, idx, f, 10, 0, 2, 7};
    CHECK(mh::view_merge_why(d, d, d, idx, 4, &dup, d, nullptr, idx, d, f, 0, idx, idx) == nullptr);
    CHECK(mh::view_merge_why(d, d, d, idx, 4, &dup, d, idx, idx, d, f, 3, idx, idx) == nullptr);
    CHECK(says(mh::view_merge_why(nullptr, d, d, idx, 4, &dup, d, nullptr, idx, d, f, 0, idx, idx), "null list"));
    CHECK(says(mh::view_merge_why(d, nullptr, d, idx, 4, &dup, d, nullptr, idx, d, f, 0, idx, idx), "null list"));
    CHECK(says(mh::view_merge_why(d, d, nullptr, idx, 4, &dup, d, nullptr, idx, d, f, 0, idx, idx), "null list"));
    CHECK(says(mh::view_merge_why(d, d, d, nullptr, 4, &dup, d, nullptr, idx, d, f, 0, idx, idx), "null list"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 0, &dup, d, nullptr, idx, d, f, 0, idx, idx), "cap <= 0"));
    CHECK(says(mh::view_merge_why(d + 1, d, d, idx, 4, &dup, d, nullptr, idx, d, f, 0, idx, idx), "16-byte aligned"));
    CHECK(says(mh::view_merge_why(d, d + 2, d, idx, 4, &dup, d, nullptr, idx, d, f, 0, idx, idx), "16-byte aligned"));
    CHECK(says(mh::view_merge_why(d, d, d + 1, idx, 4, &dup, d, nullptr, idx, d, f, 0, idx, idx), "xy 8-byte"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, nullptr, d, nullptr, idx, d, f, 0, idx, idx), "no mh_view_dup"));
    mh_view_dup bad = dup;
    bad.row_end = 11;
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, &bad, d, nullptr, idx, d, f, 0, idx, idx), "rows outside"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, &dup, nullptr, nullptr, idx, d, f, 0, idx, idx), "store's descriptors"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, &dup, d + 1, nullptr, idx, d, f, 0, idx, idx), "store's descriptors"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, &dup, d, nullptr, nullptr, d, f, 0, idx, idx), "null output"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, &dup, d, nullptr, idx, nullptr, f, 0, idx, idx), "null output"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, &dup, d, nullptr, idx, d, nullptr, 0, idx, idx), "null output"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, &dup, d, nullptr, idx, d, f, 0, nullptr, idx), "null output"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, &dup, d, nullptr, idx, d, f, 0, idx, nullptr), "null output"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, &dup, d, nullptr, idx, d + 1, f, 0, idx, idx), "merged descriptors"));
    CHECK(says(mh::view_merge_why(d, d, d, idx, 4, &dup, d, nullptr, idx, d, f, -1, idx, idx), "merged_cap < 0"));
    // the counts: exactly n_rows of them are read (a read behind them is ASan's)
    for (int n = 0; n <= 5; ++n) {
      std::vector<int32_t> v(n, 1);
      CHECK(mh::view_counts_why(n ? &v[0] : nullptr, n, n) == nullptr);
      CHECK(mh::view_counts_why(nullptr, 0, n) == nullptr);
      CHECK(n == 0 || says(mh::view_counts_why(nullptr, n, n), "without an array"));
      if (n == 0) continue;
      CHECK(says(mh::view_counts_why(&v[0], n, n + 1), "row count"));
      CHECK(says(mh::view_counts_why(&v[0], n, n - 1), "row count"));
      for (int k = 0; k < n; ++k) {
        v[k] = k & 1 ? 0 : -3;
        CHECK(says(mh::view_counts_why(&v[0], n, n), "count < 1"));
        v[k] = 0x7FFFFFFF;
        CHECK(says(mh::view_counts_why(&v[0], n, n), "cannot grow"));
        v[k] = 0x7FFFFFFE;
        CHECK(mh::view_counts_why(&v[0], n, n) == nullptr);
      }
    }
  }

  // ---- mh_db_append's table: against model_of spliced by hand ----
  const int sizes[][5] = {{3, 0, 5, 0, 2}, {1, 1, 1, 1, 1}, {0, 0, 0, 0, 0}, {7, 0, 0, 0, 0}, {0, 0, 0, 0, 9}};
  for (size_t c = 0; c < sizeof sizes / sizeof sizes[0]; ++c)
    for (int models = 1; models <= 5; ++models)
      for (int model = 0; model < models; ++model)
        for (int n_rows = 0; n_rows <= 4; n_rows += 2) {
          std::vector<int32_t> begin(1, 0), model_of;
          for (int m = 0; m < models; ++m) {
            begin.push_back(begin.back() + sizes[c][m]);
            model_of.insert(model_of.end(), sizes[c][m], m);
          }
          const std::vector<int32_t> table = mh::append_table(begin, model, n_rows);
          // by hand: old[0, e) ++ n_rows rows of `model` ++ old[e, N)
          std::vector<int32_t> want_of(model_of.begin(), model_of.begin() + begin[model + 1]);
          want_of.insert(want_of.end(), n_rows, model);
          want_of.insert(want_of.end(), model_of.begin() + begin[model + 1], model_of.end());
          CHECK(table.size() == begin.size() && table[0] == 0 && table.back() == (int32_t)want_of.size());
          for (int m = 0; m < models && table.size() == begin.size(); ++m) {
            CHECK(table[m] <= table[m + 1]);
            for (int r = table[m]; r < table[m + 1]; ++r) CHECK(want_of[r] == m);
            CHECK(table[m + 1] - table[m] == sizes[c][m] + (m == model ? n_rows : 0));
          }
        }
  if (failures) {
    std::fprintf(stderr, "view_check_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("view_check_test: ok\n");
  return 0;
}
