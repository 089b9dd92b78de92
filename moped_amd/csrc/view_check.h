// Host-only parts of the Kinect-view models (view_rows.hip, db_edit.hip): what the entry points refuse before anything is
// launched, and the per-model table of an append.  No HIP in here, so that a plain C++ program can run them under the
// sanitizers (host/view_check_test.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/moped_hip.h"

namespace mh {

inline bool view_finite_n(const float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}
inline bool view_all_zero(const float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (v[i] != 0.f) return false;
  return true;
}

// why a spec, the views or the map size are refused (nullptr: they are not)
inline const char* view_call_why(const mh_view* views, int n_views, int width, int height, const mh_view_spec* spec) {
  if (!spec) return "no mh_view_spec";
  if (!views || n_views <= 0 || n_views > MH_MAX_BATCH) return "no mh_view, or more than MH_MAX_BATCH of them";
  if (width <= 0 || height <= 0 || (long long)width * height > 0x7FFFFFFFll) return "bad map size";
  if (std::isnan(spec->roi[0]) || std::isnan(spec->roi[1]) || std::isnan(spec->roi[2]) || std::isnan(spec->roi[3]))
    return "NaN in roi";
  if (!view_finite_n(spec->box, 6)) return "non-finite box";
  if (spec->max_rows < 0) return "max_rows < 0";
  if (std::isnan(spec->max_fill_distance) || std::isnan(spec->merge_ratio) || std::isnan(spec->merge_dist))
    return "NaN in max_fill_distance, merge_ratio or merge_dist";
  for (int i = 0; i < n_views; ++i) {
    if (!views[i].depth_xyzn_dev) return "a null depth map";
    if ((uintptr_t)views[i].depth_xyzn_dev & 15) return "a depth map that is not 16-byte aligned";
    if ((uintptr_t)views[i].fill_distance_dev & 3) return "a distance map that is not 4-byte aligned";
    if (!view_finite_n(views[i].pose, 7)) return "non-finite pose";
  }
  return nullptr;
}

// why the gray images' K is refused while undistortion is on
inline const char* view_undistort_why(const mh_view* views, int n_views) {
  for (int i = 0; i < n_views; ++i) {
    const float* K = views[i].K;
    if (!view_finite_n(K, 4) || K[0] == 0.f || K[1] == 0.f) return "undistortion is on and the view's K is not finite, or fx or fy is 0";
    for (int k = 0; k < 4; ++k)
      if (K[k] != views[0].K[k]) return "undistortion is on and the views' K differ";
  }
  return nullptr;
}

inline const char* view_dup_why(const mh_view_dup* dup) {
  if (!dup) return nullptr;
  if (!dup->idx_dev || !dup->d1_dev || !dup->d2_dev || !dup->model_of_dev || !dup->xyz_dev) return "bad mh_view_dup (a null array)";
  if (dup->n_db_rows < 0 || dup->row_begin < 0 || dup->row_end < dup->row_begin || dup->row_end > dup->n_db_rows)
    return "bad mh_view_dup (rows outside [0, n_db_rows])";
  return nullptr;
}

// mh_db_append: the per-model row ranges after n_rows rows went behind the last row of `model` (0 <= model < models);
// begin = the ranges before, [models + 1]
inline std::vector<int32_t> append_table(const std::vector<int32_t>& begin, int model, int n_rows) {
  std::vector<int32_t> table(begin.begin(), begin.begin() + model + 1);   // models up to `model` begin where they began
  for (size_t m = (size_t)model + 1; m < begin.size(); ++m) table.push_back(begin[m] + n_rows);
  return table;
}

}  // namespace mh
