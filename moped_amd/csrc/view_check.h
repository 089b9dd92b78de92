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

// why mh_view_merge_dev refuses its own arrays (the view, the spec and the map size are view_call_why's); dup is required
inline const char* view_merge_why(const float* desc_dev, const float* qn_desc_dev, const float* xy_dev, const int32_t* n_dev, int cap,
                                  const mh_view_dup* dup, const float* old_desc_dev, const int32_t* views_in_dev,
                                  const int32_t* merged_idx_dev, const float* merged_desc_dev, const float* merged_xyz_dev,
                                  int merged_cap, const int32_t* n_merged_dev, const int32_t* views_out_dev) {
  if (!desc_dev || !qn_desc_dev || !xy_dev || !n_dev || cap <= 0) return "bad argument (a null list, or cap <= 0)";
  if (((uintptr_t)desc_dev & 15) || ((uintptr_t)qn_desc_dev & 15) || ((uintptr_t)xy_dev & 7))
    return "bad argument (descriptor arrays are 16-byte aligned, xy 8-byte)";
  if (!dup) return "no mh_view_dup (the merge needs MATCH's answer and the model's rows)";
  if (const char* why = view_dup_why(dup)) return why;
  if (!old_desc_dev || ((uintptr_t)old_desc_dev & 15)) return "the store's descriptors are null or not 16-byte aligned";
  if ((uintptr_t)views_in_dev & 3) return "a count array that is not 4-byte aligned";
  if (!merged_idx_dev || !merged_desc_dev || !merged_xyz_dev || !n_merged_dev || !views_out_dev) return "a null output";
  if ((uintptr_t)merged_desc_dev & 15) return "merged descriptors that are not 16-byte aligned";
  if (merged_cap < 0) return "merged_cap < 0";
  return nullptr;
}

// why a host-side array of view counts is refused for a model of n_rows rows (nullptr array: every count is 1)
inline const char* view_counts_why(const int32_t* views, int n_views, int n_rows) {
  if (!views) return n_views == 0 ? nullptr : "n_views_in != 0 without an array";
  if (n_views != n_rows) return "n_views_in is not the model's row count";
  for (int i = 0; i < n_views; ++i)
    if (views[i] < 1 || views[i] == 0x7FFFFFFF) return "a view count < 1 (or one that cannot grow by one)";
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
