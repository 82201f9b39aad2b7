// The cell-grid searches of knn.hip that other translation units call: ball_query.hip and interpolate.hip take the
// grid route through these when grid_search_pays() and the caller's workspace is large enough.
#pragma once
#include <cstddef>
#include <hip/hip_runtime.h>

namespace amc {

// b clouds of n support points and m queries each: the grid beats the all-pairs scan
bool grid_search_pays(int b, int n, int m);
size_t grid_search_workspace_bytes(int b, int n, int m);

// xyz (b,n,3) support, new_xyz (b,m,3) queries
int ball_query_grid(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int *idx,
                    void *workspace, hipStream_t stream);
// unknown (b,n,3) queries, known (b,m,3) support
int three_nn_grid(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx, void *workspace,
                  hipStream_t stream);

}  // namespace amc
