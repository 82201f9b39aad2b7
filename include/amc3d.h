/*
 * amc3d.h -- C-ABI of libamc3d_hip.so, the MI355X (gfx950) implementation of the
 * native point operators on AMContrast3D's training hot path.
 *
 * Drop-in boundary.  The reference binds its native layer through two pybind11
 * modules whose entry points take torch tensors and forward raw data pointers:
 *     pointnet2_batch_cuda  openpoints/cpp/pointnet2_batch/src/pointnet2_api.cpp:10-24
 *     pointops_cuda         openpoints/cpp/pointops/src/pointops_api.cpp:13-25
 * Each function below replaces the launcher behind one of those entry points
 * and keeps its argument order; tensors become plain device pointers and every
 * call gains a trailing `stream` (a hipStream_t passed as void*; NULL = the
 * null stream).  No torch type appears in any signature.  INTEGRATION.md shows
 * the ctypes stub that rebinds the reference's Python wrappers onto this ABI.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in `_host`;
 *   - float = IEEE fp32, indices = int32, layouts exactly as in the reference
 *     (dense row-major, batch first);
 *   - return value: 0 on success, otherwise the hipError_t of the failed
 *     launch/argument check (the reference prints and exit(-1)s instead:
 *     ball_query_gpu.cu:68-71); nothing is thrown, nothing is allocated, and
 *     no call synchronises the device -- they are graph-capturable;
 *   - functions that need scratch memory take a caller-owned `workspace`
 *     whose size is reported by the matching *_workspace_bytes() query.
 *   - distances are evaluated exactly as the reference writes them, in fp32,
 *     left to right and without FMA contraction: ((dx*dx + dy*dy) + dz*dz).
 */
#ifndef AMC3D_H
#define AMC3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* library identification: "amc3d-hip gfx950 <abi-version>" */
const char *amc3d_version(void);
/* text of the last error on this thread ("" if none) */
const char *amc3d_last_error(void);

/* A HIP stream (hipStream_t) with a hardware queue of its own, for the long latency-bound furthest-point-sampling
 * launches of a pipelined training loop: ordinary streams share four hardware queues per process, and whatever
 * shares the queue of a running FPS kernel waits milliseconds for it.  (The reference launches everything on the
 * legacy default stream; this is the hook its trainer would use to overlap batches.) */
int amc3d_stream_create_dedicated(void **stream);
/* the same with a CU mask that enables bits [first_cu, first_cu + n_cus) only (n_cus <= 0: every CU) */
int amc3d_stream_create_masked(void **stream, int first_cu, int n_cus);
/* Raise the device's scratch (private segment) high-water mark to bytes_per_lane (256 / 1024 / 4096 / 16384) with one launch, BEFORE
 * graphs are captured: the runtime re-allocates scratch when a kernel asks for more than any before it, and graph nodes
 * instantiated earlier keep the old allocation (a replay then faults).  scratch_out: any device int (not written). */
int amc3d_reserve_scratch(int bytes_per_lane, int *scratch_out, void *stream);
int amc3d_stream_destroy(void *stream);

/* ---- pointnet2_batch surface ------------------------------------------------ */

/* replaces ball_query_wrapper_fast -> ball_query_kernel_launcher_fast
 * (pointnet2_batch/src/ball_query.cpp:29-39, ball_query_gpu.cu:54-73).
 * new_xyz (b,m,3), xyz (b,n,3) -> idx (b,m,nsample): the first `nsample`
 * support indices (ascending) with d2 < radius*radius, padded with the first
 * hit; a row with no hit is written as zeros (the reference relies on the
 * caller's zero-fill, group.py:194).
 * With a workspace of amc3d_grid_search_workspace_bytes(b, n, m) the search runs on a uniform grid of cell
 * edge >= radius (27 cells per query instead of all n points); NULL / too small = the all-pairs scan.
 * Both give the reference's result exactly. */
size_t amc3d_grid_search_workspace_bytes(int b, int n_support, int m_queries);
/* 1: with that workspace (and, for the ball query, nsample <= 64 and radius > 0) this problem size is searched on the
 * grid; 0: the all-pairs scan answers.  For amc3d_three_nn the support is `known`: (b, m, n). */
int amc3d_grid_search_pays(int b, int n_support, int m_queries);
int amc3d_ball_query(int b, int n, int m, float radius, int nsample,
                     const float *new_xyz, const float *xyz, int *idx,
                     void *workspace, size_t workspace_bytes, void *stream);

/* replaces group_points_wrapper_fast (group_points.cpp, group_points_gpu.cu:53-92):
 * points (b,c,n), idx (b,npoints,nsample) -> out (b,c,npoints,nsample) */
int amc3d_group_points(int b, int c, int n, int npoints, int nsample,
                       const float *points, const int *idx, float *out, void *stream);

/* replaces group_points_grad_wrapper_fast (group_points_gpu.cu:14-50):
 * grad_points (b,c,n) += scatter(grad_out (b,c,npoints,nsample)); the caller
 * zero-initialises grad_points (group.py:111).  With a workspace of
 * b*c*n floats (one (b,n,c) fp32 image) the adds go through a point-major image (full-rate atomic
 * shape) and are transposed back; workspace = NULL selects the reference's direct per-element
 * atomics. */
int amc3d_group_points_grad(int b, int c, int n, int npoints, int nsample,
                            const float *grad_out, const int *idx, float *grad_points,
                            void *workspace, size_t workspace_bytes, void *stream);

/* replaces gather_points_wrapper_fast / gather_points_grad_wrapper_fast
 * (sampling_gpu.cu:15-90): points (b,c,n), idx (b,npoints) -> out (b,c,npoints) */
int amc3d_gather_points(int b, int c, int n, int npoints,
                        const float *points, const int *idx, float *out, void *stream);
int amc3d_gather_points_grad(int b, int c, int n, int npoints,
                             const float *grad_out, const int *idx, float *grad_points, void *stream);

/* replaces furthest_point_sampling_wrapper (sampling.cpp, sampling_gpu.cu:100-260):
 * dataset (b,n,3) -> idxs (b,m), idxs[:,0] = 0.  `temp` (b,n) is the reference's
 * running-min-distance buffer (the caller fills it with 1e10, subsample.py:95); it may be
 * NULL for n <= 24576: the running minima then start at 1e10 and stay on chip.  When given it
 * is read as the initial minima and receives the final ones, as in the reference.
 * `workspace`: amc3d_fps_workspace_bytes(b,n) bytes (the cloud's spatial sort order).
 * Ties resolve exactly as the reference's block-strided scan + shared-memory tree does for
 * its block size opt_n_threads(n) (cuda_utils.h:10-14). */
size_t amc3d_fps_workspace_bytes(int b, int n);
int amc3d_furthest_point_sampling(int b, int n, int m, const float *dataset,
                                  float *temp, int *idxs, void *workspace, size_t workspace_bytes,
                                  void *stream);

/* replaces three_nn_wrapper_fast (interpolate_gpu.cu:16-81):
 * unknown (b,n,3), known (b,m,3) -> dist2 (b,n,3) squared distances, idx (b,n,3) */
/* workspace: amc3d_grid_search_workspace_bytes(b, m, n) (support = known) selects the grid search; NULL = all pairs */
int amc3d_three_nn(int b, int n, int m, const float *unknown, const float *known,
                   float *dist2, int *idx, void *workspace, size_t workspace_bytes, void *stream);

/* replaces three_interpolate_wrapper_fast (interpolate_gpu.cu:84-124):
 * points (b,c,m), idx/weight (b,n,3) -> out (b,c,n) */
int amc3d_three_interpolate(int b, int c, int m, int n, const float *points,
                            const int *idx, const float *weight, float *out, void *stream);

/* out (b,c,n) = base (b,c,n) + three_interpolate(points (b,c,m), idx, weight): FeaturePropogation's first conv
 * (pointnext_AA.py:210-226) applied before the interpolation, W . [f1 ; up(f2)] = W1 . f1 + up(W2 . f2) */
int amc3d_three_interpolate_add(int b, int c, int m, int n, const float *points, const int *idx, const float *weight,
                                const float *base, float *out, void *stream);
/* replaces three_interpolate_grad_wrapper_fast (interpolate_gpu.cu:127-169):
 * grad_points (b,c,m) += ...; caller zero-initialises (upsampling.py:82).
 * Optional workspace: b*c*m floats, as above. */
int amc3d_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out,
                                 const int *idx, const float *weight, float *grad_points,
                                 void *workspace, size_t workspace_bytes, void *stream);
/* Where one channel's slab of m doubles fits the LDS budget (m <= 16384) and c >= 8, the gradient is summed in LDS by a workgroup per
 * (cloud, group of cg channels): no global atomics, and the workspace is not touched.  amc3d_three_interpolate_grad_route
 * says which way a shape goes: 0 one global atomic per term, 1 point-major global atomics (with the workspace), 2 LDS;
 * cg / threads (may be NULL) receive the LDS route's channel group and workgroup size, 0 otherwise. */
int amc3d_three_interpolate_grad_route(int b, int c, int n, int m, int *cg, int *threads);
/* Route 2 in overwrite form: writes every element of grad_points (b,c,m) -- +0.0f where no unknown point names the known
 * point -- so the caller neither zero-initialises nor passes a workspace.  An error for shapes whose route is not 2. */
int amc3d_three_interpolate_grad_write(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                       const float *weight, float *grad_points, void *stream);
/* The LDS kernel with cg and threads (256, 512, 1024) given; cg * m doubles <= 160 KiB.  accumulate != 0: grad_points +=. */
int amc3d_three_interpolate_grad_lds(int b, int c, int n, int m, int cg, int threads, int accumulate, const float *grad_out,
                                     const int *idx, const float *weight, float *grad_points, void *stream);
/* The same gradient without atomics (deterministic mode), from the reverse lists of idx seen as a query of n points with 3
 * samples into the m known points: rev_start (b*m + 1), rev_edge (b*n*3) = amc3d_group_csr(b, m, n, 3, idx, ...).
 * SUMMATION ORDER (part of the contract, shared by the three *_csr gathers of deterministic mode): every target takes its
 * incoming positions in ascending position order -- the order of its list -- and adds them by sequential fp32 __fadd_rn
 * starting from +0.0f; a term that is a product is rounded first by __fmul_rn; nothing is reassociated, the work is spread
 * over channels and targets only.  Here: grad_points[b,ch,t] = sum over p = u*3 + j in t's list of
 * __fmul_rn(grad_out[b,ch,u], weight[b,u,j]).  Every element of grad_points (b,c,m) is written: a target without incoming
 * positions gets exactly +0.0f, so the caller need not zero-initialise.  No workspace. */
int amc3d_three_interpolate_grad_csr(int b, int c, int n, int m, const float *grad_out, const int *idx, const float *weight,
                                     const int *rev_start, const int *rev_edge, float *grad_points, void *stream);

/* ---- pointops surface --------------------------------------------------------- */

/* replaces knnquery_cuda -> knnquery_cuda_launcher
 * (pointops/src/knnquery/knnquery_cuda.cpp:7-16, knnquery_cuda_kernel.cu:65-108).
 * xyz (n,3) support, new_xyz (m,3) queries, offset / new_offset: cumulative
 * segment ends (nbatch entries each; the reference does not pass nbatch, it
 * walks new_offset until it exceeds the query id -- pass it here).
 * -> idx (m,nsample), dist2 (m,nsample) squared distances, ascending.
 * nsample <= 100 (the reference's per-thread heap is float[100]).
 * Results equal the reference's max-heap + heap-sort including how equal
 * distances are ordered.
 * reuse_grid != 0: the workspace was last used by amc3d_knnquery with the SAME support set (xyz, offset, n,
 * nbatch) and at least as many queries; its cell grid is kept and only the queries run (the loss asks for
 * four neighbour sets of the full-resolution cloud per step).  Results are identical either way. */
size_t amc3d_knnquery_workspace_bytes(int n, int m, int nsample, int nbatch);
/* 1: this problem size goes through the cell grid (so a later call may pass reuse_grid, and this call may reuse an
 * earlier grid); 0: the all-pairs heap kernel answers and the workspace is left untouched */
int amc3d_knnquery_uses_grid(int m, int nsample, int n, int nbatch);
int amc3d_knnquery(int m, int nsample, int n, int nbatch, const float *xyz, const float *new_xyz,
                   const int *offset, const int *new_offset, int *idx, float *dist2,
                   void *workspace, size_t workspace_bytes, int reuse_grid, void *stream);

/* amc3d_knnquery(m, kr, ...) answered from the rows of a FINISHED self search of the support (k0 columns, kr < k0,
 * kr <= 31): rows_idx / rows_d2 are the (n, row_stride) outputs of amc3d_knnquery(n, k0, n, ..., xyz, xyz, offset, offset).
 * A query whose coordinates equal those of exactly one support point j of its segment (found in the query's grid cell),
 * and whose row j ascends strictly through column kr with no unfilled slot there, takes columns 0..kr-1 of that row; every
 * other query (no or several such points, a tie, a 1e10 slot) is searched as amc3d_knnquery searches its tied queries.
 * idx (m,kr) and dist2 (m,kr; NULL: not wanted) hold the bits amc3d_knnquery would store.  The workspace is
 * amc3d_knnquery's for (n, m); reuse_grid as there (0: the grid is built here, which needs n >= 256 and nbatch <= 64).
 * Afterwards the int at byte AMC_KNN_FALLBACK_COUNT_OFFSET of the workspace is the number of searched queries. */
#define AMC_KNN_FALLBACK_COUNT_OFFSET 1024
int amc3d_knn_prefix(int m, int kr, int n, int nbatch, const float *xyz, const float *new_xyz, const int *offset,
                     const int *new_offset, int k0, int row_stride, const int *rows_idx, const float *rows_d2, int *idx,
                     float *dist2, void *workspace, size_t workspace_bytes, int reuse_grid, void *stream);

/* k-NN over (b,n,3) / (b,m,3) batches, for models/layers/knn.py and group.py's KNN / DilatedKNN / KNNGroup (the reference
 * composes cdist + topk).  The search is amc3d_knnquery's over uniform segments: same distances, same order of equal
 * distances.  support (b,n,3), query (b,m,3) -> idx (b,m,ksearch/dilation) int32, CLOUD-LOCAL, columns 0, d, 2d, ... of
 * the ksearch nearest; dist NULL, or the EUCLIDEAN distances of those columns as fp32 (b,m,k) [AMC_KNN_DIST_BMK] or
 * (b,k,m) [AMC_KNN_DIST_BKM, what group.py's KNN returns].  dilation divides ksearch; ksearch <= 100 and <= n.
 * query == support (with m == n) takes the search's self-search path.  reuse_grid as for amc3d_knnquery: the workspace
 * was last used by this entry with the same support.  No allocation, no synchronisation, no memset node. */
#define AMC_KNN_DIST_BMK 0
#define AMC_KNN_DIST_BKM 1
size_t amc3d_knn_batch_workspace_bytes(int b, int n, int m, int ksearch);
int amc3d_knn_batch(int b, int n, int m, int ksearch, int dilation, const float *support, const float *query,
                    int *idx, float *dist, int dist_layout, void *workspace, size_t workspace_bytes,
                    int reuse_grid, void *stream);

/* k-NN in FEATURE space (csrc/knn_feat.hip), for models/layers/graph_conv.py's DynConv (the reference composes cdist + topk over
 * a (b,m,n) matrix; here no distance reaches global memory).  support: b clouds of n rows with c channels, query: b clouds of
 * m rows; a cloud is n * c (m * c) consecutive floats and element (row, channel) of it lies at row * row_stride + channel *
 * ch_stride: (c, 1) reads (b,n,c) tensors, (1, n) reads (b,c,n) tensors in place.  query may be support.
 * d2(i,j) = (qq_i + ss_j) - 2 * dot_ij in fp32; dot, qq and ss are fmaf chains over the channels in ascending order from 0 (what
 * the fp32 MFMA computes), so a point's distance to itself is exactly 0.  The list of a query is the ksearch smallest pairs
 * (d2, index) -- farthest != 0: (-d2, index) -- in ascending order: the same bits on every run, whatever the tiling.
 * idx (b,m,ksearch/dilation) int32 cloud-local, columns 0, d, 2d, ... of the list; dist NULL or sqrtf(max(d2, 0)) of those
 * columns in one of the AMC_KNN_DIST_* layouts.  ksearch in 1..100 and <= n, dilation divides it, c >= 1.  NaN inputs are
 * outside the contract.  The workspace size does not depend on n.  No allocation, no synchronisation, no memset node. */
size_t amc3d_knn_features_workspace_bytes(int b, int n, int m, int c, int ksearch);
int amc3d_knn_features(int b, int n, int m, int c, int ksearch, int dilation, int farthest, const float *support,
                       long s_row_stride, long s_ch_stride, const float *query, long q_row_stride, long q_ch_stride, int *idx,
                       float *dist, int dist_layout, void *workspace, size_t workspace_bytes, void *stream);

/* KNNGroup's coordinates (group.py:310-315): dp (b,3,m,k) = support[idx] (- query when `relative`); with `normalize`
 * every cloud is then divided by its own max over (m,k) of sqrt((x*x + y*y) + z*z), taken after the subtraction, which
 * is left in cloud_max (b) (an integer atomic max on the bit pattern: order-independent).  idx (b,m,k) int32
 * cloud-local, clamped to the cloud.  query may be NULL without `relative`, cloud_max without `normalize`. */
int amc3d_knn_group_dp(int b, int n, int m, int k, const float *support, const float *query, const int *idx,
                       int relative, int normalize, float *dp, float *cloud_max, void *stream);

/* The other ten entry points of pointops_api.cpp:14-24 (csrc/pointops.hip).  Layouts: xyz (n,3), new_xyz (m,3), features
 * channel-last (rows of c floats), idx (rows, nsample) int32 GLOBAL row ids, offset / new_offset cumulative segment ends
 * with nbatch entries.  Arithmetic as the reference writes it, left to right, fp32, no FMA.  Every product of sizes that
 * indexes an array must fit in 31 bits (otherwise hipErrorInvalidValue).  The kernels trust idx, as the reference does.
 * `accumulate`: 0 = every output element is written (the sum starts from +0.0f, what the reference computes into its
 * caller's zero-filled buffer); 1 = the reference's `+=` into whatever the buffer holds.
 * Row-local gradients -- grad_input1 of the subtraction, grad_position and grad_weight of the aggregation -- are sequential
 * sums without atomics (the reference uses atomicAdd for two of them): bit-reproducible in either mode.
 * The four scatters -- grouping, interpolation, subtraction's grad_input2, aggregation's grad_input -- use float atomics
 * into a caller-zeroed buffer, as the reference does; deterministic mode replaces them with the scatter_csr gather below. */

/* replaces ballquery_cuda -> ballquery_launcher (pointops/src/ballquery/ballquery_cuda_kernel.cu:26-78).
 * Query q belongs to the first segment s with q < new_offset[s] (a bounded binary search; a query past the last end
 * counts to the last segment); its support is [offset[s-1], offset[s]).  idx row = the first nsample support rows,
 * ascending, with d2 < radius*radius (strict), padded with the first hit; a row with no hit is written as zeros (row 0
 * of the whole batch, not the segment's start: the reference leaves the caller's zero-fill). */
int amc3d_pointops_ballquery(int m, float radius, int nsample, int n, int nbatch, const float *xyz, const float *new_xyz,
                             const int *offset, const int *new_offset, int *idx, void *stream);

/* replaces furthestsampling_cuda (pointops/src/sampling/sampling_cuda_kernel.cu:14-171).  One workgroup per segment:
 * idx[new_start] = start, every later pick the arg-max of the running minimum distance to the earlier picks.  tmp (n) is
 * read as the initial minima (the reference's caller fills it with 1e10) and receives the final ones.  Ties resolve as the
 * reference's strided scan + shared-memory tree does: smallest bit-reversed (k - start) mod block, then lowest k.
 * n_max is the reference's `n` argument (the longest segment; it fixes the reference's block size for all segments): it
 * does not change a pick -- the key is evaluated over 10 bits, whose order refines that of every smaller block; it only
 * selects how many points per thread (4, 8 or 12) keep their running minima in registers, and a segment beyond that budget
 * (longer than 12288, or longer than n_max promised) keeps them in tmp.  n = rows of xyz / tmp (segment ends are clamped to it).  A segment with no
 * sample (new_offset[s] == new_offset[s-1]) or no point writes nothing. */
int amc3d_pointops_furthestsampling(int nbatch, int n_max, int n, const float *xyz, const int *offset,
                                    const int *new_offset, float *tmp, int *idx, void *stream);

/* replaces grouping_forward_cuda / grouping_backward_cuda (grouping_cuda_kernel.cu:5-14, 16-25): input (n,c), idx
 * (m,nsample) -> output[i,j,:] = input[idx[i,j],:]; grad_input[idx[i,j],:] += grad_output[i,j,:] (caller zero-fills) */
int amc3d_pointops_grouping_forward(int m, int nsample, int c, int n, const float *input, const int *idx, float *output,
                                    void *stream);
int amc3d_pointops_grouping_backward(int m, int nsample, int c, int n, const float *grad_output, const int *idx,
                                     float *grad_input, void *stream);

/* replaces interpolation_forward_cuda / interpolation_backward_cuda (interpolation_cuda_kernel.cu:5-18, 20-33): input
 * (m,c), idx / weight (n,k) -> output[i,ch] = ((input[idx[i,0],ch]*weight[i,0]) + input[idx[i,1],ch]*weight[i,1]) + ...;
 * grad_input[idx[i,t],ch] += grad_output[i,ch]*weight[i,t] (caller zero-fills) */
int amc3d_pointops_interpolation_forward(int n, int c, int k, int m, int accumulate, const float *input, const int *idx,
                                         const float *weight, float *output, void *stream);
int amc3d_pointops_interpolation_backward(int n, int c, int k, int m, const float *grad_output, const int *idx,
                                          const float *weight, float *grad_input, void *stream);

/* replaces subtraction_forward_cuda / subtraction_backward_cuda (subtraction_cuda_kernel.cu:5-16, 18-30): input1, input2
 * (n,c), idx (n,nsample) -> output[i,j,:] = input1[i,:] - input2[idx[i,j],:].  Backward: grad_input1[i,ch] = sum over j
 * ascending of grad_output[i,j,ch], sequential from +0.0f, WRITTEN; grad_input2[idx[i,j],ch] += -grad_output[i,j,ch]
 * (caller zero-fills; NULL = skip it, for the scatter_csr route) */
int amc3d_pointops_subtraction_forward(int n, int nsample, int c, const float *input1, const float *input2,
                                       const int *idx, float *output, void *stream);
int amc3d_pointops_subtraction_backward(int n, int nsample, int c, const int *idx, const float *grad_output,
                                        float *grad_input1, float *grad_input2, void *stream);

/* replaces aggregation_forward_cuda / aggregation_backward_cuda (aggregation_cuda_kernel.cu:5-20, 22-39): input (n,c),
 * position (n,nsample,c), weight (n,nsample,w_c), idx (n,nsample) -> output[i,ch] = sum over j ascending of
 * (input[idx[i,j],ch] + position[i,j,ch]) * weight[i,j,ch % w_c].  Backward: grad_position[i,j,ch] = grad_output[i,ch] *
 * weight[i,j,ch % w_c] and grad_weight[i,j,wc] = sum over ch = wc, wc + w_c, ... ascending of grad_output[i,ch] *
 * (input[idx[i,j],ch] + position[i,j,ch]), both WRITTEN; grad_input[idx[i,j],ch] += grad_position[i,j,ch] (caller
 * zero-fills; NULL = skip it, for the scatter_csr route) */
int amc3d_pointops_aggregation_forward(int n, int nsample, int c, int w_c, int accumulate, const float *input,
                                       const float *position, const float *weight, const int *idx, float *output,
                                       void *stream);
int amc3d_pointops_aggregation_backward(int n, int nsample, int c, int w_c, const float *input, const float *position,
                                        const float *weight, const int *idx, const float *grad_output, float *grad_input,
                                        float *grad_position, float *grad_weight, void *stream);

/* The four scatters without atomics (deterministic mode; no counterpart in the reference), as one gather over the
 * reverse lists of idx seen as one flat cloud: rev_start (n_targets + 1), rev_edge (positions) from amc3d_group_csr
 * with b = 1.  out (n_targets,c): every element is written under the SUMMATION ORDER contract stated at
 * amc3d_three_interpolate_grad_csr (ascending position, sequential __fadd_rn from +0.0f, products rounded first by
 * __fmul_rn, exactly +0.0f for a target nobody names).  The term of position p, channel ch, by kind:
 *   0  g[p,ch]                              grouping:      g = grad_output (m*nsample,c)
 *   1  g[p / per,ch] * w[p]                 interpolation: g = grad_output (n,c), w = weight (n*k), per = k
 *   2  -g[p,ch]                             subtraction:   g = grad_output (n*nsample,c)
 *   3  g[p / per,ch] * w[p, ch % w_c]       aggregation:   g = grad_output (n,c), w = weight (n*nsample,w_c), per = nsample */
int amc3d_pointops_scatter_csr(int kind, int n_targets, int c, int per, int w_c, const float *g, const float *w,
                               const int *rev_start, const int *rev_edge, float *out, void *stream);

/* ---- adaptive-margin contrastive loss -------------------------------------------
 * The reference has no native code here: it evaluates this part with torch ops and a Python
 * loop.  These entry points replace, per decoder stage,
 *     openpoints/AMContrast3D/AEF/utils.py:29-41            (amc3d_vote_labels)
 *     openpoints/AMContrast3D/MarginContrast.py:111-115,228-230  (amc3d_posmask)
 *     openpoints/AMContrast3D/AEF/ambiguity.py:11-71 + AEF/function.py:10-39  (amc3d_ambiguity)
 *     openpoints/AMContrast3D/MarginContrast.py:77-79,117-174,250-257  (amc3d_contrast_*)
 * `nbr` is the int32 k-NN index of the stage with `nbr_stride` columns per row; pass the
 * address of the first column to USE (the reference drops column 0, the self match:
 * MarginContrast.py:225-226) and k = number of columns used. */

/* labels[q] = majority class among labels0[nbr_idx[q, 0..kr)] (lowest class id on equal
 * counts): arg-max of the mean one-hot label.  nbr_idx is dense (m,kr), kr <= 128. */
int amc3d_vote_labels(int m, int kr, int num_classes, const int *labels0, const int *nbr_idx, int *labels,
                      void *stream);

/* posmask[i,j] = labels[nbr[i,j]] == labels[i]  -> (m,k) bytes (torch.bool layout) */
int amc3d_posmask(int m, int k, int nbr_stride, const int *labels, const int *nbr, unsigned char *posmask,
                  void *stream);

/* a[i] = ambiguity of point i from its positive mask and neighbour coordinates.
 * mode 1/2/3 = cctype Method1/2/3; beta = ccbeta.  Workspace: amc3d_ambiguity_workspace_bytes(m). */
size_t amc3d_ambiguity_workspace_bytes(int m);
int amc3d_ambiguity(int m, int k, int nbr_stride, int mode, float beta, const float *p,
                    const unsigned char *posmask, const int *nbr, float *a, void *workspace,
                    size_t workspace_bytes, void *stream);

/* amc3d_posmask followed by amc3d_ambiguity as one pass over the neighbour rows (k <= 64: amc3d_loss_rows_supported):
 * posmask (m,k) and a (m) carry the bits those two calls produce.  The workspace has amc3d_ambiguity's size and layout
 * (int max n+ at byte 0; from byte 64: n+ (m) int, d+ (m), d- (m)); a == NULL stops after those statistics. */
int amc3d_loss_rows_supported(int k);
int amc3d_loss_rows(int m, int k, int nbr_stride, int mode, float beta, const int *labels, const float *p,
                    const int *nbr, unsigned char *posmask, float *a, void *workspace, size_t workspace_bytes,
                    void *stream);

/* The anchors that enter the stage loss, 0 < a <= 1 (MarginContrast.py:250-252: the boolean-mask indexing
 * features[mask], neighbor_feature[mask], ...), as a compact ascending list built once per stage plan:
 * sel[0] = count, sel[1..count] = anchor ids; sel holds amc3d_select_anchors_ints(m) ints (the tail is scratch). */
size_t amc3d_select_anchors_ints(int m);
int amc3d_select_anchors(int m, const float *a, int *sel, size_t sel_ints, void *stream);

/* Stage loss = mean over anchors with 0 < a <= 1 of
 *   -log( sum_+ e^{(s-m_i)/T} / (sum_+ e^{(s-m_i)/T} + sum_- e^{s/T}) + 1e-12 ),  m_i = mu*a_i + nu,
 * s = cosine similarity of the (m,C) embeddings f.  Outputs: norm (m) clamped row norms, sim (m,k),
 * loss_pt (m), mean_cnt[2] = {stage loss, number of anchors}; all kept for the backward.
 * sel: the list of amc3d_select_anchors for this a (sim / loss_pt are then written for the listed anchors
 * only), or NULL to visit and test every anchor.
 * unit (m,C) or NULL: receives the unit rows f_i / norm_i; with it (and C in {16, 32, 64, 128, 256}, 16-byte aligned rows) the
 * row-gather kernels run on those rows -- no division per fetched neighbour element -- and amc3d_contrast_backward_mutual
 * takes the same buffer; NULL: the generic kernel on f and norm. */
int amc3d_contrast_forward(int m, int C, int k, int nbr_stride, const float *f, const int *nbr,
                           const unsigned char *posmask, const float *a, const int *sel, float mu, float nu,
                           float temperature, float *norm, float *unit, float *sim, float *stats, float *loss_pt,
                           float *mean_cnt, void *stream);
/* stats (m,2) or NULL: with the unit-row kernels the pass leaves, per visited anchor, the two sums of exponentials its loss is made
 * of -- amc3d_contrast_backward_mutual builds its per-anchor records from them instead of re-reading sim, and sim may then be NULL
 * (the cosines are not stored: the mutual-edge backward recomputes the ones it needs from the unit rows it fetches anyway). */

/* The same on CHANNEL-major embeddings f_cm (b, C, n) -- the decoder's layout; pointnext_AA.py:518-519 makes the point-major
 * copy with flatten(transpose) -- m = b * n anchors in cloud-major order.  C in {16, 32, 64, 128, 256}; unit (b*n, C) is required
 * and receives the point-major unit rows (what amc3d_contrast_backward_mutual reads); no point-major copy of f is made. */
int amc3d_contrast_forward_cm(int b, int C, int n, int k, int nbr_stride, const float *f_cm, const int *nbr,
                              const unsigned char *posmask, const float *a, const int *sel, float mu, float nu,
                              float temperature, float *norm, float *unit, float *sim, float *stats, float *loss_pt,
                              float *mean_cnt, void *stream);

/* grad_f (m,C) += grad_out[0] * d(stage loss)/d f; the caller zero-initialises grad_f.
 * grad_out is a DEVICE scalar (no host sync).  C <= 512.  sel as in the forward. */
int amc3d_contrast_backward(int m, int C, int k, int nbr_stride, const float *f, const float *norm,
                            const int *nbr, const unsigned char *posmask, const float *a, const int *sel, float mu,
                            float nu, float temperature, const float *sim, const float *mean_cnt,
                            const float *grad_out, float *grad_f, void *stream);

/* The same gradient as a gather over reverse lists instead of float atomics (group_points_grad-style scatter,
 * MarginContrast.py:250-257 through autograd's index_put backward): fixed summation order, every row of grad_f WRITTEN
 * once (no zero-initialisation).  rev = [rev_start (m+1) | rev_edge (m*k)] int32 from amc3d_contrast_csr: the positions
 * i*k + j, ascending, of the selected anchors i whose neighbour j is row n; built with the stage's plan (coordinates and
 * labels only).  gco: m*k floats of scratch (dL/ds per edge).  16-byte aligned rows, and a width C with
 * amc3d_contrast_backward_rows_supported(C): C % 4 == 0 and 4 <= C <= 512.
 * Summation order (part of the contract: deterministic mode promises the bits):
 *   C in {16, 32, 64, 128, 256} (amc3d_contrast_backward_csr_supported; the same predicate gates the unit-row forward, the
 *     channel-major stage and the mutual-edge backward): R = 256 / C edges per round on R groups of C/4 lanes; group r sums
 *     the edges t = r, r + R, .. sequentially from +0.0f, then the groups' sums are added in a butterfly (xor C/4, .., 32).
 *   every other supported width: each output element is the sequential fp32 sum from +0.0f over the edges t = 0, 1, ..
 *   In both, the edges of row n are numbered: its own slots 0..k-1 (only if n is a selected anchor), then its reverse list
 *   in list order, which is ascending position.  A row with no edge receives +0.0f. */
size_t amc3d_contrast_csr_workspace_bytes(int m);
int amc3d_contrast_csr(int m, int k, int nbr_stride, const int *nbr, const int *sel, int *rev, void *workspace,
                       size_t workspace_bytes, void *stream);
int amc3d_contrast_backward_csr_supported(int C);
int amc3d_contrast_backward_rows_supported(int C);
int amc3d_contrast_backward_csr(int m, int C, int k, int nbr_stride, const float *f, const float *norm, const int *nbr,
                                const unsigned char *posmask, const float *a, const int *sel, const int *rev, float mu,
                                float nu, float temperature, const float *sim, const float *mean_cnt,
                                const float *grad_out, float *gco, float *grad_f, void *stream);

/* The default since round 3: the gradient over the MUTUAL edges.  In the stages' k-NN graphs ~90 % of the edges are mutual
 * (x in N(n) and n in N(x)); cosine and positive mask are symmetric in an edge's two ends, so row n, walking its own list
 * once, computes both directions of every mutual edge from one fetch of f[x] and a 32-byte record of x; only the non-mutual
 * edges of the selected anchors need reverse lists.  Every row of grad_f is WRITTEN once (no zero-initialisation), fixed
 * summation order, no float atomics.
 * amc3d_contrast_mutual: mutual (m*k) bytes, mutual[i*k+s] = how often i is in the list of nbr[i][s] (0 / 1 in a k-NN graph;
 *   counted at the first slot naming that neighbour); rev = [rev_start (m+1) |
 *   rev_edge (m*k)] int32: per row n the positions i*k+s, ascending, of the NON-mutual edges of the anchors with
 *   0 < a[i] <= 1 that point at n (those edges also carry bit 0x80 in mutual[]; the count is in the low 7 bits).  k <= 64.  Coordinates and labels only: part of the stage's plan.  Workspace:
 *   amc3d_contrast_csr_workspace_bytes(m).
 * amc3d_contrast_backward_mutual: workspace amc3d_contrast_backward_mutual_workspace_bytes(m) (the per-anchor records);
 *   unit, norm, sim, mean_cnt as amc3d_contrast_forward wrote them.  C in {16, 32, 64, 128, 256}. */
size_t amc3d_contrast_mutual_workspace_bytes(int m);
int amc3d_contrast_mutual(int m, int k, int nbr_stride, const int *nbr, const float *dist2, const float *a,
                          unsigned char *mutual, int *rev, void *workspace, size_t workspace_bytes, void *stream);
size_t amc3d_contrast_backward_mutual_workspace_bytes(int m);
int amc3d_contrast_backward_mutual(int m, int C, int k, int nbr_stride, const float *unit, const float *norm, const int *nbr,
                                   const unsigned char *posmask, const float *a, const unsigned char *mutual, const int *rev,
                                   float mu, float nu, float temperature, const float *sim, const float *stats /* or NULL */,
                                   const float *mean_cnt, const float *grad_out, void *workspace, size_t workspace_bytes,
                                   float *grad_f, void *stream);

/* All stages of the loss in one call, on channel-major embeddings: what amc3d_contrast_forward_cm (with stats, without sim) and
 * amc3d_contrast_backward_mutual compute per stage, in three launches forward (unit rows, the anchors' losses, one workgroup
 * of means) and two backward (records, gather) for ALL stages, with the gradient stored channel-major.  A stage:
 *   sizes    b clouds of n points (m = b * n anchors, cloud-major), C in {16, 32, 64, 128, 256}, k <= nbr_stride
 *   inputs   f_cm (b, C, n); nbr, posmask, a, sel, mutual, rev as the single-stage entries take them
 *   buffers  norm (m), unit (m, C), stats (m, 2), loss_pt (m), mean_cnt (2) written by the forward and read by the backward;
 *            grad_cm (b, C, n), every element written by the backward; rec is the library's (it points the backward's
 *            records into `workspace`; what the caller puts there is not read)
 * f_cm and unit 16-byte aligned, m * C < 2^34.  A stage that fails a check makes the call return an error before anything is
 * launched; nstages == 0 does nothing, more than AMC_CONTRAST_MAX_STAGES is an error.
 * forward:  every mean_cnt as amc3d_contrast_forward_cm writes it, and total[0] = scale * (((l_0 + l_1) + l_2) + ...), l_s the
 *           stage losses, each operation rounded to fp32 (the caller's additions and its loss weight).
 * backward: grad_cm_s = (grad_out[0] * scale) * d l_s / d f_cm_s; grad_out a device scalar.  A gradient element has the bits
 *           amc3d_contrast_backward_mutual leaves in the row-major gradient. */
#define AMC_CONTRAST_MAX_STAGES 8
typedef struct AmcContrastStage {
    int b, C, n, k, nbr_stride;
    const float *f_cm;
    const int *nbr;
    const unsigned char *posmask;
    const float *a;
    const int *sel;
    const unsigned char *mutual;
    const int *rev;
    float *norm, *unit, *stats, *loss_pt, *mean_cnt;
    void *rec;
    float *grad_cm;
} AmcContrastStage;
int amc3d_contrast_stages_forward_cm(int nstages, const AmcContrastStage *stages, float mu, float nu, float temperature,
                                     float scale, float *total, void *stream);
size_t amc3d_contrast_stages_backward_cm_workspace_bytes(int nstages, const AmcContrastStage *stages);
int amc3d_contrast_stages_backward_cm(int nstages, const AmcContrastStage *stages, float mu, float nu, float temperature,
                                      float scale, const float *grad_out, void *workspace, size_t workspace_bytes, void *stream);

/* The other forms of the loss, openpoints/AMContrast3D/MarginContrast.py:117-174 as a whole (what the ambiguity_args knobs
 * margin / db / supervisedCL / temperature select) on the stage of :250-257; the entry points above are the one form the
 * shipped configs use.  A form is four integers, passed at run time:
 *   margin_mode      0 constant (m = nu, :120-121)   1 adaptive (m = mu a_i + nu, :122-125)
 *                    2 learned  (m = (u_i - 1) a_i + v_i, u_i / v_i the means over all k slots of the negatives' / positives'
 *                      cosines, :127-130; the margin is differentiated through, as autograd does there)
 *   db               0 none (:144-145)   1 "-m": positives minus m (:140-141)   2 "+m": negatives plus m (:142-143)
 *   method           1 Method1 -log(P / (P + N) + 1e-12) (:163-164)
 *                    2 Method2 -log(sum_j (e_j pos_j / (e_j pos_j + N) + 1e-12) / (npos + 1e-12)), j over all k slots (:165-171)
 *   has_temperature  0: no division (temperature: null, :148-149); 1: the exponent is divided by `temperature`
 * Any other value is a bad argument.  mu is read by margin_mode 1 only, nu by 0 and 1.
 * forward: norm (m), unit (m,C) or NULL, sel as in amc3d_contrast_forward, and with the same choice of kernels, so that sim
 *   (m,k) -- required here -- holds the same bits; loss_pt (m) and mean_cnt (2) as there.
 * backward: gco (m*k floats of scratch) receives dL/ds per edge of the visited anchors; then
 *   rev != NULL (from amc3d_contrast_csr: ALL edges of the selected anchors; never the lists of amc3d_contrast_mutual):
 *     the gather of amc3d_contrast_backward_csr, in its summation order -- needs sel, amc3d_contrast_backward_rows_supported(C)
 *     and 16-byte aligned rows; every row of grad_f is written, no zero-initialisation;
 *   rev == NULL: float atomics as amc3d_contrast_backward, C <= 512, the caller zero-initialises grad_f.
 * No allocation, no synchronisation. */
int amc3d_contrast_variant_forward(int m, int C, int k, int nbr_stride, const float *f, const int *nbr,
                                   const unsigned char *posmask, const float *a, const int *sel, int margin_mode, int db,
                                   int method, int has_temperature, float mu, float nu, float temperature, float *norm,
                                   float *unit /* or NULL */, float *sim, float *loss_pt, float *mean_cnt, void *stream);
int amc3d_contrast_variant_backward(int m, int C, int k, int nbr_stride, const float *f, const float *norm, const int *nbr,
                                    const unsigned char *posmask, const float *a, const int *sel, const int *rev /* or NULL */,
                                    int margin_mode, int db, int method, int has_temperature, float mu, float nu,
                                    float temperature, const float *sim, const float *mean_cnt, const float *grad_out,
                                    float *gco, float *grad_f, void *stream);

/* ---- grouped 1x1 convolution fused with its gather (fp32 MFMA) ------------------------------------
 * Replaces, for the first layer of a SetAbstraction / LocalAggregation MLP, the chain
 *   grouping_operation(features, idx) -> torch.cat([dp, fj], 1) -> nn.Conv2d 1x1 (bias-free)
 * (openpoints/models/layers/group.py:244-255,323-325; backbone/pointnext_AA.py:57-63,164-166) and its
 * backward (conv backward, slice, group_points_grad) without materialising the (b,cin+3,npoints,nsample)
 * input.  f_pm is the POINT-major (b,n,cin) copy of the features (amc3d_transpose_cn), dp the
 * (b,3,npoints,nsample) relative positions, weight the (cout, cin+3) conv weight with the reference's
 * channel order [dp, features].  Supported: cin <= 64, cout in {32,64,96,128}. */
int amc3d_grouped_conv_supported(int cin, int cout);
int amc3d_transpose_cn(int b, int c, int n, const float *src, float *dst, void *stream);
int amc3d_grouped_conv_forward(int b, int cin, int cout, int n, int npoints, int nsample, const float *f_pm,
                               const float *dp, const int *idx, const float *weight, float *y, void *stream);
size_t amc3d_grouped_conv_workspace_bytes(int b, int cin, int cout, int npoints, int nsample);
/* df_pm (b,n,cin) += scatter(W[:,3:]^T dy) (zero-initialised by the caller; NULL to skip),
 * dweight (cout,cin+3) = dy . X^T (NULL to skip) */
int amc3d_grouped_conv_backward(int b, int cin, int cout, int n, int npoints, int nsample, const float *f_pm,
                                const float *dp, const int *idx, const float *weight, const float *dy,
                                float *df_pm, float *dweight, void *workspace, size_t workspace_bytes, void *stream);

/* Confusion matrix of the training predictions (examples/segmentation/main_AA.py:414-415, utils/metrics.py:50-75:
 * cm.update(logits.argmax(dim=1), target) every iteration): cm (v*v) int64 += histogram of (target, arg-max over the class
 * planes of logits (B,C,N); first maximum as torch.argmax), v = C + has_ignore <= 64 (points whose target == ignore count in
 * the extra row and column); invalid (1) int64 += points whose target lies outside [0, v).  One launch. */
int amc3d_confusion_update(int B, int C, long N, const float *logits, const long long *target, long long ignore,
                           int has_ignore, long long *cm, long long *invalid, void *stream);

/* ---- point losses over channel-major logits -------------------------------------------------------
 * The criteria of openpoints.loss (loss/build.py:14-257, 328-340) without the (B*N, C) transposed copy of the logits, as two
 * form-generic families on one layout and summation order (two launches forward, one backward, no atomics, nothing zero-filled,
 * any C >= 1; fixed-order fp64 sum over the points, so equal inputs give equal bits).  logits (B,C,N) fp32, target (B,N) int64.
 * A point whose class falls outside [0, C) is left out and gets a zero gradient row; with nothing counted a mean is 0/0 = NaN,
 * as torch's, and dlogits all zero.  loss_den[2] = {loss, den}; den_mode 0: den = the counted points (softmax) or their
 * elements (sigmoid), 1: den = sum of w[y] (softmax only), 2: den = 1 (reduction 'sum').  One workspace query serves every
 * forward entry below.
 *
 * Softmax family.  A point is dropped when has_ignore and target == ignore_index, or when mask (B,N) int32 is given and its
 * entry != 1; then y = remap[target] when remap (remap_len int64 entries) is given, target otherwise.  lp = log_softmax,
 * p = softmax, w = weight (C) or ones.  eps in [0, 1) smooths the target distribution q: eps_rule 0 is torch's
 * (q[y] = 1 - eps + eps/C, q[c != y] = eps/C), eps_rule 1 SmoothCrossEntropy's (q[y] = 1 - eps, q[c != y] = eps/(C-1); NaN at
 * C = 1 as there).  weight_per_class 1: Q[c] = q[c] w[c], m0 = 1;  0: Q[c] = q[c], m0 = w[y].  alpha (C) or NULL, gamma >= 0:
 *   m = m0 alpha[y] (1 - p[y])^gamma                    (0^0 = 1; m is a constant of the backward: FocalLoss detaches pt)
 *   term_i = m sum_c Q[c] (-lp_i[c]) + poly (1 - p_i[y])
 *   loss = sum_i term_i / den
 *   dlogits_i[c] = grad_out[0] / den * [ m (p_i[c] sum_c Q[c] - Q[c]) + poly p_i[y] (p_i[c] - [c == y]) ]
 * lse (B,N) out (saved for backward).  The forms:
 *   nn.CrossEntropyLoss() with its defaults, as CrossEntropyAce applies it: amc3d_cross_entropy_forward / _backward, the form
 *     with nothing but ignore_index set (mean_cnt = loss_den), on the native exp / log instructions; every other form uses expf / logf
 *   F.cross_entropy with weight and label_smoothing: weight_per_class 1, eps_rule 0, den_mode 1
 *   SmoothCrossEntropy: eps_rule 1, weight_per_class 1, den_mode 0 (eps = 0: weight_per_class 0, den_mode 1)
 *   MaskedCrossEntropy: mask, eps_rule 0;  FocalLoss: gamma, alpha, den_mode 0 or 2
 *   Poly1CrossEntropyLoss: poly, weight_per_class 0, den_mode 0 or 2
 *
 * Sigmoid family: elementwise over (B,C,N) against the one-hot of target, formed on the fly.  For logit x and target bit t:
 * z = t ? -x : x, u = sigmoid(z) = 1 - pt, ce = max(x,0) - x t + log1p(exp(-|x|)) = -log(pt),
 *   a = w[c] (t ? pos_weight[c] : 1) (alpha >= 0 ? (t ? alpha : 1 - alpha) : 1)
 *   value = a ce u^gamma + poly u^(gamma+1)
 *   d value / d z = u^gamma [ a (u + ce gamma (1 - u)) + poly (gamma + 1) u (1 - u) ],  d z / d x = t ? -1 : 1
 * BCELogits: weight / pos_weight (C) or NULL, alpha < 0, gamma = poly = 0;  Poly1FocalLoss: alpha, gamma, poly, no weights. */
size_t amc3d_cross_entropy_workspace_bytes(int B, long N);
int amc3d_cross_entropy_forward(int B, int C, long N, const float *logits, const long long *target,
                                long long ignore_index, float *lse, float *mean_cnt, void *workspace,
                                size_t workspace_bytes, void *stream);
int amc3d_cross_entropy_backward(int B, int C, long N, const float *logits, const long long *target,
                                 long long ignore_index, const float *lse, const float *mean_cnt,
                                 const float *grad_out, float *dlogits, void *stream);
int amc3d_point_loss_softmax_forward(int B, int C, long N, const float *logits, const long long *target,
                                     const long long *remap, int remap_len, long long ignore_index, int has_ignore,
                                     const int *mask, const float *weight, int weight_per_class, float eps, int eps_rule,
                                     float gamma, const float *alpha, float poly, int den_mode, float *lse, float *loss_den,
                                     void *workspace, size_t workspace_bytes, void *stream);
int amc3d_point_loss_softmax_backward(int B, int C, long N, const float *logits, const long long *target,
                                      const long long *remap, int remap_len, long long ignore_index, int has_ignore,
                                      const int *mask, const float *weight, int weight_per_class, float eps, int eps_rule,
                                      float gamma, const float *alpha, float poly, int den_mode, const float *lse,
                                      const float *loss_den, const float *grad_out, float *dlogits, void *stream);
int amc3d_point_loss_sigmoid_forward(int B, int C, long N, const float *logits, const long long *target, const float *weight,
                                     const float *pos_weight, float alpha, float gamma, float poly, int den_mode, float *loss_den,
                                     void *workspace, size_t workspace_bytes, void *stream);
int amc3d_point_loss_sigmoid_backward(int B, int C, long N, const float *logits, const long long *target, const float *weight,
                                      const float *pos_weight, float alpha, float gamma, float poly, int den_mode,
                                      const float *loss_den, const float *grad_out, float *dlogits, void *stream);

/* ---- pointwise (1x1) convolution on fp32 MFMA -----------------------------------------------------
 * Replaces the nn.Conv1d / nn.Conv2d (kernel size 1) layers of the path, which the reference builds in
 * openpoints/models/layers/conv.py:8-21 and runs through cuDNN.  Channel-major tensors: x (b,cin,P),
 * y (b,cout,P), weight (cout,cin), bias (cout) or NULL; P = points (Conv1d) or points*neighbours (Conv2d). */
int amc3d_pointwise_conv_forward(int b, int cin, int cout, long P, const float *x, const float *weight,
                                 const float *bias, float *y, void *stream);
/* forward with scratch: the short deep layers (>= 64 channels on both sides, a few hundred positions per cloud) split their K
 * axis over workgroups and sum the partial products in a fixed order; amc3d_pointwise_conv_forward_workspace_bytes() is 0
 * for every other shape (the call is then amc3d_pointwise_conv_forward) */
size_t amc3d_pointwise_conv_forward_workspace_bytes(int b, int cin, int cout, long P, int has_bias);
int amc3d_pointwise_conv_forward_ws(int b, int cin, int cout, long P, const float *x, const float *weight,
                                    const float *bias, float *y, void *workspace, size_t workspace_bytes, void *stream);
size_t amc3d_pointwise_conv_workspace_bytes(int b, int cin, int cout, long P);
/* dx (b,cin,P) = weight^T . dy (NULL to skip; weight may then be NULL too); dweight (cout,cin) = sum_{b,p} dy x^T (NULL to skip; needs
 * x and the workspace; summed in a fixed order -> deterministic) */
int amc3d_pointwise_conv_backward(int b, int cin, int cout, long P, const float *x, const float *weight,
                                  const float *dy, float *dx, float *dweight, void *workspace,
                                  size_t workspace_bytes, void *stream);
/* The same two calls with a row stride (in floats, >= cin) for weight and for dweight, so that a column block of a wider
 * matrix is an operand where it lies: weight = W + c1 with ldw = c1 + c2 is the right block of W (rows, c1 + c2).  dweight's
 * columns outside the block are left untouched.  A block that does not start on a 16-byte boundary (or whose stride is no
 * multiple of 4) takes 4-byte loads for the weight operand only; sums and their order are those of the calls above.
 * workspace: amc3d_pointwise_conv_forward_workspace_bytes() / amc3d_pointwise_conv_workspace_bytes() bytes.
 * dx_position_major != 0: dx is written as (b,P,cin) rows instead of (b,cin,P) -- the same values, four consecutive channels
 * of a position per 16-byte store -- the layout amc3d_grouped_conv_bn_backward reads from its lists with dx1_position_major = 1. */
int amc3d_pointwise_conv_forward_strided(int b, int cin, int cout, long P, const float *x, const float *weight, long ldw,
                                         const float *bias, float *y, void *workspace, size_t workspace_bytes, void *stream);
int amc3d_pointwise_conv_backward_strided(int b, int cin, int cout, long P, const float *x, const float *weight, long ldw,
                                          const float *dy, float *dx, int dx_position_major, float *dweight, long lddw,
                                          void *workspace, size_t workspace_bytes, void *stream);
/* The strided forward without a bias, y_pm written as position-major rows (b,P,cout): the layout the neighbourhood layers
 * gather from (amc3d_local_aggregation_forward, amc3d_grouped_conv_bn_forward with g_cm == NULL).  Same route, accumulators and sums
 * as amc3d_pointwise_conv_forward_strided: y_pm equals its output transposed, bit for bit.  A lane stores four consecutive
 * channels of its position as 16 bytes (y_pm 16-byte aligned and cout % 4 == 0), as four 4-byte stores otherwise.
 * workspace: amc3d_pointwise_conv_forward_workspace_bytes(b, cin, cout, P, 0) bytes. */
int amc3d_pointwise_conv_forward_rows(int b, int cin, int cout, long P, const float *x, const float *weight, long ldw,
                                      float *y_pm, void *workspace, size_t workspace_bytes, void *stream);
/* Test and measurement entries of the deep layers' MFMA GEMM (csrc/gemm.hip); the product path calls neither.
 * amc3d_gemm_tile_for: the output tile the dispatch rule gives a launch of M x N outputs per (batch * splits) slice:
 * 0 = 128 x 128, 1 = 64 x 128, 2 = 64 x 64 (-1 for a non-positive argument).  A function of its four arguments only.
 * amc3d_gemm_probe: ONE product on that kernel with tile tile_id FORCED, whatever the channel counts, with the K split of the
 * real route.  product 0: forward, out (b,cout,P) = w (cout,cin; row stride ldw) . x_or_dy (b,cin,P); 1: backward-data,
 * out (b,cin,P) = w^T . x_or_dy (b,cout,P); for both pm != 0 writes out as position-major rows, and the K axis is split when the
 * workspace holds amc3d_pointwise_conv_forward_workspace_bytes(b,cin,cout,P,0) bytes (forward; the route's own rule for
 * backward-data, at most amc3d_pointwise_conv_workspace_bytes).  product 2: the generic weight gradient, out (cout,cin; row
 * stride ldw) = sum x_or_dy (b,cout,P) . w (b,cin,P)^T, pm = 0, workspace of amc3d_pointwise_conv_workspace_bytes.  Every
 * tile gives the same bits. */
int amc3d_gemm_tile_for(int M, int N, int batch, int splits);
int amc3d_gemm_probe(int tile_id, int product, int b, int cin, int cout, long P, long ldw, int pm, const float *x_or_dy,
                     const float *w, float *out, void *workspace, size_t workspace_bytes, void *stream);

/* a weight matrix cut into two column blocks / two gradient blocks joined (the [W_dp | W_f] weight of a neighbourhood layer,
 * the [W_skip | W_up] weight of a FeaturePropagation conv): w (rows, c1 + c2) <-> a (rows, c1), b (rows, c2), one launch */
int amc3d_split_columns(int rows, int c1, int c2, const float *w, float *a, float *b, void *stream);
int amc3d_join_columns(int rows, int c1, int c2, const float *a, const float *b, float *w, void *stream);
/* dbias (c) = sum_{b,p} dy (b,c,P): bias gradient of a 1x1 convolution with bias (the stem conv and the head's last conv,
 * base_seg.py:236-252, pointnext_AA.py:104-127 with is_head), summed in a fixed order */
int amc3d_bias_grad(int b, int c, long P, const float *dy, float *dbias, void *stream);
/* 1x1 convolution with a per-cloud additive term: y (b,cout,P) = weight (cout,cin; row stride ldw >= cin) . x (b,cin,P)
 * + cloud_term (b,cout) broadcast along P.  The first FeaturePropagation conv of the part-segmentation decoders
 * (pointnext.py:628-663, pointnetv2.py:498-511) convolves input channels that are constant along the points of a cloud (the
 * shape-category embedding); their product with the weight is cloud_term = e (b,E) . W_cls^T, so no (b, E + cin, P) tensor
 * is built.  Route, accumulators and sums of amc3d_pointwise_conv_forward_strided without a bias: with cloud_term == 0 the
 * output equals that call's, bit for bit.  The streaming kernel adds the term in its epilogue (a workgroup's tile lies in one
 * cloud); behind the 128 x 128-tile GEMM (>= 64 channels on both sides) it is a pass of its own, as that route's bias is.
 * Any b >= 1: more than 65535 clouds run in launches of 65535 clouds each.
 * workspace: amc3d_pointwise_conv_forward_workspace_bytes(b, cin, cout, P, 0) bytes.
 * amc3d_cloud_term_grad: dterm (b,cout) = sum_p dy (b,cout,P), one workgroup of fixed size per (cloud, channel) row, summed in
 * a fixed order without float atomics (the same bits on every run).  dx and dweight are amc3d_pointwise_conv_backward*'s. */
int amc3d_pointwise_conv_cloud_term_forward(int b, int cin, int cout, long P, const float *x, const float *weight, long ldw,
                                            const float *cloud_term, float *y, void *workspace, size_t workspace_bytes,
                                            void *stream);
int amc3d_cloud_term_grad(int b, int cout, long P, const float *dy, float *dterm, void *stream);

/* ---- residual branch of a strided SetAbstraction block (openpoints/models/backbone/pointnext_AA.py:157-168, use_res):
 *     fi = torch.gather(f, -1, idx...); identity = self.skipconv(fi); ...; f = self.act(f + identity)
 * forward:  out (b,cout,m) = relu(y + weight . f[:, :, fps_idx] + bias), f (b,cin,n), fps_idx (b,m) int32 (the FPS picks;
 *           repeats allowed: their gradients sum, as torch.gather's backward does), weight (cout,cin), bias (cout) or NULL, y (b,cout,m) = the pooled main branch;
 *           fi (b,cin,m) or NULL = the gathered columns, kept for the weight gradient.
 * backward: g (b,cout,m) = dout * (out > 0) -- the gradient w.r.t. y AND w.r.t. the skip conv's output;
 *           df (b,cin,n) or NULL = weight^T . g at the sampled columns, zero elsewhere (written whole: no pre-zeroing);
 *           dweight (cout,cin) or NULL (needs fi; fixed-order partial sums); dbias (cout) or NULL (fixed order). */
int amc3d_sa_residual_forward(int b, int cin, int cout, int n, int m, const float *f, const int *fps_idx,
                              const float *weight, const float *bias, const float *y, float *out, float *fi, void *stream);
size_t amc3d_sa_residual_workspace_bytes(int b, int cin, int cout, int m);
int amc3d_sa_residual_backward(int b, int cin, int cout, int n, int m, const float *dout, const float *out,
                               const float *fi, const int *fps_idx, const int *dup_flag, const float *weight, float *g, float *df,
                               float *dweight, float *dbias, void *workspace, size_t workspace_bytes, void *stream);
/* dup_flag: DEVICE int of amc3d_index_duplicates for these picks, or NULL.  torch.gather's backward (pointnext_AA.py:157) SUMS
 * over repeated picks -- FPS re-picks a point when a cloud holds fewer distinct points than picks (crop_pc pads small rooms by
 * repetition, data_util.py:161-167) -- so the scatter of df adds (float atomics) when the flag is 1 or unknown, and stores plainly
 * when the plan found the picks distinct. */
size_t amc3d_index_duplicates_workspace_bytes(int b, int n);
int amc3d_index_duplicates(int b, int n, int m, const int *idx, int *flag, void *workspace, size_t workspace_bytes, void *stream);

/* ---- input pipeline on the device (openpoints/dataset/data_util.py:92-174; dataset/s3dis/s3dis.py:122-144) -----------
 * voxelize: floor(coord / voxel_size) in float64 -> FNV-1a 64-bit hash of the three cell coordinates (fnv_hash_vec) ->
 * stable sort by key -> voxel ids / starts / counts.  coord (n,3) fp32 must be shifted to its min corner (crop_pc does
 * that first).  numpy's argsort is not stable, so the reference leaves the order of the points inside one voxel
 * unspecified; idx_sort here is the stable order.  key (n) = hash per point; idx_sort (n); voxel_idx (n) = voxel id of
 * sorted position i (np.unique's inverse); start (n+1); count (n, zero beyond nvox); nvox (1) -- all device memory. */
size_t amc3d_voxelize_workspace_bytes(int n);
int amc3d_voxelize(int n, const float *coord, double voxel_size, unsigned long long *key, int *idx_sort, int *voxel_idx,
                   int *start, int *count, int *nvox, void *workspace, size_t workspace_bytes, void *stream);
/* train mode (data_util.py:136-140): idx_unique[v] = idx_sort[start[v] + rnd[v] % count[v]], rnd = the caller's
 * np.random.randint(0, count.max(), nvox) draw */
int amc3d_voxel_select(int nvox, const int *start, const int *count, const int *idx_sort, const int *rnd, int *idx_unique,
                       void *stream);
/* crop_pc's crop (data_util.py:157-160): d2 (n) fp32 = squared distances to coord[init_idx] (((dx^2+dy^2)+dz^2), no
 * contraction), crop_idx (keep) = indices of the keep nearest points in ascending distance */
size_t amc3d_crop_nearest_workspace_bytes(int n);
int amc3d_crop_nearest(int n, const float *coord, int init_idx, int keep, float *d2, int *crop_idx, void *workspace,
                       size_t workspace_bytes, void *stream);
/* float64 coordinates (ScanNet: np.dot(pos_f32, R_f64) makes the rooms float64 before crop_pc): the same hash of
 * floor(coord / voxel_size), and d2 (n) double = ((dx^2+dy^2)+dz^2) in double, sorted on its 64-bit pattern.  voxelize_f64
 * takes amc3d_voxelize_workspace_bytes(n). */
int amc3d_voxelize_f64(int n, const double *coord, double voxel_size, unsigned long long *key, int *idx_sort, int *voxel_idx,
                       int *start, int *count, int *nvox, void *workspace, size_t workspace_bytes, void *stream);
size_t amc3d_crop_nearest_f64_workspace_bytes(int n);
int amc3d_crop_nearest_f64(int n, const double *coord, int init_idx, int keep, double *d2, int *crop_idx, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---- neighbourhood aggregation with one grouped conv: "convolve first, gather after" ---------------------------------
 * LocalAggregation.forward / single-layer SetAbstraction.forward (openpoints/models/backbone/pointnext_AA.py:57-63,
 * 139-170; layers/group.py:244-255, 323-325): grouping_operation -> cat([dp, fj]) -> Conv2d 1x1 -> BatchNorm2d (batch
 * statistics) [-> ReLU] -> max over the nsample neighbours.  W . [dp ; f[idx]] = (W_f . f)[idx] + W_dp . dp, so the conv
 * runs on the n source points (amc3d_pointwise_conv_forward), BatchNorm's statistics follow from n-sized sums and the
 * geometry moments below, and the only pass over npoints * nsample positions is the gather + max itself (csrc/lagg.hip).
 * Supported: cout in {8,16,32,64,128} or a multiple of 128; nsample <= 64. */
int amc3d_local_aggregation_supported(int cout, int nsample);
/* geometry moments of a neighbourhood query (coordinates only; part of the geometry plan): idx (b,npoints,nsample) into
 * the n support points, dp (b,3,npoints,nsample) -> opaque buffer holding each support point's in-degree and the sum of
 * the dp that reference it (fixed point: independent of the order of the atomics) and the global sums of dp and dp dp^T */
size_t amc3d_group_moments_bytes(int b, int n);
int amc3d_group_moments(int b, int n, int npoints, int nsample, const int *idx, const float *dp, void *moments,
                        size_t moments_bytes, void *stream);
/* The pooled layer.  G = W_f . f comes from the caller in one of two layouts.  g_cm == NULL: g_pm (b,n,cout), 16-byte aligned,
 * already holds its rows and is an INPUT (amc3d_pointwise_conv_forward_rows writes them; no channel-major G exists).
 * Otherwise g_cm (b,cout,n) (amc3d_pointwise_conv_forward) is first transposed into g_pm (amc3d_transpose_cn).
 * w_dp = the conv weight's dp columns at a row stride of ldw floats (>= 3): w_dp = W, ldw = cin + 3 reads them inside the
 * layer's own (cout, cin + 3) weight, no split.
 * Outputs: pooled (b,cout,npoints), arg (b,cout,npoints) bytes = torch.max's indices, ystar = the pre-BatchNorm value at
 * arg, gd (cout,3) doubles (all kept for backward, with g_pm), mean / invstd / var_unbiased (cout) + nn.BatchNorm's running
 * update when running_mean != NULL (momentum < 0: left to the caller).  The statistics read the rows; their partial sums are
 * taken over a fixed partition of the b*n points in a fixed order (the same bits on every run).
 * training == 0 (eval): mean / invstd are inputs (running statistics); moments, gd, var_unbiased, workspace may be NULL, and
 * with g_cm == NULL nothing is launched but the max-pool.
 * Statistics over several ranks (the reference converts every BatchNorm to SyncBatchNorm when world_size > 1,
 * main_AA.py:146-148): phase 0 = one rank, everything in one call.  phase 1 writes this rank's {sum y, sum y^2} per channel
 * and its position count to sums (2*cout + 1 doubles) and returns; the caller all-reduces sums; phase 2 finishes from the
 * reduced sums (same arguments, same workspace).  Backward likewise: phase 1 -> dsums (2*cout doubles: sum dq, sum dq xhat),
 * all-reduce, phase 2 with count = sums + 2*cout of the forward call; parameter gradients stay rank-local. */
size_t amc3d_local_aggregation_workspace_bytes(int b, int cout, int n, int npoints);
int amc3d_local_aggregation_forward(int b, int cout, int n, int npoints, int nsample, int training, int relu, float eps,
                                    float momentum, const float *g_cm, const int *idx, const float *dp, const float *w_dp,
                                    long ldw, const void *moments, const float *gamma, const float *beta, float *g_pm,
                                    float *pooled, unsigned char *arg, float *ystar, float *mean, float *invstd,
                                    float *var_unbiased, double *gd, float *running_mean, float *running_var,
                                    long long *num_batches_tracked, int phase, double *sums, void *workspace,
                                    size_t workspace_bytes, void *stream);
/* dg_cm (b,cout,n) = gradient w.r.t. G (feed it to amc3d_pointwise_conv_backward for df and dW_f); dw_dp (cout,3) at a row
 * stride of lddw floats (>= 3): dw_dp = dW, lddw = cin + 3 writes columns 0-2 of the layer's weight gradient
 * (amc3d_pointwise_conv_backward_strided writes columns 3 onwards), no join; dgamma, dbeta (cout).
 * rev_start == NULL: the pooled gradient is scattered into Q with cout * npoints float atomics (not x nsample); workspace:
 * amc3d_local_aggregation_workspace_bytes.
 * With rev_start (b*n + 1) / rev_edge (b*npoints*nsample), the reverse lists of idx (amc3d_group_csr; rev_edge is then
 * required), there are no float atomics (deterministic mode).  Only the scatter into Q changes:
 * Q[b,j,c] = the sum, over the positions (m,k) of j's list in list order (ascending m*nsample + k), of dq[b,c,m] where
 * arg[b,c,m] == k -- dq the ReLU-masked pooled gradient; of the several k at which a padded ball-query row holds j only the
 * one that equals arg carries it -- by sequential fp32 __fadd_rn from +0.0f (the summation order stated at
 * amc3d_three_interpolate_grad_csr).  The five per-channel fp64 partial sums, the finalize / apply passes and both
 * SyncBatchNorm phases are those of the atomic form.  Workspace: amc3d_local_aggregation_csr_workspace_bytes (the atomic
 * form's plus the point-major (b,npoints,cout) copies of dq and arg that the gather reads). */
size_t amc3d_local_aggregation_csr_workspace_bytes(int b, int cout, int n, int npoints);
/* byte offset of Q (b,n,cout) fp32 in the workspace after either backward form (phase 0 or 1): what the order above is checked on */
size_t amc3d_local_aggregation_workspace_q_offset(int b, int cout, int n, int npoints);
int amc3d_local_aggregation_backward(int b, int cout, int n, int npoints, int nsample, int relu, const float *dpooled,
                                     const float *ystar, const unsigned char *arg, const float *g_pm, const int *idx,
                                     const float *dp, const float *w_dp, long ldw, const void *moments, const double *gd,
                                     const float *mean, const float *invstd, const float *gamma, const float *beta,
                                     const int *rev_start, const int *rev_edge, float *dg_cm, float *dw_dp, long lddw,
                                     float *dgamma, float *dbeta, int phase, double *dsums, const double *count,
                                     void *workspace, size_t workspace_bytes, void *stream);
/* how many partial records per channel each producer leaves for the finalize kernels at this shape (a fixed function of the
 * shape): counts[0] the forward statistics, [1] the pooled layer's backward scatter, [2] the atomic collapse of
 * amc3d_grouped_conv_bn_backward, [3] its reverse-list collapse.  counts: 4 ints on the host. */
int amc3d_local_aggregation_partial_counts(int b, int cout, int n, int npoints, int nsample, int *counts);
/* centroids per wave of the forward's max-pool launch at this shape: 8, or 4, 2, 1 where 8 would leave the grid below 1024
 * workgroups (a workgroup of four waves pools 4 times as many).  The launch itself uses this rule.  -1: not a shape of the layer. */
int amc3d_local_aggregation_pool_centroids(int b, int cout, int npoints);

/* ---- the same three products in bf16 compute / fp32 accumulate (mixed precision: main_AA.py:389-394 wraps model and
 * criterion in autocast; BASELINE config 5).  Tensors stay fp32 in memory; operands are rounded to bf16 as they are
 * staged, multiplied on v_mfma_f32_32x32x16_bf16 and accumulated in fp32 (csrc/gemm_bf16.hip). */
int amc3d_pointwise_conv_forward_bf16(int b, int cin, int cout, long P, const float *x, const float *weight,
                                      const float *bias, float *y, void *stream);
size_t amc3d_pointwise_conv_workspace_bytes_bf16(int b, int cin, int cout, long P);
int amc3d_pointwise_conv_backward_bf16(int b, int cin, int cout, long P, const float *x, const float *weight,
                                       const float *dy, float *dx, float *dweight, void *workspace,
                                       size_t workspace_bytes, void *stream);

/* ---- first layer of a multi-layer SetAbstraction MLP (PointNeXt-S, sa_layers = 2; pointnext_AA.py:104-127, 164-166):
 * the same convolve-before-gather conv + BatchNorm [+ ReLU], with the activation x1 (b,cout,npoints,32) materialised for
 * the layers that follow.  Supported: nsample == 32, cout in {8,16,32} or a multiple of 64.
 * forward: the arguments, the two layouts of G (g_cm == NULL: g_pm holds the rows and is an input), the row strides and the
 * SyncBatchNorm phases of amc3d_local_aggregation_forward, with x1 in place of pooled / arg / ystar: statistics from the
 * moments, one gather + write pass (training == 0 with g_cm == NULL launches the expand kernel alone).  Workspace:
 * amc3d_local_aggregation_workspace_bytes.
 * backward, from dx1, in one of two forms; dg_cm then goes to amc3d_pointwise_conv_backward.
 * rev_start == NULL: ONE pass masks the ReLU, scatters into the source points (row-contiguous float atomics) and accumulates
 * BatchNorm's two sums and the dp weight gradient.  It needs idx; dx1 (b,cout,npoints,nsample) is channel-major
 * (dx1_position_major must be 0) and rev_dp must be NULL.  Workspace: amc3d_local_aggregation_workspace_bytes.
 * With the reverse lists rev_start / rev_edge of amc3d_group_csr (below) the same sums are a gather over the lists: no
 * atomics, deterministic.  idx may be NULL.  dx1 is transposed to position-major rows in the workspace first, or, with
 * dx1_position_major, is already (b,npoints,nsample,cout), 16-byte aligned (amc3d_sa_tail_backward writes it that way) and is
 * read in place.  rev_dp: the stream of amc3d_group_csr_dp, or NULL.  Workspace: amc3d_grouped_conv_bn_csr_workspace_bytes. */
int amc3d_grouped_conv_bn_supported(int cout, int nsample);
int amc3d_grouped_conv_bn_forward(int b, int cout, int n, int npoints, int nsample, int training, int relu, float eps,
                                  float momentum, const float *g_cm, const int *idx, const float *dp, const float *w_dp,
                                  long ldw, const void *moments, const float *gamma, const float *beta, float *g_pm,
                                  float *x1, float *mean, float *invstd, float *var_unbiased, double *gd,
                                  float *running_mean, float *running_var, long long *num_batches_tracked, int phase,
                                  double *sums, void *workspace, size_t workspace_bytes, void *stream);
size_t amc3d_grouped_conv_bn_csr_workspace_bytes(int b, int cout, int n, int npoints, int nsample);
int amc3d_grouped_conv_bn_backward(int b, int cout, int n, int npoints, int nsample, int relu, const float *dx1,
                                   int dx1_position_major, const float *g_pm, const int *idx, const int *rev_start,
                                   const int *rev_edge, const float *rev_dp, const float *dp, const float *w_dp, long ldw,
                                   const void *moments, const double *gd, const float *mean, const float *invstd,
                                   const float *gamma, const float *beta, float *dg_cm, float *dw_dp, long lddw,
                                   float *dgamma, float *dbeta, int phase, double *dsums, const double *count,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* ---- reverse adjacency of a neighbourhood query: gathers instead of float atomics in backward (csrc/csr.hip) ---------
 * The reference's grouping backward scatters with atomicAdd (group_points_gpu.cu:34-51).  The edges depend on coordinates
 * only: amc3d_group_csr sorts them once by target (stable radix sort), after which every source point sums its incoming
 * positions in list order -- deterministic, no atomics.  rev_start (b*n + 1) int32, rev_edge (b*npoints*nsample) int32:
 * rev_edge[rev_start[b*n + j] .. rev_start[b*n + j + 1]) = positions p = m*nsample + k of batch b with idx[b,m,k] == j. */
size_t amc3d_group_csr_workspace_bytes(int b, int npoints, int nsample);
int amc3d_group_csr(int b, int n, int npoints, int nsample, const int *idx, int *rev_start, int *rev_edge, void *workspace,
                    size_t workspace_bytes, void *stream);
/* rev_dp (b*npoints*nsample, 4) fp32, 16-byte aligned: per edge of the lists, in list order, the relative position
 * dp[b, :, p] of its position p and p itself (its int32 bits in the fourth float): what the gather of
 * amc3d_grouped_conv_bn_backward reads as one 16-byte stream instead of an edge id and three scattered floats.
 * Coordinates only: part of the plan. */
int amc3d_group_csr_dp(int b, int npoints, int nsample, const int *rev_edge, const float *dp, float *rev_dp, void *stream);
/* the moments buffer of amc3d_group_moments from the lists (no scattered atomics) */
int amc3d_group_moments_csr(int b, int n, int npoints, int nsample, const int *rev_start, const int *rev_edge,
                            const float *dp, void *moments, size_t moments_bytes, void *stream);

/* ---- tail of a two-layer SetAbstraction block, recomputed instead of materialised -----------------------------
 * BN1 -> ReLU -> Conv2d 1x1 (C1 -> C2) -> BN2 [-> ReLU] -> max over the K = 32 neighbours
 * (openpoints/models/backbone/pointnext_AA.py:104-127, 164-166) from the first conv's raw output y1 (B,C1,M,32),
 * without ever writing the (B,C2,M,32) activation: every pass re-creates it tile by tile on the MFMA.
 * Supported: K == 32, even C1 <= 64, C2 <= 128, y1 16-byte aligned.  BN1's statistics (mean1, invstd1) come from
 * amc3d_bn_stats(y1); its backward (from dx1) is amc3d_bn_backward(x = y1, dy = dx1, relu = 1). */
int amc3d_sa_tail_supported(int C1, int C2, int K);
int amc3d_sa_tail_pays(int C1, int C2);  /* 1 where the fused tail is faster than the layer-by-layer kernels (HBM-bound widths) */
size_t amc3d_sa_tail_workspace_bytes(int B, int C1, int C2, int M);
/* pooled (B,C2,M); mean2 / invstd2 / var_unbiased2 (C2) are BN2's batch statistics; running buffers of BN2 are
 * updated when given (momentum2 < 0: left to the caller).  One recomputation pass: it emits the statistics and the
 * raw max / min over the neighbours, from which the pooled output follows because BN's affine and the ReLU are
 * monotone in fp32; the backward finds the arg-max itself (first neighbour attaining the maximum, torch.max's rule) */
int amc3d_sa_tail_forward(int B, int C1, int C2, int M, int K, const float *y1, const float *mean1,
                          const float *invstd1, const float *gamma1, const float *beta1, const float *w2,
                          const float *gamma2, const float *beta2, float eps2, float momentum2, int relu2,
                          float *pooled, float *mean2, float *invstd2, float *var_unbiased2,
                          float *running_mean2, float *running_var2, long long *num_batches_tracked2,
                          float *zext_out, unsigned char *arg_out, void *workspace, size_t workspace_bytes, void *stream);
/* zext_out (B,C2,M) fp32 and arg_out (B,C2,M) bytes -- both or neither: per (b, c2, centroid) the raw extreme of conv2's output
 * over the 32 neighbours that BN2 + max-pool select (the maximum for gamma2 > 0, the minimum for gamma2 < 0, neighbour 0's
 * value for gamma2 == 0, where all 32 normalised values equal beta2) and the first neighbour attaining it (torch.max's rule on the raw values).  Handed to amc3d_sa_tail_backward they replace its two
 * recomputation passes by the algebraic form: q is sparse (one neighbour per pooled element) and BatchNorm's backward adds
 * terms affine in z = W2 x1, so  dx1 = W2^T Dq q - (W2^T E W2) x1 - c  and  dW2 = Dq q x1^T - E W2 (x1 x1^T) - t (x1 1)^T
 * (csrc/sa_tail.hip): one pass over x1 with a C1 x C1 product and the Gram matrix on the MFMA and C2 rank-1 terms per centroid. */
/* dx1 (B,C1,M,32) = gradient w.r.t. relu(bn1(y1)) -- written as (B,M,32,C1) rows when dx1_position_major
 * (C1 % 4 == 0), the layout amc3d_grouped_conv_bn_backward gathers from; dw2 (C2,C1) deterministic; dgamma2, dbeta2 (C2);
 * arg_out (B,C2,M) bytes or NULL: the neighbour each pooled gradient was routed to (what torch.max returns as
 * indices, pointnext_AA.py:166) -- the parity tests hold the routing fixed with it */
int amc3d_sa_tail_backward(int B, int C1, int C2, int M, int K, const float *y1, const float *mean1,
                           const float *invstd1, const float *gamma1, const float *beta1, const float *w2,
                           const float *mean2, const float *invstd2, const float *gamma2, const float *beta2,
                           int relu2, const float *dpooled, const float *zext /* of the forward, or NULL */,
                           const unsigned char *arg_ext /* of the forward, or NULL */, float *dx1, int dx1_position_major,
                           float *dw2, float *dgamma2, float *dbeta2, unsigned char *arg_out, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---- training-mode BatchNorm fused with ReLU / neighbourhood max-pool ---------------------------
 * The reference runs nn.Conv -> nn.BatchNorm -> nn.ReLU(inplace) [-> torch.max over the neighbours]
 * as separate torch layers (openpoints/models/layers/conv.py:24-102, backbone/pointnext_AA.py:166).
 * Tensors are the reference's channel-major (B, C, L); statistics per channel over (B, L). */
size_t amc3d_bn_workspace_bytes(int C);  /* for amc3d_bn_stats; amc3d_bn_backward needs this + 8*C bytes */

/* mean (C), invstd = 1/sqrt(biased var + eps) (C), var_unbiased (C, for the running estimate) */
int amc3d_bn_stats(int B, int C, long L, float eps, const float *x, float *mean, float *invstd,
                   float *var_unbiased, void *workspace, size_t workspace_bytes, void *stream);
/* Training-mode BatchNorm forward in two launches (statistics; normalise [+ReLU] [+max over K neighbours]):
 * K == 0: y (B,C,L);  K > 0: L = M*K, y (B,C,M) and arg (B,C,M) bytes.  Writes mean, invstd, var_unbiased (C)
 * for the backward pass and, when running_mean != NULL, updates nn.BatchNorm's buffers
 * (torch/nn/modules/batchnorm.py; momentum < 0 = momentum None, the cumulative average). */
int amc3d_bn_forward(int B, int C, long L, int K, int relu, float eps, float momentum, const float *x,
                     const float *gamma, const float *beta, float *y, unsigned char *arg, float *mean,
                     float *invstd, float *var_unbiased, float *running_mean, float *running_var,
                     long long *num_batches_tracked, void *workspace, size_t workspace_bytes, void *stream);
/* nn.BatchNorm's training-mode bookkeeping in one launch: num_batches_tracked += 1 and the moving average of
 * mean / unbiased variance (torch/nn/modules/batchnorm.py); momentum < 0 stands for momentum=None (cumulative) */
int amc3d_bn_update_running(int C, float momentum, const float *mean, const float *var_unbiased,
                            float *running_mean, float *running_var, long long *num_batches_tracked, void *stream);

/* y (B,C,L) = [relu](((x - mean) * invstd) * gamma + beta) */
int amc3d_bn_act(int B, int C, long L, int relu, const float *x, const float *mean, const float *invstd,
                 const float *gamma, const float *beta, float *y, void *stream);

/* y (B,C,M) = max over K of [relu](bn(x (B,C,M,K))); arg (B,C,M) = first arg-max (bytes), K <= 255 */
int amc3d_bn_max(int B, int C, int M, int K, int relu, const float *x, const float *mean, const float *invstd,
                 const float *gamma, const float *beta, float *y, unsigned char *arg, void *stream);

/* backward of amc3d_bn_act (arg = NULL, K = 1, dy (B,C,L)) or amc3d_bn_max (arg given, dy (B,C,L/K)) under
 * batch statistics: dx (B,C,L), dgamma (C), dbeta (C) */
int amc3d_bn_backward(int B, int C, long L, int K, int relu, const float *x, const float *dy,
                      const unsigned char *arg, const float *mean, const float *invstd, const float *gamma,
                      const float *beta, float *dx, float *dgamma, float *dbeta, void *workspace,
                      size_t workspace_bytes, void *stream);

/* ---- the same BatchNorm with statistics over all ranks (torch.nn.SyncBatchNorm: the reference converts every BN
 * layer to it when world_size > 1, examples/segmentation/main_AA.py:146-148, 820).  The per-channel sums leave the
 * library between two launches so that the caller can all-reduce them (RCCL):
 *     forward    amc3d_bn_sums -> all-reduce(sums[2C] ++ count) -> amc3d_bn_forward_synced
 *     backward   amc3d_bn_backward_sums -> all-reduce(dsums[2C]) -> amc3d_bn_backward_synced
 * Element counts are read from device memory: ranks may differ in size, and the sequence can be graph-captured. */
/* sums (2C doubles) = {sum x, sum x^2} per channel over this rank's (B, L) */
int amc3d_bn_sums(int B, int C, long L, const float *x, double *sums, void *workspace, size_t workspace_bytes,
                  void *stream);
/* amc3d_bn_forward's second launch from global statistics: sums_count = 2C sums, then the global element count */
int amc3d_bn_forward_synced(int B, int C, long L, int K, int relu, float eps, float momentum, const float *x,
                            const double *sums_count, const float *gamma, const float *beta, float *y,
                            unsigned char *arg, float *mean, float *invstd, float *var_unbiased, float *running_mean,
                            float *running_var, long long *num_batches_tracked, void *stream);
/* dsums (2C doubles) = {sum dq, sum dq*xhat} per channel over this rank; dgamma / dbeta (C) = the same, rank-local
 * (as torch's SyncBatchNorm leaves them; the gradient all-reduce averages parameter gradients) */
int amc3d_bn_backward_sums(int B, int C, long L, int K, int relu, const float *x, const float *dy,
                           const unsigned char *arg, const float *mean, const float *invstd, const float *gamma,
                           const float *beta, double *dsums, float *dgamma, float *dbeta, void *workspace,
                           size_t workspace_bytes, void *stream);
/* dx (B,C,L) from the global dsums and the global element count (*count, device memory) */
int amc3d_bn_backward_synced(int B, int C, long L, int K, int relu, const float *x, const float *dy,
                             const unsigned char *arg, const float *mean, const float *invstd, const float *gamma,
                             const float *beta, const double *dsums, const double *count, float *dx, void *stream);

/* ---- tail of an InvResMLP block (openpoints/models/backbone/pointnext_AA.py:296-307): y = relu(batch_norm(x) + res) with
 * batch statistics -- the last Conv1d -> BatchNorm1d of pwconv, `f += identity`, `self.act(f)` -- in the two launches of a
 * plain BatchNorm layer; backward: dres = dy * (y > 0), dx / dgamma / dbeta = BatchNorm backward of that.  x, res, y, dy,
 * dx, dres (B,C,L) fp32; workspace: amc3d_bn_workspace_bytes(C). */
int amc3d_bn_residual_forward(int B, int C, long L, float eps, float momentum, const float *x, const float *res,
                              const float *gamma, const float *beta, float *y, float *mean, float *invstd,
                              float *var_unbiased, float *running_mean, float *running_var,
                              long long *num_batches_tracked, void *workspace, size_t workspace_bytes, void *stream);
int amc3d_bn_residual_backward(int B, int C, long L, const float *x, const float *y, const float *dy, const float *mean,
                               const float *invstd, const float *gamma, const float *beta, float *dx, float *dres,
                               float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream);

/* ---- masked refinement of AMContrast3D++, the DualMasks rule with fusion 'MIN' (openpoints/AMContrast3D/MaskedRefine.py:55-131,
 * called per decoder level by models/backbone/pointnext_MM.py:541-560): points whose predicted ambiguity a lies in
 * [threshold, threshold_max] take the feature row of their least ambiguous neighbour,
 *     out = gamma * (f * ~mask + f_rows[best] * mask) + (1 - gamma) * f,
 * with the reference's two reinterpretations kept (f (B,D,n) viewed as (B*n, D) rows for the gather, the mask (B,1,n) broadcast
 * in the (B,D,n) indexing).  f, out, dout, df (B,D,n) fp32; a (B*n) fp32; nbr (B*n, k) int32 with row stride nbr_stride (self
 * match dropped); outputs kept for the backward: best (B*n) int32, mask (B*n) bytes; count (1) int32 = refined points.
 * Backward: df = (gamma * dout) * ~mask + (1 - gamma) * dout, plus gamma * dout of the masked elements added to row best[r]
 * (float atomics, like torch's index_add). */
size_t amc3d_masked_refine_workspace_ints(int m);
int amc3d_masked_refine_forward(int B, int D, int n, int k, int nbr_stride, const float *f, const float *a, const int *nbr,
                                float threshold, float threshold_max, float gamma, float *out, int *best, unsigned char *mask,
                                int *count, int *workspace, void *stream);
int amc3d_masked_refine_backward(int B, int D, int n, float gamma, const float *dout, const int *best, const unsigned char *mask,
                                 float *df, void *stream);
/* The backward without atomics (deterministic mode).  rev_start (B*n + 1), rev_edge (B*n) = amc3d_group_csr(1, B*n, B*n, 1,
 * best, ...): the rows as one cloud, as the forward sees them.  For element r'*D + d of df: S = the masked elements'
 * __fmul_rn(gamma, dout[r*D + d]) over the rows r of r''s list in list order (ascending r), sequential __fadd_rn from +0.0f
 * (the summation order of amc3d_three_interpolate_grad_csr); df = __fadd_rn(direct term, S).  Writes every element. */
int amc3d_masked_refine_backward_csr(int B, int D, int n, float gamma, const float *dout, const int *best,
                                     const unsigned char *mask, const int *rev_start, const int *rev_edge, float *df,
                                     void *stream);

/* y = sigmoid(batch_norm(x)) with batch statistics -- nn.BatchNorm1d -> nn.Sigmoid of the APM towers of AMContrast3D++
 * (openpoints/AMContrast3D/APM/concatenation.py:20-60) -- in the two launches of a plain BatchNorm layer; backward from the saved
 * output: dq = dy * y (1 - y), then BatchNorm backward.  Layout and workspace as amc3d_bn_forward. */
int amc3d_bn_sigmoid_forward(int B, int C, long L, float eps, float momentum, const float *x, const float *gamma,
                             const float *beta, float *y, float *mean, float *invstd, float *var_unbiased,
                             float *running_mean, float *running_var, long long *num_batches_tracked, void *workspace,
                             size_t workspace_bytes, void *stream);
int amc3d_bn_sigmoid_backward(int B, int C, long L, const float *x, const float *y, const float *dy, const float *mean,
                              const float *invstd, const float *gamma, const float *beta, float *dx, float *dgamma, float *dbeta,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ---- gradient-norm clipping + AdamW over all parameter tensors in two launches ---------------------
 * Replaces  torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm, norm_type=2); optimizer.step()  with
 * torch.optim.AdamW (examples/segmentation/main_AA.py:586-592; optimizer built by openpoints/optim/optim_factory.py:160-230).
 * table: ntensors records in DEVICE memory; block_map: nblocks pairs (tensor index, chunk index) in device memory, one per
 * amc3d_adamw_chunk() elements of every tensor; every record's step (a device float of its own: torch counts steps per
 * parameter) is incremented by the call; partial: nblocks doubles of scratch; total_norm: device float or NULL (the 2-norm of all gradients before clipping, what clip_grad_norm_ returns);
 * max_grad_norm <= 0: no clipping.  The clipped gradient is used for the update, the .grad tensors are left as they are. */
typedef struct {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    float *step;
    long long numel;
    float weight_decay;
    float lr;
} amc3d_adamw_tensor;
int amc3d_adamw_chunk(void);
int amc3d_adamw_step(const void *table, const int *block_map, int nblocks, double beta1, double beta2, float eps,
                     float max_grad_norm, double *partial, float *total_norm, void *stream);

/* ---- training-time augmentation of a batch of cropped clouds (the loader's transform chain, cfgs/s3dis/default.yaml:33-43:
 * ChromaticAutoContrast, PointCloudScaling, PointCloudXYZAlign, PointCloudRotation, PointCloudJitter, ChromaticDropGPU,
 * ChromaticNormalize -- openpoints/transforms/point_transform_cpu.py:192-209, point_transformer_gpu.py:70-89,135-164,216-229,
 * 267-311,373-409 -- which the reference applies per cloud in loader workers).  Two launches for the whole batch.  The random
 * draws are the caller's: params (b,24) floats per cloud = {contrast 0/1, blend, scale[3], rot[9] row-major (pos' = pos @ rot^T),
 * drop 0/1, 9 unused}, noise (b,n,3) standard-normal draws.  pos (b,n,3), color (b,n,3) (0..255, or 0..1: colours are divided by
 * 255 when their maximum exceeds 1, as ChromaticNormalize does) -> pos_out (b,n,3), x_out (b,n,3) = (colour - mean) / std,
 * heights (b,n) = the UNtransformed gravity coordinate (dataset/s3dis/s3dis.py:141-142). */
size_t amc3d_augment_workspace_bytes(int b);
int amc3d_augment_clouds(int b, int n, int gravity_dim, float jitter_sigma, float jitter_clip, const float *pos,
                         const float *color, const float *noise, const float *params, const float *color_mean,
                         const float *color_std, float *pos_out, float *x_out, float *heights, void *workspace,
                         size_t workspace_bytes, void *stream);

/* ---- any chain of the reference's training transforms as one compiled program (amcontrast3d_amd/transforms.py compiles a
 * `datatransforms.train` list; csrc/transforms.hip interprets it).  Clouds are ragged: points concatenated, offsets (b+1)
 * int64 in device memory, no empty cloud.  program: device memory, program_bytes long = {int n_ops, n_phases, stride,
 * gravity_dim, phase_mask[4] (bit 0: position statistics, bit 1: colour statistics)} then max_ops records of 64 bytes {int
 * code, phase (the reduction phase whose statistics the op reads, -1: none), slot (offset into the cloud's row of table),
 * iarg (bit 0: keep float64 / has mean and std; bits 8..: per-point tensor, axis or channel mask); float f[8]; double d[2]}.
 * table (b, stride) doubles: the per-cloud draws, already turned into what the op multiplies or adds (a float32 value is stored
 * exactly).  noise: HOST array of 4 device pointers to the per-point draws ((total,3) float64 for the numpy classes, (total,3)
 * or (total) float32 for the torch classes; unused entries NULL).  flags: bit 0 pos is float64, bit 1 x is ScanNet's [-1, 1]
 * colour and becomes (x + 1) * 127.5 first, bit 2 pos_out is float64.  pos (total,3), x (total,3) fp32 -> pos_out (total,3),
 * x_out (total,3) fp32, heights (total) fp32 or NULL (the gravity coordinate before the chain unless an op sets it).
 * 1 + n_phases launches of one kernel: launch k replays the ops that need phases < k from the input and reduces the state each
 * stream has at its first op of phase k (per-workgroup partials, folded in a fixed order by the next launch: no atomics, the
 * same bits on every run); the last launch writes the outputs.  No intermediate of the batch's size is stored. */
int amc3d_transform_max_ops(void);
int amc3d_transform_max_phases(void);
int amc3d_transform_program_bytes(void);
size_t amc3d_transform_workspace_bytes(int b, long long total, int n_phases);
int amc3d_transform_chain(int b, long long total, int n_phases, const long long *offsets, const void *program, const double *table,
                          const void *const *noise, int flags, const void *pos, const float *x, void *pos_out, float *x_out,
                          float *heights, void *workspace, size_t workspace_bytes, void *stream);

/* ---- ScanNet training input for a batch of RAW rooms (dataset/scannetv2/scannet.py:140-176: colours (feat + 1) * 127.5, the
 * chain RandomRotateZ, RandomScale, ChromaticAutoContrast, RandomDropFeature, NumpyChromaticNormalize -- transforms/
 * point_transform_cpu.py:43-92,192-209,304-332 -- on the whole room, then crop_pc and `heights`).  Rooms are ragged: points
 * concatenated, offsets (b+1) int64.  The random draws are the caller's: params (b,16) doubles per room = {rot[9] row-major
 * (pos' = pos @ rot), scale[3] (scale * mirror), contrast 0/1, w_keep = f32(1 - blend), w_contrast = f32(blend), drop 0/1}.
 * room_stats: stats (b,8) floats = {lo[3], hi[3] of the colours, cmax = max of the colours after contrast and drop (NaN when
 * one is NaN, as numpy's max()), unused} -- three launches, kStatBlocks workgroups per room.
 * transform_rooms: coord (total,3) fp32, feat (total,3) fp32 in [-1, 1] -> pos_out (total,3) DOUBLE (np.dot's dgemm order:
 * fma(p2, R[2,j], fma(p1, R[1,j], p0 * R[0,j])), then * scale[j]), x_out (total,3) fp32 = (colour [/ 255 if cmax > 1] -
 * mean) / std.  One launch.
 * crop_tail: one room (one launch): slot k <- point sel[crop[perm[k]]] (crop / perm NULL: identity) of the room's float64
 * coord (already shifted to its min corner for the voxel grid), minus the cropped cloud's float64 min corner, cast to fp32 ->
 * pos_out (n,3), x_out (n,3), heights (n) = pos_out[:, gravity_dim] (the float32 minimum of that column is exactly 0), y_out
 * (n) int64: the room's slot of the collated batch. */
size_t amc3d_scannet_stats_workspace_bytes(int b);
int amc3d_scannet_room_stats(int b, const long long *offsets, const float *feat, const double *params, float *stats,
                             void *workspace, size_t workspace_bytes, void *stream);
int amc3d_scannet_transform_rooms(int b, long long total, const long long *offsets, const float *coord, const float *feat,
                                  const double *params, const float *stats, const float *color_mean, const float *color_std,
                                  double *pos_out, float *x_out, void *stream);
int amc3d_scannet_crop_tail(int n, int gravity_dim, const double *coord, const float *x, const long long *y, const int *sel,
                            const int *crop, const int *perm, float *pos_out, float *x_out, float *heights, long long *y_out,
                            void *stream);

/* ---- ScanNet validation / whole-room testing (main_AA.py:71-116 `load_data`, :574-611 the sub-cloud loop, :662-671 the vote;
 * dataset/scannetv2/scannet.py:140-176 the val item).  Voxel tables as amc3d_voxelize writes them for a room of npts points.
 * room_parts: p = count.max() sub-clouds of one point per voxel; perm (p,nvox): row i a permutation of the voxel ids (the
 * stand-in for np.random.shuffle) -> parts[i,j] = idx_sort[start[v] + i % count[v]], v = perm[i,j]; where[i,v] = j.  One launch.
 * part_batch: rows of an index matrix idx (rows,n) into coord (npts,3), feat (npts,3) [, label (npts) int64] -> pos (rows,n,3) =
 * coordinate - the row's fp32 minimum corner; colours by mode (0 test: clip((f + 1) / 2, 0, 1); 1 val: (f + 1) * 127.5), / 255
 * when the row's maximum exceeds 1 (NaN propagates: then not), (x - mean) / std; heights (rows,n) = pos[..., gravity_dim];
 * x (rows,Cx,n) channel-major = nseg <= 3 segments in the caller's order, seg_kinds[i] in {0 pos, 1 x, 2 heights}
 * (get_features_by_keys); y (rows,n) int64 when y_out is not NULL.  Two launches through the workspace (8-byte aligned).
 * vote_parts: logits (p,num_classes,nvox) = the stacked model outputs -> voted (npts,num_classes) = the mean over the parts that
 * hold the point (rank r of count c: parts r, r + c, ... < p), summed in ascending part order in fp32 and divided by their
 * number; pred (npts) int64 = the first maximum, a NaN counting as the maximum (torch.argmax).  No atomics: reproducible bits. */
int amc3d_room_parts(int p, int nvox, int npts, const int *start, const int *count, const int *idx_sort, const int *perm,
                     int *parts, int *where, void *stream);
size_t amc3d_part_batch_workspace_bytes(int rows);
int amc3d_part_batch(int rows, int n, int npts, int mode, int gravity_dim, int nseg, const int *seg_kinds, const int *idx,
                     const float *coord, const float *feat, const long long *label, const float *color_mean,
                     const float *color_std, float *pos_out, float *x_out, float *heights, long long *y_out, void *workspace,
                     size_t workspace_bytes, void *stream);
int amc3d_vote_parts(int npts, int p, int num_classes, int nvox, const float *logits, const int *where, const int *start,
                     const int *count, const int *idx_sort, const int *voxel_idx, float *voted, long long *pred, void *stream);

/* ---- S3DIS validation / whole-room testing (examples/segmentation/main.py:68-113 `load_data`, :559-588 the sub-cloud loop with
 * `val: [PointsToTensor, PointCloudXYZAlign, ChromaticNormalize]`, :605 the nearest-neighbour expansion;
 * dataset/s3dis/s3dis.py:94-144 the val item).  Voxel tables as amc3d_voxelize writes them for a room of npts points.
 * s3dis_part_batch: rows of an index matrix idx (rows,n) into coord (npts,3) and colour (npts,3), both fp32 (coord_f64 = 0) or
 * both fp64 (1), colour raw 0..255 [, label (npts) int64].  mode 0 (test): colour = fl32(clip(f / 255, 0, 1)), q = fl32(c - the
 * row's minimum corner), division, minimum and subtraction in the input's precision; mode 1 (val, fp32 only): colour = f, q = c.
 * heights (rows,n) = q[gravity_dim]; centre (rows,3) = the column sums of q in fp64 in a fixed order (per-chunk partials folded
 * in ascending order, no atomics), divided by n in fp64 and rounded once to fp32, or centre_in (rows,3) when it is not NULL;
 * pos (rows,n,3) = fl32(q - centre), then pos[gravity_dim] -= its row minimum; colours / 255 when the row's maximum exceeds 1
 * (a NaN maximum: not), then (x - mean) / std; x (rows,Cx,n) channel-major = nseg <= 3 segments in the caller's order,
 * seg_kinds[i] in {0 pos, 1 x, 2 heights}; y (rows,n) int64 when y_out is not NULL; centre_out (rows,3) always.  An index outside
 * [0, npts) is never read: its slot is left unwritten and it takes no part in the statistics (the centre is the mean of the
 * others).  NaN stays inside its own row.  Three launches through the workspace (8-byte aligned), two when centre_in is given.
 * room_representatives (test_mode nearest_neighbor): parts[j] = idx_sort[start[v] + rnd[v] % count[v]], v = perm[j], perm a
 * permutation of the voxel ids, rnd (nvox) >= 0; where[v] = j; a perm entry that is no voxel id, a negative rnd or an empty voxel gives parts[j] = -1
 * (and a bad perm entry leaves its where slot unwritten): nothing is read through them.  One launch.
 * expand_parts: logits (num_classes,nvox) of that one sub-cloud -> voted (npts,num_classes): every room point takes the logits
 * of its voxel's representative; pred (npts) int64 = the first maximum, a NaN counting as the maximum (torch.argmax). */
size_t amc3d_s3dis_part_batch_workspace_bytes(int rows);
int amc3d_s3dis_part_batch(int rows, int n, int npts, int mode, int coord_f64, int gravity_dim, int nseg, const int *seg_kinds,
                           const int *idx, const void *coord, const void *colour, const long long *label, const float *color_mean,
                           const float *color_std, const float *centre_in, float *pos_out, float *x_out, float *heights,
                           long long *y_out, float *centre_out, void *workspace, size_t workspace_bytes, void *stream);
int amc3d_room_representatives(int nvox, int npts, const int *start, const int *count, const int *idx_sort, const int *rnd,
                               const int *perm, int *parts, int *where, void *stream);
int amc3d_expand_parts(int npts, int num_classes, int nvox, const float *logits, const int *where, const int *idx_sort,
                       const int *voxel_idx, float *voted, long long *pred, void *stream);

/* ---- S3DIS training input for a batch of RAW rooms (dataset/s3dis/s3dis.py:122-144 with presample=False: the room cast to fp32,
 * xyz -= min, then crop_pc, dataset/data_util.py:146-174; the transform chain that follows is amc3d_augment_clouds).  Rooms are
 * ragged: raw (rows,7) = {xyz, rgb 0..255, label}, fp32 (raw_f64 = 0) or fp64 (1); room r is rows [src[r], src[r] + its size)
 * of raw and points [offsets[r], offsets[r+1]) of the batch (src (rooms), offsets (rooms+1) int64, device memory; total =
 * offsets[rooms] < 2^31, no empty room).  Everything is exact arithmetic: the results equal amc3d_voxelize / amc3d_voxel_select /
 * amc3d_crop_nearest run room by room, bit for bit.
 * voxelize_rooms: corner (rooms,3) = the fp32 minimum of fl32(xyz); coord (total,3) = fl32(xyz) - corner; key (total) as
 * amc3d_voxelize; idx_sort (total) = batch point indices ordered by (room, key), stable (two device-wide radix sorts: 64 key
 * bits, then the room-id bits); voxels numbered through the batch, a room boundary always starting one: start (total+1),
 * count (total; written for the voxels only), vbase (rooms+1) = first voxel of every room, vbase[rooms] = their number,
 * cmax (rooms) = count.max() per room.  Nothing is read back.
 * select_crop (nvox = vbase[rooms], read back by the caller): sel (nvox) = idx_sort[start[v] + rnd[v] % count[v]], where
 * rnd[v] < 0 or rnd NULL takes (int)(rnd_u[v] * cmax[room]); with any_crop, for every room with at least voxel_max voxels d2
 * (nvox) = ((dx^2 + dy^2) + dz^2) in fp32 from its representative number init[r] (init[r] < 0 or init NULL:
 * min((int)(init_u[r] * its voxel count), that - 1)), and order (nvox) = voxel numbers sorted by (room, d2 bits), stable (one
 * device-wide radix sort): a room's crop is the first voxel_max entries of its range of order.
 * crop_tail: one launch, one workgroup per room: slot k of room r <- representative c = perm[r,k] (perm (rooms,n) or NULL:
 * identity) of the crop order, or, for a room below voxel_max, voxel c for c below its voxel count and voxel pad[r,c] above
 * (pad (rooms,n), only those slots read); pos_out (rooms,n,3) = coord minus the fp32 min corner of the room's n slots,
 * colour_out (rooms,n,3) = fl32(rgb), y_out (rooms,n) int64 = the label. */
size_t amc3d_s3dis_voxelize_workspace_bytes(int rooms, long long total);
int amc3d_s3dis_voxelize_rooms(int rooms, long long total, int raw_f64, const void *raw, const long long *src,
                               const long long *offsets, double voxel_size, float *coord, unsigned long long *key,
                               int *idx_sort, int *start, int *count, int *vbase, int *cmax, float *corner, void *workspace,
                               size_t workspace_bytes, void *stream);
size_t amc3d_s3dis_crop_workspace_bytes(int nvox);
int amc3d_s3dis_select_crop(int rooms, int nvox, int voxel_max, int any_crop, const float *coord, const int *idx_sort,
                            const int *start, const int *count, const int *vbase, const int *cmax, const int *rnd,
                            const double *rnd_u, const int *init, const double *init_u, int *sel, float *d2, int *order,
                            void *workspace, size_t workspace_bytes, void *stream);
int amc3d_s3dis_crop_tail(int rooms, int n, int voxel_max, int raw_f64, const void *raw, const long long *src,
                          const long long *offsets, const float *coord, const int *vbase, const int *sel, const int *order,
                          const int *pad, const int *perm, float *pos_out, float *colour_out, long long *y_out, void *stream);

/* ---- ScanNet training input for a batch of rooms, the part after the transform chain (dataset/scannetv2/scannet.py:166-176:
 * crop_pc in float64, dataset/data_util.py:146-174, then heights).  The float64 sibling of the S3DIS block above.  Rooms are
 * ragged: pos (total,3) double, x (total,3) fp32 and y (total) int64 as amc3d_scannet_transform_rooms leaves them for the
 * concatenated rooms; room r is points [offsets[r], offsets[r+1]) (offsets (rooms+1) int64, device memory; total =
 * offsets[rooms] < 2^31, no empty room).  Everything is exact arithmetic: the results equal amc3d_voxelize_f64 /
 * amc3d_voxel_select / amc3d_crop_nearest_f64 / amc3d_scannet_crop_tail run room by room, bit for bit.
 * voxelize_rooms: corner (rooms,3) = the fp64 minimum of pos; coord (total,3) = pos - corner; key (total) as
 * amc3d_voxelize_f64; idx_sort (total) = batch point indices ordered by (room, key), stable (two device-wide radix sorts: 64 key
 * bits, then the room-id bits; one room: the first only); voxels numbered through the batch, a room boundary always starting
 * one: start (total+1), count (total; written for the voxels only), vbase (rooms+1) = first voxel of every room,
 * vbase[rooms] = their number, cmax (rooms) = count.max() per room.  Nothing is read back.
 * select_crop (nvox = vbase[rooms], read back by the caller): sel (nvox) = idx_sort[start[v] + rnd[v] % count[v]], where
 * rnd[v] < 0 or rnd NULL takes (int)(rnd_u[v] * cmax[room]); with any_crop, for every room with at least voxel_max voxels d2
 * (nvox) = ((dx^2 + dy^2) + dz^2) in fp64 from its representative number init[r] (init[r] < 0 or init NULL:
 * min((int)(init_u[r] * its voxel count), that - 1)), and order (nvox) = voxel numbers sorted by (room, the 64 bits of d2),
 * stable (the composite key is wider than 64 bits: one device-wide radix sort over the d2 bits, then the stable pass over the
 * room-id bits): a room's crop is the first voxel_max entries of its range of order.  d2 is 0 in the other rooms.
 * crop_tail_rooms: two launches for the batch, several workgroups per room (partial minima, then fold and gather): slot k of
 * room r <- representative c = perm[r,k] (perm (rooms,n) or NULL: identity) of the crop order, or, for a room below voxel_max,
 * voxel c for c below its voxel count and voxel pad[r,c] above (pad (rooms,n), only those slots read); pos_out (rooms,n,3) =
 * fl32(coord - the fp64 min corner of the room's n slots), x_out (rooms,n,3) = x, heights (rooms,n) = pos_out[..., gravity_dim],
 * y_out (rooms,n) int64 = y. */
size_t amc3d_scannet_voxelize_workspace_bytes(int rooms, long long total);
int amc3d_scannet_voxelize_rooms(int rooms, long long total, const double *pos, const long long *offsets, double voxel_size,
                                 double *coord, unsigned long long *key, int *idx_sort, int *start, int *count, int *vbase,
                                 int *cmax, double *corner, void *workspace, size_t workspace_bytes, void *stream);
size_t amc3d_scannet_crop_workspace_bytes(int nvox);
int amc3d_scannet_select_crop(int rooms, int nvox, int voxel_max, int any_crop, const double *coord, const int *idx_sort,
                              const int *start, const int *count, const int *vbase, const int *cmax, const int *rnd,
                              const double *rnd_u, const int *init, const double *init_u, int *sel, double *d2, int *order,
                              void *workspace, size_t workspace_bytes, void *stream);
size_t amc3d_scannet_crop_tail_workspace_bytes(int rooms);
int amc3d_scannet_crop_tail_rooms(int rooms, int n, int voxel_max, int gravity_dim, const double *coord, const float *x,
                                  const long long *y, const int *vbase, const int *sel, const int *order, const int *pad,
                                  const int *perm, float *pos_out, float *x_out, float *heights, long long *y_out,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ---- S3DISSphere: spheres cut out of whole voxel-subsampled Areas, centres picked by a running potential
 * (dataset/s3dis/s3dis_sphere.py:214-247 the schedule, :288-347 the item; csrc/sphere.hip).  The sub-clouds are concatenated:
 * points (total,3) fp32, colours (total,3) fp32, labels (total) int64, cloud c = points [cloud_off[c], cloud_off[c+1])
 * (cloud_off (clouds+1) int32, device memory, no empty cloud, total < 2^31); n_max = the largest cloud's size.  point indices
 * are cloud-local.  potentials (total) fp64; blk_val / blk_idx / touched (ceil(total / 1024)): the first minimum of every 1024
 * consecutive potentials (value, global index) and a mark "stale", all three written by sphere_minima.
 * The radius query of a centre (cloud, point, noise (3) fp64): pick = points[point] + noise in fp64, as the reference forms it
 * from the KD-tree's float64 copy of the coordinates (centre (.,3) fp64, written); d2 = ((dx*dx + dy*dy) + dz*dz) in fp64, no
 * contraction, as sklearn's KDTree evaluates it; the points with
 * d2 <= radius*radius in ascending (d2, point) order -- equal distances in ascending point order, which sklearn leaves
 * unspecified (one stable device-wide radix sort of n_max pairs).  cur = their number, count = min(cur, num_points), order
 * (.,num_points) = the first num_points of them, -1 beyond.
 * sphere_schedule, per step s: cloud = argmin over the clouds' minima, point = argmin of its potentials, first minimum in both
 * (cloud_ind[s], point_ind[s], written); the query with noise[s]; potentials[q] += t for the count listed points, t =
 * (1 - d32 / r^2)^2 and 0 where d32 > r^2, d32 = ((x*x + y*y) + z*z) in fp32 of the fp64 differences point - pick rounded to
 * fp32, and everything after it in fp64 (numpy >= 2: np.square(python float) is a float64 scalar and promotes); then the stale table entries of that cloud.
 * Points of one sphere are distinct: no atomics, the same bits on every run.  Five launches per step counting the sort as
 * one; nb_max = the most table entries one cloud spans.  order may be NULL.  An empty sphere (cur = 0) updates nothing.
 * sphere_query: the query alone for given centres (three launches per sphere counting the sort as one).
 * sphere_tail, one launch for all spheres: slot k < count takes list entry perm[k] (perm (spheres,num_points), its first count
 * entries a permutation of them; NULL: identity), slot k >= count entry perm[pad[k]] (pad (spheres,num_points), only those
 * slots read; negative or NULL: (int)(pad_u[k] * count)); input_inds (int64, cloud-local), mask (int32, 1 below count), pos =
 * fl32(point - pick), the difference in fp64, x = colours, y = label, heights = the point's own gravity coordinate.  An empty sphere gives the
 * centre's point in every slot and mask 0 (the reference raises there).  Draws out of range are clamped.
 * No entry allocates, synchronises or reads back, and no memset node appears under capture. */
size_t amc3d_sphere_workspace_bytes(int n_max);
int amc3d_sphere_minima(int total, const double *potentials, double *blk_val, int *blk_idx, int *touched, void *stream);
int amc3d_sphere_schedule(int clouds, int total, int n_max, int nb_max, int steps, int num_points, double radius,
                          const float *points, const int *cloud_off, double *potentials, double *blk_val, int *blk_idx,
                          int *touched, const double *noise, int *cloud_ind, int *point_ind, double *centre, int *order,
                          int *cur, int *count, void *workspace, size_t workspace_bytes, void *stream);
int amc3d_sphere_query(int clouds, int total, int n_max, int spheres, int num_points, double radius, const float *points,
                       const int *cloud_off, const int *cloud_ind, const int *point_ind, const double *noise, double *centre,
                       int *order, int *cur, int *count, void *workspace, size_t workspace_bytes, void *stream);
int amc3d_sphere_tail(int clouds, int spheres, int num_points, int gravity_dim, const float *points, const float *colours,
                      const long long *labels, const int *cloud_off, const int *cloud_ind, const int *point_ind,
                      const double *centre, const int *order, const int *count, const int *perm, const int *pad,
                      const double *pad_u, long long *input_inds, int *mask, float *pos, float *x, long long *y,
                      float *heights, void *stream);

/* ---- separable neighbourhood aggregation (ASSA, models/layers/local_aggregation.py:127-131) ----------------------
 * out[b, d*c + ch, m] = red over k of dp[b,d,m,k] * f[b,ch,idx[b,m,k]], d in 0..2, without the (b,c,npoints,nsample) and
 * (b,3c,npoints,nsample) tensors of the reference's expand / multiply / reduce.  reduction: 0 mean, 1 sum, 2 max.
 * f_pm (b,n,c): the POINT-major features (amc3d_transpose_cn), idx (b,npoints,nsample) int32 into the n support points,
 * dp (b,3,npoints,nsample); out (b,3c,npoints), d-major as the reference's view lays it out.  nsample <= 255.
 * ARITHMETIC (part of the contract): every product is one __fmul_rn; sum adds them by sequential __fadd_rn in ascending k
 * from +0.0f; mean is that sum through one __fdiv_rn by (float)nsample; max keeps the FIRST maximum in k (a later product
 * replaces the kept one only when it compares greater, or when it is the first NaN: NaN propagates as in torch.max) and
 * writes its k to arg_pm (b,npoints,3c) bytes, point-major
 * (required for max, ignored otherwise).  An index outside [0,n) is clamped into it.  No workspace.
 * Backward, to f only: g_pm (b,npoints,3c) is the POINT-major gradient of out, df_pm (b,n,c) the point-major gradient of f.
 * The term of edge (m,k) for channel ch, with s = __fdiv_rn(1, nsample) for mean and 1 otherwise:
 *   mean, sum: __fmul_rn(s, (dp0*g[m,0*c+ch] + dp1*g[m,1*c+ch]) + dp2*g[m,2*c+ch])   (products and sums rounded one by one)
 *   max:       the same sum with the product of d replaced by +0.0f unless arg_pm[b,m,d*c+ch] == k, s = 1.
 * amc3d_assa_aggregate_backward zero-fills df_pm itself and scatters the terms with float atomics (one row segment of c
 * floats per edge; max: only edges some d selected); an index outside [0,n) is skipped.
 * amc3d_assa_aggregate_backward_csr gathers over the reverse lists rev_start (b*n + 1) / rev_edge (b*npoints*nsample) of
 * amc3d_group_csr(b, n, npoints, nsample, idx, ...) under the SUMMATION ORDER stated at
 * amc3d_three_interpolate_grad_csr (list order, sequential __fadd_rn from +0.0f) and writes every element of df_pm:
 * exactly +0.0f for a support point nobody gathers.  Neither allocates, synchronises or reads back. */
int amc3d_assa_aggregate_forward(int b, int c, int n, int npoints, int nsample, int reduction, const float *f_pm,
                                 const int *idx, const float *dp, float *out, unsigned char *arg_pm, void *stream);
int amc3d_assa_aggregate_backward(int b, int c, int n, int npoints, int nsample, int reduction, const float *g_pm,
                                  const int *idx, const float *dp, const unsigned char *arg_pm, float *df_pm, void *stream);
int amc3d_assa_aggregate_backward_csr(int b, int c, int n, int npoints, int nsample, int reduction, const float *g_pm,
                                      const float *dp, const unsigned char *arg_pm, const int *rev_start,
                                      const int *rev_edge, float *df_pm, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AMC3D_H */
