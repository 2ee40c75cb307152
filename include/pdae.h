/*
 * pdae.h -- C ABI of the MI355X-native Point-DAE hot path (libpdae_hip.so).
 *
 * This is the drop-in boundary for the pretraining step's native operators.
 * The reference (YBZh/Point-DAE) reaches its CUDA kernels through pybind11
 * torch extensions; every entry below names the reference host function it
 * replaces (file:line under the reference tree) and keeps that function's
 * argument meaning.  Differences that hold for every entry:
 *
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers
 *     to contiguous row-major buffers owned by the caller.  Nothing is
 *     allocated, retained or freed by the library.
 *   - every entry takes an explicit stream (a hipStream_t passed as void*);
 *     the reference launches chamfer/emd on the legacy default stream
 *     (chamfer.cu:159, emd_kernel.cu:188) and pointnet2 on torch's current
 *     stream (sampling_gpu.cu:183).  Calls are asynchronous and re-entrant.
 *   - return value: PDAE_OK (0) or a negative pdae_status; the reference
 *     either printf()s (chamfer.cu:166-169) or exit(-1)s (cuda_utils.h:32-41).
 *   - outputs are fully written by the call (the reference relies on
 *     torch::zeros in its host wrappers; here the zero-fill, where the
 *     semantics need one, is part of the call).
 *
 * Arithmetic contract (shared with oracle/pdae_oracle.c): fp32, squared
 * distances evaluated as ((dx*dx + dy*dy) + dz*dz) with every operation
 * rounded (no FMA contraction), indices by the reference's tie rules.
 */
#ifndef PDAE_H
#define PDAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pdae_stream_t; /* hipStream_t */

enum pdae_status {
  PDAE_OK = 0,
  PDAE_ERR_BAD_ARG = -1,     /* null pointer / negative size / unsupported size */
  PDAE_ERR_LAUNCH = -2,      /* hipGetLastError() != hipSuccess after launch    */
  PDAE_ERR_UNSUPPORTED = -3  /* shape outside what the kernels implement         */
};

/* Library identification: returns "pdae-hip gfx950 <abi version>". */
const char* pdae_version(void);
/* Text for the last failing status on this thread (hipGetErrorString or arg). */
const char* pdae_last_error(void);

/* Contexts.  The library's mutable state -- the deterministic-mode workspace, the parked (deferred) reductions, the
 * GEMM arithmetic -- lives in a context; every entry point works on the calling thread's CURRENT context, which is
 * the process default context until the thread sets one (the model of the CUDA / HIP runtime's current device; the
 * reference's extensions keep no state at all, so it has nothing to bind here).  A host that drives several streams
 * from several threads gives each thread its own context (and its own workspaces): nothing is shared between them.
 * One context must not be used by two threads at once.  Everything else the library holds (per-kernel launch
 * attributes set at first use) is immutable after its first write. */
typedef struct pdae_ctx* pdae_ctx_t;
int pdae_ctx_create(pdae_ctx_t* out);
int pdae_ctx_destroy(pdae_ctx_t ctx);          /* not while it is current on the calling thread */
int pdae_ctx_set_current(pdae_ctx_t ctx);      /* NULL: back to the process default context */
pdae_ctx_t pdae_ctx_current(void);             /* NULL when the thread is on the default context */

/* Deterministic mode.  The reference's reductions (cuDNN batch-norm statistics, cuBLAS split-K
 * weight gradients, ATen layer_norm backward: models/PointCAE_transformer.py:37-51, 94-147) and,
 * by default, this library's end in float atomics whose order of arrival varies from launch to
 * launch.  With a device workspace registered here (>= 1 MiB; 64 MiB covers the pretraining step
 * at batch 128) the batch-norm statistics, the embedder's weight / bias gradients, the LayerNorm
 * parameter gradients and the column sums store per-block partials and add them in block order:
 * bit-identical results from run to run and from hipGraph replay to eager launch, for one small
 * extra launch per reduction.  The workspace is shared by all launches of its CONTEXT: one stream at a time per context.
 * workspace == NULL switches the mode off.  A reduction that needs more than `bytes` fails with
 * PDAE_ERR_UNSUPPORTED.  Not covered (LDS float atomics, kept): group_points_grad,
 * three_interpolate_grad and the large-cloud Chamfer gradient of the PointNet++ configuration. */
int pdae_set_deterministic(void* workspace, size_t bytes);
int pdae_deterministic(void);   /* 1 when a workspace is registered */

/* Deferred column reductions.  Between deferred_begin and deferred_flush the LayerNorm backward entries park their
 * per-block parameter-gradient partials in `workspace` instead of finishing with float atomics; deferred_flush adds
 * the partials of all parked calls (up to 48) in block order into their outputs with ONE launch.  The outputs
 * (dgamma, dbeta, dbias) are complete only after the flush: for callers that consume them later, such as the
 * hipGraph-replayed step, whose gather copy follows the whole backward (graph_step.py).  A call that does not fit
 * the workspace simply behaves as usual.  Host-side state: one stream / one thread at a time. */
int pdae_deferred_begin(void* workspace, size_t bytes);
int pdae_deferred_flush(pdae_stream_t stream);
/* rows_wgrad parks its partial-tile reduction in the same window (the dW / db outputs and the workspace of the call
 * must then stay untouched until the flush, which adds the tiles of up to 8 parked launches per reduction launch). */

/* ------------------------------------------------------------------------
 * Farthest point sampling.
 * Replaces furthest_point_sampling_kernel_wrapper(b, n, m, dataset, temp, idxs)
 *   extensions/pointnet2/_ext_src/src/sampling_gpu.cu:178-229 (kernel :72-176),
 *   host alloc sampling.cpp:67-88 (third-party pointnet2_ops twin called from
 *   utils/misc.py:18).
 * dataset (b,n,3) f32 -> idxs (b,m) i32.  idxs[:,0]=0; points with
 * x*x+y*y+z*z <= 1e-3 are never selected; ties resolved as the reference's
 * 512-thread strided scan + lower-tid tree reduce.  The reference's `temp`
 * scratch (b,n) lives in registers here and is not part of the ABI.
 * If `centres` is non-null it receives dataset[idxs] as (b,m,3) f32 (the
 * gather_operation + 2 transposes of utils/misc.py:19 fused).
 */
int pdae_furthest_point_sampling(int b, int n, int m, const float* dataset,
                                 int32_t* idxs, float* centres /*nullable*/,
                                 pdae_stream_t stream);

/* gather_points_kernel_wrapper(b, c, n, npoints, points, idx, out)
 *   sampling_gpu.cu:25-33: out[b,c,j] = points[b,c,idx[b,j]].            */
int pdae_gather_points(int b, int c, int n, int npoints, const float* points,
                       const int32_t* idx, float* out, pdae_stream_t stream);
/* gather_points_grad_kernel_wrapper, sampling_gpu.cu:52-60: scatter-add of
 * grad_out (b,c,npoints) into grad_points (b,c,n); grad_points is zero-filled
 * by this call (sampling.cpp:50-52 does it with torch::zeros).            */
int pdae_gather_points_grad(int b, int c, int n, int npoints,
                            const float* grad_out, const int32_t* idx,
                            float* grad_points, pdae_stream_t stream);
/* The fine-tuning runner's batch preparation behind FPS in one launch (tools/runner_finetune.py:415-420: the host's
 * subset of the FPS order, the gather, train_transforms) with the per-cloud map of datasets/data_transforms.py
 * (PointcloudRotate: A, PointcloudScaleAndTranslate: diagonal A and t):
 *   out[b,n,j] = sum_i raw[b, fps_idx[b, choice[n]], i] * A[b,i,j] + t[b,j]        i, j in 0..2
 * raw (b,p,c) with c >= 3 (only the first three channels are read), fps_idx (b,point_all), choice (npoints) shared by
 * the batch, A (b,3,3) and t (b,3) each nullable, out (b,npoints,3).  A == t == NULL moves the coordinates bit for bit;
 * with a map the sum runs i = 0, 1, 2, then + t, every operation rounded.  An index outside its array is not followed
 * (that point is written as NaN).  c < 3, npoints > point_all and non-positive sizes: PDAE_ERR_BAD_ARG.            */
int pdae_resample_affine(int b, int p, int c, int point_all, int npoints, const float* raw, const int32_t* fps_idx,
                         const int32_t* choice, const float* A /*nullable*/, const float* t /*nullable*/, float* out,
                         pdae_stream_t stream);

/* query_ball_point_kernel_wrapper(b, n, m, radius, nsample, new_xyz, xyz, idx)
 *   ball_query_gpu.cu:49-57 (kernel :12-47), host ball_query.cpp:11-35.
 * idx (b,m,nsample) i32: first nsample indices k (ascending) with d2 < r*r;
 * short lists padded with the first hit; empty ball -> zeros.  n == 0 (xyz
 * may then be NULL) leaves every ball empty.                               */
int pdae_ball_query(int b, int n, int m, float radius, int nsample,
                    const float* new_xyz, const float* xyz, int32_t* idx,
                    pdae_stream_t stream);

/* group_points_kernel_wrapper(b, c, n, npoints, nsample, points, idx, out)
 *   group_points_gpu.cu:33-43: out[b,c,j,k] = points[b,c,idx[b,j,k]].     */
int pdae_group_points(int b, int c, int n, int npoints, int nsample,
                      const float* points, const int32_t* idx, float* out,
                      pdae_stream_t stream);
/* group_points_grad_kernel_wrapper, group_points_gpu.cu:69-78; grad_points
 * (b,c,n) is zero-filled by this call (group_points.cpp:49-51).           */
int pdae_group_points_grad(int b, int c, int n, int npoints, int nsample,
                           const float* grad_out, const int32_t* idx,
                           float* grad_points, pdae_stream_t stream);

/* QueryAndGroup.forward (extensions/pointnet2/pointnet2_utils.py:345-361) in ROW layout, the set-abstraction MLP's input:
 *   out[(b*np + p)*ns + s] = [ xyz[b, idx[b,p,s]] - new_xyz[b,p] | 0 | features[b*N + idx[b,p,s], 0:C] ]  (4 + C floats;
 *   features (B*N, C) rows, nullable with C = 0; C a multiple of 4; the zero column keeps the reduction length of the
 *   row GEMMs a multiple of 4).  One pass instead of grouping_operation x 2 + subtract + cat.
 * sa_group_rows_grad: dfeatures[b*N + j, c] = sum of dout[row, 4 + c] over the rows of cloud b whose idx is j (the
 *   backward of the two grouping_operation calls, group_points_gpu.cu:69-78, for the feature part; coordinates carry no
 *   gradient on this path).  Fully written (no zero-fill needed).  A cloud's rows are ordered by source point with a
 *   counting sort in LDS (integer atomics), then summed per point in registers: no float atomics; the order of a point's
 *   rows -- hence of its fp32 sum -- is the sort's order of arrival.  N <= 4096, 4 (2 N + 1 + np ns) <= 150 KB, C <= 1024. */
int pdae_sa_group_rows(int B, int N, int np, int ns, int C, const float* xyz, const float* new_xyz,
                       const int32_t* idx, const float* features /*nullable*/, float* out, pdae_stream_t stream);
int pdae_sa_group_rows_grad(int B, int N, int np, int ns, int C, const int32_t* idx, const float* dout,
                            float* dfeatures, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * k nearest neighbours.  Replaces KNN_CUDA 0.2 `knn(ref, query, k)` as used
 * through KNN(k, transpose_mode=True)(ref, query) at
 * models/PointCAE_transformer.py:59,76 (third-party wheel, not in the
 * reference tree; semantics restated in oracle/pdae_oracle.c).
 * ref (b,n,3), query (b,g,3) -> idx (b,g,k) int64 ascending by squared
 * distance, earlier index first on ties; dist (b,g,k) f32 = sqrtf(d2),
 * nullable.  Requires 1 <= k <= min(n, 64).
 * If `nbr` is non-null it receives ref[idx] - query as (b,g,k,3) f32, i.e.
 * the flat-index gather + centre subtraction of Group.forward
 * (models/PointCAE_transformer.py:79-85) fused into the same launch.
 */
int pdae_knn(int b, int n, int g, int k, const float* ref, const float* query,
             int64_t* idx, float* dist /*nullable*/, float* nbr /*nullable*/,
             pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Feature propagation (PointNet++ FP modules; segmentation / Point-M2AE heads).
 * Replaces three_nn_kernel_wrapper / three_interpolate_kernel_wrapper /
 *   three_interpolate_grad_kernel_wrapper, extensions/pointnet2/_ext_src/src/
 *   interpolate_gpu.cu:12-146 (Python: pointnet2_utils.py:118-204).
 * three_nn: unknown (b,n,3), known (b,m,3) -> dist2 (b,n,3) SQUARED distances to
 *   the three nearest known points, ascending, idx (b,n,3) i32; strict `<`
 *   insertion as the reference (ties keep the earlier index; fewer than three
 *   known points leave +inf / index 0).  The Python wrapper returns sqrt(dist2).
 * three_interpolate: points (b,c,m), idx (b,n,3), weight (b,n,3) -> out (b,c,n) =
 *   sum_k points[b,c,idx[b,n,k]] * weight[b,n,k].
 * three_interpolate_grad: grad_out (b,c,n) -> grad_points (b,c,m), fully written
 *   (the reference zero-fills and scatters with global atomics).
 */
int pdae_three_nn(int b, int n, int m, const float* unknown, const float* known,
                  float* dist2, int32_t* idx, pdae_stream_t stream);
int pdae_three_interpolate(int b, int c, int m, int n, const float* points,
                           const int32_t* idx, const float* weight, float* out,
                           pdae_stream_t stream);
int pdae_three_interpolate_grad(int b, int c, int n, int m, const float* grad_out,
                                const int32_t* idx, const float* weight,
                                float* grad_points, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * In-forward patch corruption.  Fuses, for PointCAE_transformer.forward
 * (models/PointCAE_transformer.py:680-684):
 *     neighborhood += center; (t_nb, t_c) = corrupt_data(neighborhood, center);
 *     neighborhood -= center;  t_nb -= t_c
 * where corrupt_data (datasets/corrupt_util_tensor.py:706-727) applies 1-3
 * per-sample linear maps ('translate' / 'scale_nonorm' multiply by a 3-vector,
 * :59-116; 'rotate' / 'reflection' / 'shear' right-multiply by a 3x3 matrix,
 * :139-342).  The maps are drawn on the host with the reference's RNG calls and
 * passed as steps (nsteps, b, 10) f32: [kind (0 = multiply, 1 = matrix), then
 * 3 factors or 9 row-major matrix entries].
 * nbr (b,g,k,3) centre-subtracted, center (b,g,3) ->
 * gt_nbr (b,g,k,3) = (nbr + c) - c, t_nbr (b,g,k,3), t_center (b,g,3).
 */
int pdae_patch_affine(int b, int g, int k, int nsteps, const float* nbr,
                      const float* center, const float* steps, float* gt_nbr,
                      float* t_nbr, float* t_center, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Point-M2AE token pyramid: index bookkeeping of the hierarchical grouping.
 * Replaces the tensor chains of Group.forward, models/Point_M2AE_modules.py:239-247 (the flat neighbour index
 *   `idx + arange(B).view(-1,1,1) * num_points` that Group returns next to neighbourhood and centre) and of
 *   H_Encoder.forward, models/Point_M2AE.py:112-117 (multi-scale masking pushed one level down).  FPS and kNN of a
 *   level are pdae_furthest_point_sampling / pdae_knn.
 * flatten_group_index: idx (b, g*k) i64 local indices into clouds of n points -> flat (b*g*k) i64 = idx + cloud*n.
 * mask_propagate: parent_masked (parents) u8, flat_idx (parents*k) i64 into `children` finer tokens ->
 *   child_masked (children) u8, fully written: 1, except 0 at every child of a visible parent -- and at flat child 0
 *   whenever some parent is masked (the reference multiplies the indices of masked parents by 0 and scatters them
 *   too; kept bug-for-bug).
 */
int pdae_flatten_group_index(int b, int n, int gk, const int64_t* idx, int64_t* flat, pdae_stream_t stream);
int pdae_mask_propagate(int parents, int k, int children, const uint8_t* parent_masked, const int64_t* flat_idx,
                        uint8_t* child_masked, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Point-M2AE hierarchical encoder in evaluation mode, forward only (csrc/m2ae.hip; H_Encoder.forward with eval=True,
 * models/Point_M2AE.py:99-180; Token_Embed, models/Point_M2AE_modules.py:169-216; Attention, :269-305).
 * attention_local_forward: qkv (B*T, 3*H*D) rows [3][H][D], centres (B*T, 3) with the padded rows zero, len (B) i32
 *   visible tokens per sample (len[b] <= T) -> o (B*T, H*D) = softmax(q k^T * scale + mask * -100000) v with
 *   mask[b][q][k] = !(q < len[b] && k < len[b]) && (radius == 0 || |centre_q - centre_k| >= radius), evaluated in
 *   the kernel; no (B, T, T) tensor is read or written.  Masked pairs are left out of the softmax, which is the
 *   reference's -100000 in fp32 for every row that keeps a key.  With radius == 0 a padded query row (q >= len[b])
 *   keeps none: its output, which nobody reads, is written as zeros.  D in {16, 32, 64}, 1 <= T <= 512, any T.
 *   No log-sum-exp is kept: there is no backward.
 * m2ae_compact: masked (B, G) u8 -> len (B) = visible tokens per sample, ids (B, G) i32 = their indices in ascending
 *   order, -1 behind them.
 * m2ae_pack: x (B*T_pad, C) / cen (B*T_pad, 3) = the visible tokens / centres of tokens (B*G, C) / centres (B*G, 3) at
 *   the front of each sample, zeros behind them (T_pad >= max len).  m2ae_unpack: rows t < len[b] of x back to rows
 *   ids[b][t] of tokens; other rows of tokens are not touched.  C % 4 == 0.
 * m2ae_group_max: out (P, C) = max over the n consecutive rows of each patch of x (P*n, C).
 * m2ae_gather_max: out (P, C) = max over the k rows idx[p][.] (i64, flat) of x.
 * m2ae_gather_add_relu: out (P*k, C), row (p, j) = relu(x[idx[p][j]] + g[p]).
 * m2ae_embed_tail: tok (R/n, N4) = max over each patch's n rows of relu(F (R, K) Wl (N3, K)^T + gb[patch] (R/n, N3))
 *   W4 (N4, N3)^T, + b4: second_conv of Token_Embed(3 -> C) with the BatchNorm folded into Wl / gb; neither the
 *   (R, N3) nor the (R, N4) product is stored.  n in {4, 8, 16, 32}, K % 8 == 0, K <= 256, N3 % 128 == 0,
 *   N4 % 32 == 0, N4 <= 128.
 */
int pdae_attention_local_forward(int B, int T, int H, int D, float scale, float radius, const float* qkv,
                                 const float* centres, const int32_t* len, float* o, pdae_stream_t stream);
int pdae_m2ae_compact(int B, int G, const uint8_t* masked, int32_t* len, int32_t* ids, pdae_stream_t stream);
int pdae_m2ae_pack(int B, int G, int Tp, int C, const int32_t* ids, const int32_t* len, const float* tokens,
                   const float* centres, float* x, float* cen, pdae_stream_t stream);
int pdae_m2ae_unpack(int B, int G, int Tp, int C, const int32_t* ids, const int32_t* len, const float* x,
                     float* tokens, pdae_stream_t stream);
int pdae_m2ae_group_max(long long P, int n, int C, const float* x, float* out, pdae_stream_t stream);
int pdae_m2ae_gather_max(long long P, int k, int C, const float* x, const int64_t* idx, float* out,
                         pdae_stream_t stream);
int pdae_m2ae_gather_add_relu(long long P, int k, int C, const float* x, const int64_t* idx, const float* g,
                              float* out, pdae_stream_t stream);
int pdae_m2ae_embed_tail(long long R, int n, int K, int N3, int N4, const float* F, const float* Wl, const float* gb,
                         const float* W4, const float* b4, float* tok, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Loader-side corruption on the device.  Replaces corrupt_dropout_local
 *   datasets/corrupt_util.py:590-612, which the reference runs per item in its
 *   DataLoader workers (ShapeNet55Dataset.__getitem__ :90-119).
 * xyz (b,p,3) f32; for cloud i, nclusters[i] <= 8 clusters c = 0..: the seed is
 * the seed_rank[i*8+c]-th surviving point in index order, the sizes[i*8+c]
 * survivors nearest to it (squared distance, ties by lower index) are dropped.
 * alive (b,p) u8 receives 1 for survivors.  The draws are inputs: the host side
 * draws them with the reference's distributions.  p <= 16384.
 */
int pdae_dropout_local(int b, int p, const float* xyz, const int32_t* nclusters,
                       const int32_t* seed_rank, const int32_t* sizes,
                       unsigned char* alive, pdae_stream_t stream);

/* The other loader-side stages (ShapeNet55Dataset.__getitem__ :90-119 = augment_data 'norm' -> random_sample ->
 * corrupt_data -> random_sample); the random draws are inputs (the host side draws them with the reference's
 * distributions; tests/golden/make_loader_fixtures.py records the live reference's).  Clouds live in (b, stride, 3)
 * buffers so that added points can be appended behind the p original ones.
 * pipeline_norm_affine: replaces _pc_normalize (corrupt_util.py:7-17; when `normalise`), the maps of 'affine_r3'
 *   (:1062-1070 -> corrupt_tranlate :130-140, corrupt_scale_nonorm_2p :82-92, corrupt_rotate_360 :241-263,
 *   corrupt_reflection :390-409, corrupt_shear_p5 :412-428) as nmaps[i] <= 3 maps of 12 floats (3x3 M row-major, t):
 *   y = x M + t applied in order, and corrupt_jitter (:179-191): y += sigma[i] * noise[i,k,:] (noise may be NULL).
 * pipeline_add_global: replaces corrupt_add_global (:830-841) with _sample_points_inside_unit_sphere (:42-56):
 *   u (b, nmax, 3) = the radius / cos(theta) / phi uniforms; count[i] points are written behind row p0.
 * pipeline_add_local: replaces corrupt_add_local (:844-870): added point j of cloud i = cloud point seed[i,j] +
 *   sigma[i,j] * noise[i,j,:], divided by its squared norm when that exceeds 1 (as the reference does).
 * pipeline_density: replaces density (:875-897): alive[i,k] &= dist01(xyz, view[i]) * gate[i] < r[i,k].
 * pipeline_subset: replaces ShapeNet.random_sample (:76-88): out (b, n, 3) = the n alive points of smallest key, in
 *   ascending key order (ties by index) -- with keys = ranks of a permutation this IS pc[permutation[:n]]; with fewer
 *   than n survivors they repeat cyclically (the reference refills by sampling with replacement, then shuffles).
 *   alive may be NULL (all alive).  p <= 16384, n <= 16384.
 */
int pdae_pipeline_norm_affine(int b, int p, int out_stride, int normalise, const float* xyz, const int32_t* nmaps,
                              const float* maps, const float* sigma, const float* noise, float* out,
                              pdae_stream_t stream);
int pdae_pipeline_add_global(int b, int nmax, int stride, int p0, const int32_t* count, const float* u, float* xyz,
                             pdae_stream_t stream);
int pdae_pipeline_add_local(int b, int nmax, int stride, int p0, const int32_t* count, const int32_t* seed,
                            const float* sigma, const float* noise, float* xyz, pdae_stream_t stream);
int pdae_pipeline_density(int b, int p, int stride, const float* xyz, const float* view, const float* gate,
                          const float* r, unsigned char* alive, pdae_stream_t stream);
int pdae_pipeline_subset(int b, int p, int stride, int n, const float* xyz, const unsigned char* alive,
                         const float* keys, float* out, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Chamfer distance.  Replaces chamfer_cuda_forward(xyz1, xyz2)
 *   extensions/chamfer_dist/chamfer.cu:147-171 (kernel :15-145) and
 * chamfer_cuda_backward(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2)
 *   chamfer.cu:203-229 (kernel :173-201); pybind names chamfer.forward /
 *   chamfer.backward (chamfer_cuda.cpp:36-39).
 * xyz1 (b,n,3), xyz2 (b,m,3) -> dist1 (b,n), idx1 (b,n) i32 [nearest in xyz2],
 * dist2 (b,m), idx2 (b,m) i32 [nearest in xyz1]; lowest index wins ties.
 * backward: grad_xyz1 (b,n,3), grad_xyz2 (b,m,3) fully written.
 */
int pdae_chamfer_forward(int b, int n, const float* xyz1, int m,
                         const float* xyz2, float* dist1, float* dist2,
                         int32_t* idx1, int32_t* idx2, pdae_stream_t stream);
int pdae_chamfer_backward(int b, int n, const float* xyz1, int m,
                          const float* xyz2, const int32_t* idx1,
                          const int32_t* idx2, const float* grad_dist1,
                          const float* grad_dist2, float* grad_xyz1,
                          float* grad_xyz2, pdae_stream_t stream);
/* ChamferDistanceL2 (extensions/chamfer_dist/__init__.py:29-44: `torch.mean(dist1) + torch.mean(dist2)`) without the
 * reduction / expand / divide launches around the two kernels: mean_sum2 writes mean(a) + mean(b) into out[0] (two
 * small launches, fixed summation order);
 * chamfer_backward_mean is chamfer.backward for grad_dist1 = grad_loss[0] / (b n), grad_dist2 = grad_loss[0] / (b m)
 * (what autograd's mean backward would materialise), grad_loss a DEVICE scalar. */
int pdae_mean_sum2(long long na, const float* a, long long nb, const float* b, float* workspace /* 256 floats */,
                   float* out, pdae_stream_t stream);
int pdae_chamfer_backward_mean(int b, int n, const float* xyz1, int m, const float* xyz2, const int32_t* idx1,
                               const int32_t* idx2, const float* grad_loss, float* grad_xyz1, float* grad_xyz2,
                               pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Approximate earth mover's distance.  Replaces ApproxMatchForward /
 * MatchCostForward / MatchCostBackward, extensions/emd/cuda/emd_kernel.cu
 * :168-194, :256-280, :369-398 (kernels :25-158, :200-243, :286-355); pybind
 * names emd_cuda.approxmatch_forward / matchcost_forward / matchcost_backward
 * (emd.cpp:23-27).
 * xyz1 (b,n,3), xyz2 (b,m,3); match (b,m,n) f32; cost (b) f32;
 * temp is scratch of b*2*(n+m) floats (the reference allocates it,
 * emd_kernel.cu:183).
 */
int pdae_emd_approxmatch(int b, int n, int m, const float* xyz1,
                         const float* xyz2, float* match, float* temp,
                         pdae_stream_t stream);
int pdae_emd_matchcost(int b, int n, int m, const float* xyz1,
                       const float* xyz2, const float* match, float* cost,
                       pdae_stream_t stream);
int pdae_emd_matchcost_grad(int b, int n, int m, const float* grad_cost,
                            const float* xyz1, const float* xyz2,
                            const float* match, float* grad1, float* grad2,
                            pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * DGCNN encoder (csrc/dgcnn.hip).  Replaces, for Point_CAE_DGCNN_FCOnly (models/PointCAE_DGCNN.py:146-231), the
 * reference's feature-space kNN + edge features (models/dgcnn_util.py:7-34: matmul, topk, advanced-index gather,
 * cat of (x_j - x_i, x_i) as a (B, 2C, N, 20) tensor) and the Conv2d -> BatchNorm2d -> LeakyReLU(0.2) -> max over the
 * 20 neighbours of every EdgeConv (:99-131), and conv5's BatchNorm1d -> LeakyReLU -> max over the points (:132-136).
 * Activations are rows (points) x channels; b clouds of n points; R = b n.
 *   rows_sqnorm:  xx[r] = |x_r|^2 (C % 4 == 0).   rows_pad: out (R, cp) = x (R, c) with zero columns appended.
 *   edge_weight_stack: ws (2 co, kp) = [W1; W2 - W1], zero-padded from cin to kp columns, from the Conv2d weight
 *                 w (co, 2 cin) = [W1 | W2] over cat(x_j - x_i, x_i); edge_weight_unstack: its transpose,
 *                 dw (co, 2 cin) = [dWs_top - dWs_bottom | dWs_bottom].
 *   gram_topk:    idx (b, n, k) int32, ids within the cloud: the k largest of pd[i][j] = (-xx_j + 2 g_ij) - xx_i
 *                 (dgcnn_util.knn's expression -- xx (B, 1, N) broadcasts over the columns first -- each operation
 *                 rounded), best first, the lower id on equal values;
 *                 gram (b, n, n) = X_b X_b^T from pdae_rows_gemm_batched.  k <= 64.
 *   xyz_topk:     the same idx for the FIRST EdgeConv, whose features are the points themselves: x4 (b n, 4) = xyz rows
 *                 zero-padded to 4 columns (rows_pad), g_ij = fma(z z', fma(y y', x x')) computed in the kernel -- no
 *                 (b, n, n) Gram matrix; n <= 6144 (a block keeps its cloud in LDS).  pd_out (nullable, b n n): the -pd values the selection saw (tests).
 *   knn_reverse:  the reverse graph: rev_start (b, n+1), rev_src (b, n k): the points that list point s as a
 *                 neighbour are rev_src[b][rev_start[b][s] .. rev_start[b][s+1]), ascending.  n <= 4096.
 *   edge_gather_stats: pq (R, 2 co) = [p | q], p = W1 x, q = (W2 - W1) x, so that the conv output of edge (r, j) is
 *                 e = p[idx[r][j]] + q[r].  ONE pass over the gathered rows: esel (R, co) the winning e of every
 *                 (point, channel) -- max over j where gamma > 0, min where gamma < 0 (y = lrelu(bn(e)) is monotone
 *                 in e with the sign of gamma), the first edge where gamma = 0 (torch.max's first occurrence) --
 *                 sel (R, co) uint16 the winner's id within the cloud, psum (R, co) = sum_j p[idx[r][j]], and
 *                 sums (2 co doubles) = sum e, sum e^2 over all R k edges (part: pdae_edge_parts() x 2 co doubles of
 *                 scratch; added in block order).  co a power of two in 16..1024, n <= 65535.
 *                 -> pdae_bn_finalize(co, R k, sums, ...) gives scale / shift / mean / invstd and the running estimates.
 *   bn_lrelu_rows: out[r][c] = lrelu(e[r][c] scale[c] + shift[c]), slope 0.2; out2 (nullable, row stride ld2): a
 *                 second copy into a wider row-major tensor (the concatenated features conv5 reads).
 *   bn_lrelu_backward_reduce: g = (d1 + d2) * (y > 0 ? 1 : 0.2), y = e scale + shift (d1 contiguous, d2 with row
 *                 stride ld2, either nullable); sums (2 C doubles) = sum g, sum g xhat, xhat = (e - mean) invstd;
 *                 dbeta = sum g, dgamma = sum g xhat as floats (nullable).  part: pdae_edge_parts() x 2 C doubles.
 *   edge_backward: dpq (R, 2 co) = [dp | dq], the gradient of pq under training-mode BatchNorm over the R k edges:
 *                 d e[r][j] = scale (dy[r][j] - c1 - xhat[r][j] c2), dy = g at the winners and 0 elsewhere,
 *                 c1 = sums[0] / (R k), c2 = sums[1] / (R k); dq[r] = sum_j d e[r][j] (closed form from psum),
 *                 dp[s] = sum over the edges arriving at s (a gather over the reverse graph: no atomics).
 *   cloud_pool_stats: y (R, C) -> ysel (b, C) the winning row value per cloud and channel (max / min / first by
 *                 the sign of gamma), arow (b, C) int32 its row within the cloud, sums (2 C doubles) = sum y, sum y^2.
 *                 A cloud's rows are split over rs = pdae_cloud_pool_splits(b, n) blocks; scratch: pv, pr (b, rs, C)
 *                 the ranges' winners, part b rs x 2 C doubles.
 *   cloud_pool_backward: dy[r][c] = scale ((r == arow[b][c] ? g[b][c] : 0) - c1 - xhat[r][c] c2), sums from
 *                 bn_lrelu_backward_reduce over the (b, C) winners, c1 / c2 = sums / R.
 */
int pdae_rows_sqnorm(int R, int C, const float* x, float* xx, pdae_stream_t stream);
int pdae_rows_pad(long long R, int c, int cp, const float* x, float* out, pdae_stream_t stream);
int pdae_edge_weight_stack(int co, int cin, int kp, const float* w, float* ws, pdae_stream_t stream);
int pdae_edge_weight_unstack(int co, int cin, int kp, const float* dws, float* dw, pdae_stream_t stream);
/* ..._multi: the same for n <= 8 layers in ONE launch (HOST arrays of sizes and device pointers): the encoder stacks its
 * four EdgeConv weights before the first layer and unstacks their gradients after the last one. */
int pdae_edge_weight_stack_multi(int n, const int* co, const int* cin, const int* kp, const float* const* w,
                                 float* const* ws, pdae_stream_t stream);
int pdae_edge_weight_unstack_multi(int n, const int* co, const int* cin, const int* kp, const float* const* dws,
                                   float* const* dw, pdae_stream_t stream);
int pdae_gram_topk(int b, int n, int k, const float* gram, const float* xx, int32_t* idx, pdae_stream_t stream);
int pdae_xyz_topk(int b, int n, int k, const float* x4, const float* xx, int32_t* idx, float* pd_out /*nullable*/,
                  pdae_stream_t stream);
int pdae_knn_reverse(int b, int n, int k, const int32_t* idx, int32_t* rev_start, int32_t* rev_src,
                     pdae_stream_t stream);
int pdae_edge_parts(void);
int pdae_edge_gather_stats(int b, int n, int k, int co, const float* pq, const int32_t* idx, const float* gamma,
                           float* esel, unsigned short* sel, float* psum, double* part, double* sums,
                           pdae_stream_t stream);
int pdae_bn_lrelu_rows(long long R, int C, const float* e, const float* scale, const float* shift, float* out,
                       float* out2 /*nullable*/, int ld2, pdae_stream_t stream);
int pdae_bn_lrelu_backward_reduce(long long R, int C, const float* d1 /*nullable*/, const float* d2 /*nullable*/,
                                  int ld2, const float* e, const float* scale, const float* shift, const float* mean,
                                  const float* invstd, float* g, double* part, double* sums,
                                  float* dgamma /*nullable*/, float* dbeta /*nullable*/, pdae_stream_t stream);
int pdae_edge_backward(int b, int n, int k, int co, const float* g, const float* pq, const unsigned short* sel,
                       const float* psum, const int32_t* rev_start, const int32_t* rev_src, const float* scale,
                       const float* mean, const float* invstd, const double* sums, float* dpq, pdae_stream_t stream);
int pdae_cloud_pool_splits(int b, int n);
int pdae_cloud_pool_stats(int b, int n, int C, const float* y, const float* gamma, float* ysel, int32_t* arow,
                          float* pv, int32_t* pr, double* part, double* sums, pdae_stream_t stream);
int pdae_cloud_pool_backward(int b, int n, int C, const float* y, const float* g, const int32_t* arow,
                             const float* scale, const float* mean, const float* invstd, const double* sums,
                             float* dy, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Dense layers (csrc/rows_gemm.hip).  The reference runs nn.Linear / 1x1
 * nn.Conv1d through cuBLAS / cuDNN in fp32; here: row-major activations
 * (rows, channels), weights in torch's (out, in) layout, K % 4 == 0.  Attention.qkv /
 * proj (models/PointCAE_transformer.py:113-137), Mlp.fc1 / act / fc2 (:94-110),
 * pos_embed (:329-333), increase_dim (:653-658), and their backward.  Small-M
 * GEMMs (M = B * T tokens): a family of tile shapes, a per-shape plan, optional
 * split-K into slabs, no atomics (results are bit-identical run to run).
 *
 *   rows_gemm:  Y[M,N] = epi(X[M,K] . op(W))
 *       w_kn = 0: W is [N,K] (torch's (out,in) layout: a Linear's forward)
 *       w_kn = 1: W is [K,N] (the same (out,in) weight as the data-gradient
 *                 operand: dX[M,in] = dY[M,out] . W[out,in]; no transposed copy)
 *       epi  = 0: Y = acc (+ bias, nullable)
 *              1: Y = ReLU(acc + bias)                              (w_kn = 0)
 *              2: z = acc + bias, Y = GELU(z), Z = GELU'(z)   fc1 + nn.GELU in
 *                 one pass; Z is the factor the backward needs     (w_kn = 0)
 *              3: Y = acc * Z                   backward of 2: X = the gradient
 *                 of fc2's output, W = fc2's weight, Z from the forward: Y is
 *                 the gradient of fc1's output                     (w_kn = 1)
 *              4: Y = Z > 0 ? acc : 0      backward through a ReLU whose output
 *                 Z the forward kept (epi 1, or fold_input): the data gradient
 *                 arrives already masked, relu'(0) = 0 as ATen  (either layout)
 *       cfg    : tile shape 0..7, or -1 = planned per shape
 *       splits : 1, or S in 2..8 = split the reduction: Y is then S slabs
 *                [S][M][N] of partial products (epi 0, no bias) which the
 *                consumer adds up (residual_layernorm_forward / layernorm_backward
 *                take a slab count); -1 = 1.
 *       stream_blocks : 0, or P (a multiple of 8) = stream-K: the (tile, k-tile)
 *                units are dealt in equal contiguous ranges to P blocks; the q-th
 *                piece of a tile goes to slab q of Y, unused slabs of a tile are
 *                zero-filled (`splits` = number of slabs, as planned).
 *   rows_gemm_plan: the (cfg, splits, stream_blocks) rows_gemm would pick;
 *       may_split = 0 keeps splits = 1 and stream_blocks = 0; 1 allows up to 4 slabs (what the LayerNorm
 *       kernels add on their way); 2..8 up to that many (a caller with its own consumer: slab_sum_epi).
 *   slab_sum_epi: Y (M,N) = epi(sum_s slabs[s] + bias) in slab order, epi 0 store | 1 ReLU | 4 Z > 0 ? . : 0 --
 *       the Linear layers of the coarse heads (models/PointCAE_DGCNN.py:160-166 recfc, PointCAE_pointnetv2.py:151-156
 *       folding1, PointCAE_transformer.py coarse_pred) run on 32-128 rows: their reductions are split 8 ways.
 *   rows_wgrad: weight gradients of a GROUP of nprob <= 8 Linear layers that
 *       share M in one launch: dW_p[N_p,K_p] = dY_p[M,N_p]^T . X_p[M,K_p],
 *       db_p[N_p] = column sums of dY_p (db or db[p] nullable).  Pointer arrays
 *       are HOST arrays of device pointers.  (tile, 32-row chunk) work units are
 *       dealt in equal contiguous ranges to one residency of the chip; the
 *       partial tiles go to `workspace` and are added in block order by a second
 *       launch; rows_wgrad_workspace returns the workspace size in floats.
 */
int pdae_rows_gemm(int M, int N, int K, const float* X, const float* W, int w_kn,
                   const float* bias /*nullable*/, int epi, float* Z /*epi 2,3,4*/,
                   float* Y, int cfg, int splits, int stream_blocks,
                   pdae_stream_t stream);
/* The masked patches' share of the embedder backward by algebra (point_dae_amd/patch_embed.py; Encoder,
 * models/PointCAE_transformer.py:37-51, behind MaskTransformer.forward :424-469 which drops the masked tokens).
 * Rows of a group whose token is dropped carry no activation gradient into BatchNorm-2's backward, so their
 * conv-output gradient is the correction alone, dh = u + v * h (u, v per channel).  Entries:
 *   bnrelu_backward_listed_apply (declared with rows_gemm_bnrelu_stats below): given S (the sums = dbeta, dgamma,
 *       over the listed groups' compact dA), dA is overwritten in place with the listed groups' conv-output
 *       gradient, gsum (nullable) receives their row sums (row = position in the list, or the group id when
 *       gsum_by_group), uv[2][C] (nullable) the correction's u, v.  n_listed <= G.
 *   masked_group_sums: dgb[groups[cg]] = v * hs[cg] + 32 * xe[cg]: the row sums of dh over a masked group
 *       (hs = the group's summed conv output without its bias term, xe = u + v * gb).
 *   group_sum_listed: out[cg] = sum of the 32 rows of X's group groups[cg] (groups NULL: of group cg, every group).
 *   rows_wgrad_listed (declared with the weight gradients below): dW[N,K] = sum_m dY[rowA(m)]^T X[rowB(m)], whole
 *       32-row groups gathered on either operand; dY = X with one list = a Gram matrix.
 *   group_gemm_scatter: Y[c_groups[m/32]*32 + m%32] = X[a_groups[m/32]*32 + m%32] . W[N,K]^T + gbias[m/32]
 *       (a_groups, gbias nullable); rows of Y outside the listed groups are not touched. */
int pdae_masked_group_sums(int n_listed, int C, const float* hs, const float* xe, const float* v,
                           const int32_t* groups, float* dgb, pdae_stream_t stream);
int pdae_group_sum_listed(int n_listed, int C, const float* X, const int32_t* groups, float* out,
                          pdae_stream_t stream);
int pdae_group_gemm_scatter(int M, int N, int K, const float* X, const int32_t* a_groups, const float* W,
                            const float* gbias, float* Y, int ldy, const int32_t* c_groups,
                            pdae_stream_t stream);
/*   group_gemm_scatter_add: group_gemm_scatter, and the gradient of the max over a group's 32 points (:47 torch.max)
 *       lands where the rows are stored: Y[g*32 + sarg[g][n]][n] receives + sgrad[g][n] for every destination group
 *       g = c_groups[m/32] (sgrad, sarg: [groups of Y][N]; both NULL: group_gemm_scatter).  Bit for bit the rows that
 *       group_gemm_scatter followed by group_scatter_add leaves. */
int pdae_group_gemm_scatter_add(int M, int N, int K, const float* X, const int32_t* a_groups, const float* W,
                                const float* gbias, float* Y, int ldy, const int32_t* c_groups, const float* sgrad,
                                const unsigned char* sarg, pdae_stream_t stream);

/* Set-abstraction levels of the PointNet++ encoder (Point_CAE_PointNetv2;
 * extensions/pointnet2/pointnet2_modules.py PointnetSAModule: SharedMLP of
 * Conv2d 1x1 (no bias) -> BatchNorm2d -> ReLU layers, then F.max_pool2d over nsample)
 * on rows = (cloud, centre, sample):
 *   conv_stats: Y[M,N] = act(X[M,K]) . W[N,K]^T and this layer's batch statistics
 *       (stats [8][2][N] partial sums / sums of squares for bn_finalize); act = the
 *       previous layer's BatchNorm + ReLU, relu(x*scale[k] + shift[k]), applied while
 *       X is staged (scale = shift = NULL: X as is).  The normalised activations are
 *       never stored.  Backward of a layer: bnrelu_backward, then
 *       rows_wgrad_listed / rows_gemm (w_kn) as in the patch embedder.
 *   bnrelu_group_max: out[g][c] = max_j relu(y[g*ns+j][c]*scale[c] + shift[c]),
 *       arg[g][c] = the first j attaining it (ns <= 256).
 *   group_max_scatter_n: dense[g*ns+j][c] = (j == arg[g][c]) ? grad[g][c] : 0. */
int pdae_conv_stats(int M, int N, int K, const float* X, const float* scale /*nullable*/,
                    const float* shift /*nullable*/, const float* W, float* Y, float* stats,
                    pdae_stream_t stream);
int pdae_bnrelu_group_max(long long G, int ns, int C, const float* y, const float* scale,
                          const float* shift, float* out, unsigned char* arg, pdae_stream_t stream);
int pdae_group_max_scatter_n(long long G, int ns, int C, const float* grad, const unsigned char* arg,
                             float* dense, pdae_stream_t stream);
/* pool_bn_backward: ReLU + BatchNorm backward of a level's LAST layer straight through the max-pool:
 * grad[G][C] = gradient of the pooled output `out`, arg from bnrelu_group_max, y the raw conv output;
 * -> dy[G*ns][C] = gradient of y, S[2][C] = (dbeta, dgamma).  The gradient of relu(bn(y)) is non-zero
 * only at the arg-max rows, so the sums gather one y element per (group, channel) and the dense
 * scatter + two sweeps over it (group_max_scatter_n, bnrelu_backward) are replaced by one read of y
 * and one write of dy.  Fixed summation order (per-block partials in `workspace`, C/4 must divide 256;
 * pool_bn_backward_workspace gives its size in floats). */
long long pdae_pool_bn_backward_workspace(long long G, int C);
int pdae_pool_bn_backward(long long G, int ns, int C, const float* grad, const unsigned char* arg,
                          const float* out, const float* y, const float* mean, const float* invstd,
                          const float* gamma, float* S, float* workspace, float* dy, pdae_stream_t stream);
/* One set-abstraction level in EVALUATION mode, forward only, as one kernel (csrc/sa_eval.hip;
 * extensions/pointnet2/pointnet2_modules.py:31-72,124-158 with every BatchNorm2d on its running estimates, i.e. the
 * per-channel affine scale_l = gamma / sqrt(var + eps), shift_l = beta - mean * scale_l):
 *   out[b*np + p, :] = max over s of relu(scale2 (W2 relu(scale1 (W1 relu(scale0 (P[b*N + j] + W0x d) + shift0)) + shift1))
 *                      + shift2),   j = idx[b,p,s],  d = xyz[b,j] - new_xyz[b,p]
 * xyz (B,N,3), new_xyz (B,np,3), idx (B,np,ns) i32; P (B*N, C1) = features (B*N, C0) . W0f^T, the feature columns of the
 * first layer's weight applied once per SOURCE point by the caller (NULL exactly when C0 == 0); W0x (C1, 3) its
 * coordinate columns, applied per (centre, sample) on the centred difference; W1 (C2, C1), W2 (C3, C2); out (B*np, C3).
 * No (B np ns, .) tensor exists; no atomics, fixed reduction order.  An index outside [0, N) is clamped.
 * sa_eval_supported: 1 when the kernel takes the layout -- ns 32 or 64 and (C1, C2, C3) = (64, 64, 128) or
 * (128, 128, 256) -- else 0; sa_eval_forward returns PDAE_ERR_UNSUPPORTED for every other before anything is launched.
 * P, scale0, shift0, W1, W2 16-byte aligned. */
int pdae_sa_eval_supported(int ns, int C0, int C1, int C2, int C3);
int pdae_sa_eval_forward(int B, int N, int np, int ns, int C0, int C1, int C2, int C3, const float* xyz,
                         const float* new_xyz, const int32_t* idx, const float* P /*nullable, C0 = 0*/, const float* W0x,
                         const float* scale0, const float* shift0, const float* W1, const float* scale1,
                         const float* shift1, const float* W2, const float* scale2, const float* shift2, float* out,
                         pdae_stream_t stream);

/* The FIRST layer of a set-abstraction level in TRAINING mode, split by source point (csrc/sa_train.hip): the identity of
 * sa_eval_forward's layer 0 with batch statistics, forward and backward.  No (B np ns, 4 + C0) grouped tensor exists.
 *   sa_first_forward:  y0[row, :] = P[b*N + j, :] + W0x d,  j = idx[row],  d = xyz[b,j] - new_xyz[b,p]  (row = (b, p, s);
 *       R = B np ns rows; P (B*N, C1) = features . W0f^T from the caller, NULL exactly when C0 == 0; W0x (C1, 3)), the raw
 *       conv output the level's next pdae_conv_stats reads, and stats [8][2][C1], the partial column sums of y0 and y0^2
 *       in the layout pdae_conv_stats writes (-> pdae_bn_finalize with P = 8).
 *   sa_first_backward: dy0 (R, C1) the gradient of y0 ->
 *       dP[b*N + j, :] = the sum of dy0[row, :] over the rows of cloud b whose idx is j, in ascending row order (fully
 *           written; NULL exactly when C0 == 0), from which the caller takes dW0f = dP^T features and dfeatures = dP W0f;
 *       dW0x[c, k]     = sum over the rows of dy0[row, c] * d[row, k].
 * Fixed summation order throughout (block partials in `workspace`, added in block order; no float atomics): the same bits
 * on every run.  An index outside [0, N) is clamped.  workspace: sa_first_forward_workspace / _backward_workspace floats.
 * sa_first_supported: 1 when the kernels take the layout -- ns 32 or 64, C0 and C1 multiples of 4, C1 / 4 a divisor of
 * 256, and with C0 > 0 (a dP to form) N <= 4096 and 4 (2 N + 1 + 2 np ns) <= 150 KB, the sort of a cloud's rows in LDS --
 * else 0; both entries return PDAE_ERR_UNSUPPORTED for every other layout before anything is read or launched.
 * P, y0, dy0, dP and the workspace 16-byte aligned. */
int pdae_sa_first_supported(int B, int N, int np, int ns, int C0, int C1);
long long pdae_sa_first_forward_workspace(long long R, int C1);
long long pdae_sa_first_backward_workspace(long long R, int C1);
int pdae_sa_first_forward(int B, int N, int np, int ns, int C0, int C1, const float* xyz, const float* new_xyz,
                          const int32_t* idx, const float* P /*nullable, C0 = 0*/, const float* W0x, float* y0, float* stats,
                          float* workspace, pdae_stream_t stream);
int pdae_sa_first_backward(int B, int N, int np, int ns, int C0, int C1, const float* xyz, const float* new_xyz,
                           const int32_t* idx, const float* dy0, float* dP /*nullable, C0 = 0*/, float* dW0x,
                           float* workspace, pdae_stream_t stream);

/* First layer of the FoldingNet stage of Point_CAE_PointNetv2 (csrc/folding.hip;
 * models/PointCAE_pointnetv2.py:157-167: folding2[0] over [grid(2) | coarse point(3) |
 * global feature(1024)] for `cells` grid cells x `coarse` points x `clouds`).  The
 * conv is linear in the three column blocks: a[clouds,C] (feature block + bias),
 * p[clouds*coarse,C] (coarse-point block), gd[cells,C] (grid block) come from three
 * small GEMMs and
 *   fold_input:      h[((b*coarse + c)*cells + g), :] = ReLU((a[b] + p[b,c]) + gd[g])
 *   fold_input_grad: dpre = the gradient of the pre-activation, already masked by the
 *       ReLU (rows_gemm epi 4 of the next layer's data gradient):
 *       dp[b,c] = sum_g dpre,  dgd_part[blk][g] = sum over block blk's 64 (b,c) pairs --
 *       the caller adds the fold_input_grad_parts(clouds, coarse) partial sets in
 *       order (no atomics) and reduces dp over c for da.  C <= 1024. */
/*   fold_out_backward: the stage's last layer (C -> 3 outputs zero-padded to 4, weight W[4][C]) backwards in one
 *       pass over the kept middle activation h2: d2[r] = (h2[r] > 0) ? dy[r] . W : 0 and the per-block partials
 *       part[blk][4][C] of dW = dy^T h2 (fold_out_backward_parts(rows) sets; the caller adds them in order). */
int pdae_fold_input(int clouds, int coarse, int cells, int C, const float* a, const float* p,
                    const float* gd, float* h, pdae_stream_t stream);
/*   fold_input_rows: the first layer with a per-ROW term instead of the per-cloud / per-cell ones (the published
 *       variant's second folding stage, models/PointCAE_transformer.py:1050-1059, where the first fold's points are the
 *       extra input): h[r] = ReLU(row[r] + p[r / cells]); its backward is fold_input_grad's dp (clouds = 1). */
int pdae_fold_input_rows(long long pairs, int cells, int C, const float* row, const float* p, float* h,
                         pdae_stream_t stream);
int pdae_fold_input_grad_parts(int clouds, int coarse);
int pdae_fold_input_grad(int clouds, int coarse, int cells, int C, const float* dpre, float* dp,
                         float* dgd_part, pdae_stream_t stream);
int pdae_fold_out_backward_parts(long long rows);
int pdae_fold_out_backward(long long rows, int C, const float* dy /*[rows][4]*/, const float* h2, const float* W,
                           float* d2, float* part, pdae_stream_t stream);

/* Batched Y_b[M,N] = X_b[M,K] . W_b[N,K]^T, b < batch, element strides between the
 * problems (W_b = X_b: the Gram matrices behind DGCNN's feature-space kNN,
 * models/dgcnn_util.py:7-12).                                                  */
int pdae_rows_gemm_batched(int batch, int M, int N, int K, const float* X,
                           long long strideX, const float* W, long long strideW,
                           float* Y, long long strideY, pdae_stream_t stream);
int pdae_rows_gemm_plan(int M, int N, int K, int w_kn, int may_split, int* cfg,
                        int* splits, int* stream_blocks);
int pdae_slab_sum_epi(int S, int M, int N, const float* slabs /*[S][M][N]*/, const float* bias /*nullable*/, int epi,
                      const float* Z /*epi 4*/, float* Y, pdae_stream_t stream);
/* GEMM arithmetic of the row-GEMM family (rows_gemm, rows_wgrad*; the Linear layers the reference runs through
 * cuBLAS sgemm: models/PointCAE_transformer.py:94-158).  Both are fp32 in, fp32 out, fp32 accumulation:
 *   PDAE_GEMM_BF16X3  (default) every operand element is split EXACTLY into three bf16 terms, x = h + m + l, and a
 *       product is the sum of the six largest of the nine exact bf16 x bf16 partial products (hh, hm, mh, hl, lh, mm;
 *       the dropped ones are below 2^-25 of the product) accumulated in fp32 on v_mfma_f32_32x32x16_bf16, the hh
 *       terms and the small terms in separate accumulators.  Error against fp64 at or below the fp32-input MFMA
 *       kernels' on every shape of the models (tests/test_gpu_rows3.py), 2.67x their matrix-pipe ceiling.  Reductions
 *       with K % 32 != 0 run on the fp32-input kernels in either mode.
 *   PDAE_GEMM_F32MFMA v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain (the reference's arithmetic class bit for bit
 *       up to summation order).  Also selected by the environment variable PDAE_GEMM=f32mfma at first use.
 * Set before planning: pdae_rows_gemm_plan / the workspace queries answer for the arithmetic in force. */
enum { PDAE_GEMM_F32MFMA = 0, PDAE_GEMM_BF16X3 = 1 };
int pdae_set_gemm_arith(int arith);
int pdae_gemm_arith(void);
int pdae_rows_wgrad_workspace(int M, int nprob, const int* Ns, const int* Ks,
                              long long* floats);
int pdae_rows_wgrad(int M, int nprob, const float* const* dY,
                    const float* const* X, float* const* dW,
                    float* const* db /*nullable*/, const int* Ns, const int* Ks,
                    float* workspace, pdae_stream_t stream);
/* The same with a row count PER layer: the weight gradients of layers that do not share their rows -- every Linear of
 * every Transformer block of a stack -- in ONE launch (nprob <= 48): work = (128 x 128 output tile, 32-row chunk) units
 * of all layers in one list, dealt in equal contiguous ranges to one residency of the chip, partial tiles added in
 * block order by the reduction launch that follows.  A step's backward thereby issues its blocks' weight gradients as
 * two large launches (decoder stack, encoder stack) instead of one small launch per block.  Output tiles: 128 x 128 on the
 * default exact-split arithmetic (pdae_set_gemm_arith below; two accumulator sets per tile); on the fp32-input kernels
 * 128 x 384 when every K of the group is a multiple of 384 (8 waves per block), 128 x 128 otherwise.  On the exact-split
 * arithmetic a group whose layers share their row count and whose tiles fill the chip more than once runs as whole
 * rounds of ONE TILE PER BLOCK first (consecutive tiles together on an XCD, stored by their blocks: no partials) and the
 * remaining tiles as above.  The workspace queries answer for the arithmetic in force. */
int pdae_rows_wgrad_multi_workspace(int nprob, const int* Ms, const int* Ns, const int* Ks, long long* floats);
/* One weight gradient dW[N,K] = sum_m dY[rowA(m)]^T x(X[rowB(m)]) with the patch embedder's operand forms (Encoder,
 * models/PointCAE_transformer.py:37-51; its conv layers' weight gradients, which autograd computes with cuDNN/cuBLAS in
 * the reference): whole 32-row groups gathered on either operand (rowA(m) = a_groups[m/32]*32 + m%32; lists nullable =
 * compact operand; M % 32 == 0 with a list) and x = relu(X * scale[k] + shift[k]) when scale / shift are given
 * (BatchNorm + ReLU recomputed while X is staged).  db nullable: column sums of dY.  On the grouped weight-gradient
 * kernel: partial tiles in `workspace` (pdae_rows_wgrad_workspace(M, 1, &N, &K) floats), ordered reduction -- no
 * atomics, no memset, bit-identical run to run. */
int pdae_rows_wgrad_listed(int M, int N, int K, const float* dY, const int32_t* a_groups /*nullable*/, const float* X,
                           const int32_t* b_groups /*nullable*/, const float* scale /*nullable*/,
                           const float* shift /*nullable*/, float* dW, float* db /*nullable*/, float* workspace,
                           pdae_stream_t stream);
int pdae_rows_wgrad_multi(int nprob, const int* Ms, const float* const* dY, const float* const* X, float* const* dW,
                          float* const* db, const int* Ns, const int* Ks, float* workspace, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused layers of the patch embedder, Encoder.forward
 * (models/PointCAE_transformer.py:37-51).  Rows are points, 32 consecutive rows
 * form one group (patch); M % 32 == 0.  The reference runs each of these as a
 * cuDNN 1x1 conv followed by separate BatchNorm / ReLU / max / concat passes
 * over (B*G*32, C) tensors.
 *
 *   embed_conv_groupbias_stats  (second_conv[0] on concat([global, local]), :48-49,
 *       with the weight split into its global / local halves)
 *       Y[M,N] = X[M,K].W[N,K]^T + gbias[M/32,N]   (gbias = global half + bias,
 *       one row per group);  stats[8][2][N] receives 8 partial (sum, sum of
 *       squares) of Y's columns -- BatchNorm batch statistics (:32) without a
 *       pass over Y.  stats is zero-filled by the call.
 *   embed_bnrelu_conv_groupmax  (second_conv[1..3] + the max of :50)
 *       gmax[M/32,N] = max over groups of (relu(X*scale + shift).W^T + bias),
 *       garg[M/32,N] (u8) = first row inside the group attaining it; the (M,N)
 *       product itself is never written.
 * The weight gradients of these layers, dW[N,K] = dY[M,N]^T . relu(X[M,K]*scale + shift)
 * with the activation recomputed while it is staged, are rows_wgrad_listed's.
 */
int pdae_embed_conv_groupbias_stats(int M, int N, int K, const float* X,
                                    const float* W, const float* gbias,
                                    float* Y, float* stats,
                                    pdae_stream_t stream);
int pdae_embed_bnrelu_conv_groupmax(int M, int N, int K, const float* X,
                                    const float* scale, const float* shift,
                                    const float* W, const float* bias,
                                    float* gmax, unsigned char* garg,
                                    const int32_t* groups /*nullable*/,
                                    pdae_stream_t stream);
/* `groups` (embed_bnrelu_conv_groupmax, bnrelu_backward; b_groups of
 * rows_wgrad_listed): a list of group (patch) ids.  The last conv of the embedder
 * comes after the last BatchNorm, and the tokens of masked patches are thrown
 * away by MaskTransformer.forward (:449), so only the VISIBLE patches need that
 * GEMM: with a list, the M = 32*len(groups) rows of the product are gathered
 * from X group-wise (row m <- X[groups[m/32]*32 + m%32]) and the outputs are
 * compact, in list order.  Same numbers as computing all patches and selecting. */
/*   embed_bnrelu_conv_store_groupmax  (first_conv[1..3] + the max of :47)
 *       Y[M,N] = relu(X*scale + shift).W^T + bias;  gmax[M/32,N] = max over each
 *       group's 32 rows of Y, garg = the first row attaining it. */
int pdae_embed_bnrelu_conv_store_groupmax(int M, int N, int K, const float* X,
                                          const float* scale, const float* shift,
                                          const float* W, const float* bias,
                                          float* Y, float* gmax,
                                          unsigned char* garg,
                                          pdae_stream_t stream);
/*   embed_bnrelu_conv_store_groupmax_sum  (first_conv[1..3] + the max of :47, for a step whose backward takes the
 *       masked-groups algebra above) the same Y, gmax, garg, and gsum[M/32,N] = the sum over each group's 32 rows of
 *       Y out of the same epilogue, the rows added in row order: bit for bit group_sum_listed's sums, the fsum of
 *       that algebra without a sweep over Y. */
int pdae_embed_bnrelu_conv_store_groupmax_sum(int M, int N, int K, const float* X, const float* scale, const float* shift,
                                              const float* W, const float* bias, float* Y, float* gmax,
                                              unsigned char* garg, float* gsum, pdae_stream_t stream);

/*   embed_conv1_stats  first_conv[0] (:24, Conv1d(3, C, 1)) on rows (R,3):
 *       y[R,C] = x.W^T + bias, evaluated as ((x0*w0 + x1*w1) + x2*w2) + b, and
 *       stats[0][c] += sum y, stats[1][c] += sum y*y in fp64 (caller zeroes
 *       stats before the first call; C/4 must divide 256).
 *   bn_finalize         training-mode nn.BatchNorm1d bookkeeping (:25,:31) in one
 *       launch: batch mean and biased variance from `stats64` ([2][C] fp64 sums)
 *       or, when that is null, from `P` fp32 partial sets `partials` [P][2][C]
 *       (what embed_conv_groupbias_stats leaves); running_mean / running_var
 *       (unbiased, `momentum`; nullable) and num_batches_tracked (nullable)
 *       are updated in place; scale = gamma*invstd, shift = beta - mean*scale,
 *       mean and invstd (C each) are written.                               */
int pdae_embed_conv1_stats(int R, int C, const float* x, const float* W,
                           const float* bias /*nullable*/, float* y,
                           double* stats, pdae_stream_t stream);
/* embed_conv1_backward_weight: the first conv's weight gradient (K = 3), dW[c][k] = sum_r d[r][c] x[r][k], as
 * per-block partials part[blk][3][C] in one pass over d (embed_conv1_backward_weight_parts(R) sets; the caller
 * adds them in block order and transposes to the (C, 3, 1) weight layout). */
int pdae_embed_conv1_backward_weight_parts(int R);
int pdae_embed_conv1_backward_weight(int R, int C, const float* d, const float* x, float* part,
                                     pdae_stream_t stream);
/* embed_bnrelu_backward_conv1_weight: bnrelu_backward_apply on first_conv[1..2] (:25-26 BatchNorm1d + ReLU; R = 32 G rows,
 * sums S given) and embed_conv1_backward_weight on first_conv[0] (:24) in one pass: d (R, C) is READ ONLY, the gradient of
 * the conv output is formed per element by bnrelu_backward_apply's expression and consumed by embed_conv1_backward_weight's
 * row walk without being stored (the K = 3 conv has no data gradient).  part is bit for bit what the two entries leave. */
int pdae_embed_bnrelu_backward_conv1_weight(int R, int C, const float* d, const float* y1, const float* scale,
                                            const float* shift, const float* mean, const float* invstd,
                                            const float* gamma, const float* S, const float* x, float* part,
                                            pdae_stream_t stream);
int pdae_bn_finalize(int C, long long rows, const double* stats64 /*nullable*/,
                     const float* partials /*nullable*/, int P,
                     const float* gamma, const float* beta, float eps,
                     float momentum, float* running_mean /*nullable*/,
                     float* running_var /*nullable*/,
                     long long* num_batches_tracked /*nullable*/,
                     float* scale, float* shift, float* mean, float* invstd,
                     pdae_stream_t stream);

/* Memory-bound backward passes of the embedder (autograd of torch.max over the
 * 32 points of a group, nn.ReLU and training-mode nn.BatchNorm1d, :26,:32,:47,:50),
 * each a single fused sweep.  G groups of 32 rows, C channels (C % 4 == 0).
 *   group_max_scatter: out[g*32+r][c] = (r == arg[g][c]) ? grad[g][c] : 0
 *   group_scatter_add: dst[g*32+arg[g][c]][c] += grad[g][c]
 *   bnrelu_backward:   t = dA * (X*scale+shift > 0); S[0][c] = sum t (= d beta),
 *                      S[1][c] = sum t*xhat (= d gamma), xhat = (X-mean)*invstd;
 *                      dA <- gamma*invstd*(t - S0/R - xhat*S1/R) in place;
 *                      gsum[g][c] (nullable) = sum of the new dA over the group.
 */
int pdae_group_max_scatter(int G, int C, const float* grad,
                           const unsigned char* arg, float* out,
                           pdae_stream_t stream);
int pdae_group_scatter_add(int G, int C, const float* grad,
                           const unsigned char* arg, float* dst,
                           pdae_stream_t stream);
int pdae_bnrelu_backward(int G, int C, float* dA, const float* X,
                         const float* scale, const float* shift,
                         const float* mean, const float* invstd,
                         const float* gamma, float* S, float* gsum /*nullable*/,
                         int n_listed, const int32_t* groups /*nullable*/,
                         const int32_t* inv_group /*nullable*/,
                         float* dX /*nullable*/, pdae_stream_t stream);
/*   with groups / inv_group / dX: dA is compact (n_listed*32 rows, the listed
 *   groups; every other group's dA is zero), inv_group[g] = position of g in the
 *   list or -1, and the result for ALL G groups is written to dX.            */
/* The data gradient that flows INTO such a BatchNorm + ReLU, with bnrelu_backward's sums out of the same launch
 * (autograd of nn.Conv1d -> nn.BatchNorm1d -> nn.ReLU chains: models/PointCAE_transformer.py:26-35 Encoder,
 * extensions/pointnet2/pointnet2_modules.py SharedMLP; the reference runs a cuDNN/cuBLAS product, then ATen's
 * threshold_backward and batch_norm_backward sweeps over the (M, N) gradient):
 *   rows_gemm_bnrelu_stats   T[M,N] = (X*scale+shift > 0) ? dY[M,K] . W[K,N] : 0 -- the ReLU mask applied while the
 *       product tile is in registers -- and S[0][n] = sum_m T, S[1][n] = sum_m T xhat, xhat = (X-mean)*invstd.  X rows
 *       through `groups` (row m of the product = row groups[m/32]*32 + m%32 of X; M % 32 == 0) when given.  workspace:
 *       rows_gemm_bnrelu_stats_workspace(M, N) floats (one partial row of sums per 128-row band; added in band order
 *       in fp64: no atomics, bit-identical run to run).  On the fp32-input arithmetic, or without a workspace, the
 *       entry runs the plain product and bnrelu_backward's own reduction sweep.
 *   bnrelu_backward_apply   the second half of bnrelu_backward for a caller that holds S already: same arguments,
 *       S is read.
 *   bnrelu_backward_listed_apply   the same over a list of groups alone (the masked patches' algebra above). */
long long pdae_rows_gemm_bnrelu_stats_workspace(int M, int N);
int pdae_rows_gemm_bnrelu_stats(int M, int N, int K, const float* dY, const float* W, const float* X,
                                const int32_t* groups /*nullable*/, const float* scale, const float* shift,
                                const float* mean, const float* invstd, float* T, float* S, float* workspace,
                                pdae_stream_t stream);
int pdae_bnrelu_backward_apply(int G, int C, float* dA, const float* X, const float* scale, const float* shift,
                               const float* mean, const float* invstd, const float* gamma, const float* S,
                               float* gsum /*nullable*/, int n_listed, const int32_t* groups /*nullable*/,
                               const int32_t* inv_group /*nullable*/, float* dX /*nullable*/, pdae_stream_t stream);
int pdae_bnrelu_backward_listed_apply(int G, int C, float* dA, const float* X, const float* scale, const float* shift,
                                      const float* mean, const float* invstd, const float* gamma, const float* S,
                                      float* gsum, int gsum_by_group, float* uv, int n_listed, const int32_t* groups,
                                      pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Transformer block, Block.forward (models/PointCAE_transformer.py:155-158 with
 * the per-block position add of :174-177) and Attention.forward (:125-137).
 * Activations are rows (B*T, C); T tokens per sample, H heads of D = 64.
 *
 *   attention_forward   qkv (B*T, 3*H*D) as laid out by the qkv Linear
 *                       ([3][H][D] per row) -> o (B*T, H*D) =
 *                       softmax(q k^T * scale) v per (sample, head), and
 *                       lse (B,H,T) = log-sum-exp of each score row (saved for
 *                       the backward).  T <= 128.
 *   attention_backward  -> dqkv (B*T, 3*H*D), fully written.
 *   add_layernorm_forward  s = x (+ pos, nullable; then xsum receives s);
 *                       y = LayerNorm(s) * gamma + beta; mean/rstd (M) saved.
 *   layernorm_backward  dx = LayerNorm'(dy) (+ dres, nullable: the gradient
 *                       arriving over the skip connection); dgamma/dbeta (C)
 *                       are overwritten (or added to, see `accumulate`).
 *   gelu_forward / gelu_backward   exact (erf) GELU, nn.GELU default (:97,:107).
 *   scale_residual      y = res + keep[row/T] * (a + bias): Linear bias, timm
 *                       DropPath (keep[b] is 0 or 1/keep_prob) and the residual
 *                       add in one pass; bias / keep / res nullable.
 *   colsum              out[c] = sum over rows of X[:, c] (bias gradients).
 */
int pdae_attention_forward(int B, int T, int H, int D, float scale,
                           const float* qkv, float* o, float* lse,
                           pdae_stream_t stream);
int pdae_attention_backward(int B, int T, int H, int D, float scale,
                            const float* qkv, const float* o, const float* lse,
                            const float* d_o, float* dqkv, pdae_stream_t stream);
int pdae_add_layernorm_forward(int M, int C, const float* x,
                               const float* pos /*nullable*/, const float* gamma,
                               const float* beta, float eps,
                               float* xsum /*nullable*/, float* y, float* mean,
                               float* rstd, pdae_stream_t stream);
int pdae_layernorm_backward(int M, int C, const float* dy, int dy_slabs, const float* x,
                            const float* mean, const float* rstd,
                            const float* gamma, const float* dres /*nullable*/,
                            float* dx, float* dgamma, float* dbeta,
                            int accumulate, float* dacc /*nullable*/, int dacc_mode,
                            pdae_stream_t stream);
/*   residual_layernorm_forward / _backward: the previous sub-layer's tail folded in
 *       (Block.forward :155-158: x = x + drop_path(branch(...)) followed by the next
 *       norm):  s = res + keep[row/T] * (a + bias) (+ pos);  y = LayerNorm(s);
 *       xsum receives s.  bias / keep / pos nullable.  Backward:
 *       dx = LayerNorm'(dy) + dres (the gradient w.r.t. s = w.r.t. res and pos);
 *       da = keep[row/T] * dx (written only when keep is given; otherwise da == dx);
 *       dbias = column sums of da; dgamma / dbeta as layernorm_backward.
 *       a_slabs / dy_slabs (1..8): `a` / `dy` arrive as that many split-K slabs
 *       [slabs][M][C] of partial products (pdae_rows_gemm with splits > 1) and are
 *       added up in slab order while they are read; 1 = a plain [M][C] matrix.
 *       dacc / dacc_mode (both backward entries): dacc_mode 1 also writes dx to dacc,
 *       2 adds dx to dacc (the position embedding is re-added before EVERY block of a
 *       stack, :174-177, so its gradient is the sum of the blocks' dx: accumulated
 *       here instead of by one elementwise add per block); 0 = off.                  */
int pdae_residual_layernorm_forward(int M, int C, int T, const float* a, int a_slabs,
                                    const float* bias /*nullable*/,
                                    const float* keep /*nullable*/,
                                    const float* res, const float* pos /*nullable*/,
                                    const float* gamma, const float* beta,
                                    float eps, float* xsum, float* y, float* mean,
                                    float* rstd, pdae_stream_t stream);
int pdae_residual_layernorm_backward(int M, int C, int T, const float* dy, int dy_slabs,
                                     const float* x, const float* mean,
                                     const float* rstd, const float* gamma,
                                     const float* dres /*nullable*/,
                                     const float* keep /*nullable*/, float* dx,
                                     float* da /*nullable unless keep*/,
                                     float* dgamma, float* dbeta, float* dbias,
                                     int accumulate, float* dacc /*nullable*/,
                                     int dacc_mode, pdae_stream_t stream);
int pdae_gelu_forward(long long n, const float* z, float* h,
                      pdae_stream_t stream);
int pdae_gelu_backward(long long n, const float* z, const float* dh, float* dz,
                       pdae_stream_t stream);
int pdae_scale_residual(int M, int C, int T, const float* a,
                        const float* bias /*nullable*/,
                        const float* keep /*nullable*/,
                        const float* res /*nullable*/, float* y,
                        pdae_stream_t stream);
/* Two small fused launches in place of chains of framework elementwise kernels inside the step:
 * drop_path_keep: timm 0.4.5 DropPath (models/PointCAE_transformer.py:146-158 `self.drop_path`) for all `sites`
 *   stochastic-depth sites of a stack: r (sites, B) uniforms -> floor(r + keep[s]) / keep[s] (in place allowed).
 * pos_embed_fc1: the first layer of pos_embed / decoder_pos_embed (:329-333, :636-640: Linear(3,128) -> GELU) on the
 *   centre rows `rows` (int64 indices into xyz (.,3); NULL = all rows in order): h = GELU(z), gp = GELU'(z) for
 *   z = xyz . W1^T + b1, and xp (M,4) = the gathered rows zero-padded (the backward's weight-gradient operand). */
int pdae_drop_path_keep(int sites, int B, const float* r, const float* keep, float* out, pdae_stream_t stream);
/* tail_rows_gather / _scatter: TransformerDecoder.forward returns x[:, -return_token_num:] (models/PointCAE_transformer.py:
 *   225-232), so the last block's row-wise second half runs on the last `tail` tokens of every sample only.
 *   gather:  a_t (B tail, C) = rows T - tail .. T - 1 of every sample of a (B T, C); the same for b -> b_t (b nullable).
 *   scatter: da (B T, C) = da_t on those rows, ZERO elsewhere; the same for db_t -> db (db nullable).  C % 4 == 0. */
int pdae_tail_rows_gather(int B, int T, int tail, int C, const float* a, const float* b /*nullable*/, float* a_t,
                          float* b_t /*nullable*/, pdae_stream_t stream);
int pdae_tail_rows_scatter(int B, int T, int tail, int C, const float* da_t, const float* db_t /*nullable*/, float* da,
                           float* db /*nullable*/, pdae_stream_t stream);
int pdae_pos_embed_fc1(int M, int H, const float* xyz, const int64_t* rows, const float* w1, const float* b1, float* h,
                       float* gp, float* xp, pdae_stream_t stream);
int pdae_colsum(int M, int N, const float* X, float* out, int accumulate,
                pdae_stream_t stream);
/* Single launches in place of groups of framework launches inside the graphed step (csrc/glue.hip; every node of the step's
 * graph costs ~5 us whatever it moves):
 *   partials_sum_t    out (C, K) = sum_p part[p] (K, C) in a fixed order, written transposed: the first conv's weight gradient in the
 *                     parameter's layout (models/PointCAE_transformer.py:22 nn.Conv1d(3, 128, 1): weight (128, 3, 1)) from
 *                     embed_conv1_backward_weight's ordered partials.
 *   multi_copy        n independent float copies src[i] -> dst[i] of counts[i] elements in ONE launch per 128 entries (the gather of
 *                     the gradients autograd produced outside the flat gradient buffer of the data-parallel wrapper -- the
 *                     reference's DistributedDataParallel owns that copy inside its reducer, runner_pretrain.py:84-90).  src, dst,
 *                     counts, cols, src_ld are HOST arrays; cols / src_ld (both or neither; NULL = contiguous): entry i reads a 2-D
 *                     source of cols[i] columns with row stride src_ld[i] (<= 65535), dst is always contiguous.  src[i] NULL: dst[i] is zero-filled
 *                     (the parameters that received no gradient).
 *   assemble_tokens   the decoder's input (:700-703): out (B, G, C) = per sample [the Tv visible tokens | G - Tv copies of
 *                     mask_token]; _grad splits dout (B, G, C) into dvis (B, Tv, C) and dmask (B, G - Tv, C) (the mask token's
 *                     gradient is the column sum of dmask).  C % 4 == 0.
 *   embed_split_conv3_weight   second_conv[0]'s weight w (N, 2 K2) (:29 nn.Conv1d(512, 512, 1) on concat([global, local]), :44-46)
 *                     -> wg = w[:, :K2], wl = w[:, K2:], and wlt = wl^T (K2, N) (nullable).
 *   embed_masked_prep / embed_dw3_assemble   element-wise steps of the masked-groups algebra of conv3's backward
 *                     (point_dae_amd/patch_embed.py _masked_by_algebra): xe (Gm, C3) = u + gb[masked] * v and wv (C3, C2) =
 *                     diag(v) wl, with uv (2, C3) = [u; v];  dw3 (C3, 2 C2) = [dwg | dwl + diag(v) wgram + xterm]
 *                     (v NULL: [dwg | dwl], wgram / xterm unread). */
/*   pad2d             out (R2, C2) = in (R, C; row stride ld >= C: a column slice of a wider matrix) in the top-left corner, zeros elsewhere: the zero-padding of a ragged weight or
 *                     of a 3-column activation to the row GEMMs' multiples of 4 (F.pad: a fill and a copy) in one launch. */
/*   max_plus_mean     out (B, C) = max over t + mean over t of x (B, T, C), arg (B, C) = the first t of the maximum (uint8, T <= 255):
 *                     the published variant's global feature (models/PointCAE_transformer.py:1024 `x_vis.max(dim=1)[0] +
 *                     x_vis.mean(1)`); _grad: dx = g (1 / T + [t == arg]). */
int pdae_max_plus_mean(int B, int T, int C, const float* x, float* out, uint8_t* arg, pdae_stream_t stream);
int pdae_max_plus_mean_grad(int B, int T, int C, const float* g, const uint8_t* arg, float* dx, pdae_stream_t stream);
/*   hcat              out (R, sum cols) = up to four row-major pieces side by side, piece q read through row stride ld[q] >= cols[q]
 *                     (src, cols, ld: HOST arrays; src[q] NULL: cols[q] zero columns): the gradient of a conv weight whose column blocks were used as separate
 *                     operands (models/PointCAE_transformer.py:1040-1059 folding1/2[0] on [token | grid or point];
 *                     models/PointCAE_pointnetv2.py:157-167 folding2[0] on [grid | coarse point | feature]) in one launch. */
int pdae_hcat(int n, int R, const float* const* src, const int* cols, const int* ld, float* out, pdae_stream_t stream);
int pdae_pad2d(int R, int C, int ld, int R2, int C2, const float* in, float* out, pdae_stream_t stream);
int pdae_partials_sum_t(int P, int K, int C, const float* part, float* out, pdae_stream_t stream);
int pdae_multi_copy(int n, const float* const* src, float* const* dst, const long long* counts, const int* cols /*nullable*/,
                    const int* src_ld /*nullable*/, pdae_stream_t stream);
int pdae_assemble_tokens(int B, int G, int Tv, int C, const float* vis, const float* token, float* out, pdae_stream_t stream);
int pdae_assemble_tokens_grad(int B, int G, int Tv, int C, const float* dout, float* dvis, float* dmask, pdae_stream_t stream);
int pdae_embed_split_conv3_weight(int N, int K2, const float* w, float* wg, float* wl, float* wlt /*nullable*/,
                                  pdae_stream_t stream);
int pdae_embed_masked_prep(int Gm, int C3, int C2, const float* uv, const float* gb, const int32_t* masked, const float* wl,
                           float* xe, float* wv, pdae_stream_t stream);
/*   embed_masked_prep_fsum   embed_masked_prep (point_dae_amd/patch_embed.py _masked_by_algebra; Encoder,
 *                     models/PointCAE_transformer.py:37-51) whose launch also gathers fsum_m (Gm, C2) = gsum[masked] from
 *                     embed_bnrelu_conv_store_groupmax_sum's group sums gsum (BG, C2). */
int pdae_embed_masked_prep_fsum(int Gm, int C3, int C2, const float* uv, const float* gb, const int32_t* masked, const float* wl,
                                float* xe, float* wv, const float* gsum, float* fsum_m, pdae_stream_t stream);
int pdae_embed_dw3_assemble(int C3, int C2, const float* dwg, const float* dwl, const float* v /*nullable*/,
                            const float* wgram /*nullable*/, const float* xterm /*nullable*/, float* dw3, pdae_stream_t stream);
/*   scale_colsum        Y = keep[row/T] * X and out[c] (nullable) = column sums
 *                       of Y: autograd of scale_residual w.r.t. its branch and
 *                       bias in one pass (DropPath backward, timm drop.py).   */
int pdae_scale_colsum(int M, int N, int T, const float* X, const float* keep,
                      float* Y, float* out /*nullable*/, int accumulate,
                      pdae_stream_t stream);
/*   bias_gelu_forward   h = GELU(z + bias)            (fc1 epilogue, :104-106)
 *   bias_gelu_backward  dz = dh * GELU'(z + bias), dbias = column sums of dz
 * `accumulate` != 0 (layernorm_backward, colsum, bias_gelu_backward): the small
 * reduction outputs (dgamma/dbeta, out, dbias) are added to instead of being
 * zero-filled first, so a caller can hand in slices of ONE pre-zeroed arena and
 * save a memset node per call.                                              */
int pdae_bias_gelu_forward(int M, int C, const float* z, const float* bias,
                           float* h, pdae_stream_t stream);
int pdae_bias_gelu_backward(int M, int C, const float* z, const float* bias,
                            const float* dh, float* dz, float* dbias,
                            int accumulate, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused AdamW over a contiguous fp32 range (torch.optim.AdamW arithmetic:
 * decoupled weight decay, bias correction, eps added to sqrt(v_hat)); the
 * reference builds it over two parameter groups, tools/builder.py:41-101.
 * step is the 1-based update count.  One streaming pass: 16 B read + 12 B
 * written per parameter.
 */
int pdae_adamw_step(long long n, float* param, const float* grad,
                    float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int step,
                    pdae_stream_t stream);
/* adamw_step_gscale: pdae_adamw_step reading g * (*gscale) in place of g (the
 * multiply first, as torch scales .grad before the optimiser reads it); gscale
 * is a device scalar, e.g. grad_norm_clip's coefficient. */
int pdae_adamw_step_gscale(long long n, float* param, const float* grad,
                           float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                           float beta2, float eps, float weight_decay, int step,
                           const float* gscale, pdae_stream_t stream);
/* adamw_step_segments: the same update over up to PDAE_ADAMW_MAX_SEGMENTS
 * disjoint segments [offset, offset + count) of flat buffers of n floats, each
 * with its own lr and weight_decay, in ONE launch.  `segments` is a HOST array:
 * the table travels by value as a kernel argument, so a learning-rate change
 * writes nothing to the device and the launch can be captured.  Elements
 * outside every segment are neither read nor written.  Segments need no
 * alignment (up to 3 head and 3 tail elements are updated one by one); the
 * buffers are 16-byte aligned.  gscale: NULL, or adamw_step_gscale's device
 * scalar.  Two 16-byte aligned segments give the bits of two adamw_step[_gscale]
 * launches over the same ranges. */
#define PDAE_ADAMW_MAX_SEGMENTS 8
typedef struct pdae_adamw_segment {
  long long offset, count;
  float lr, weight_decay;
} pdae_adamw_segment;
int pdae_adamw_step_segments(long long n, int num_segments, const pdae_adamw_segment* segments,
                             float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                             float beta1, float beta2, float eps, int step,
                             const float* gscale /*nullable*/, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Classification fine-tuning glue (csrc/finetune.hip; models/Point_MAE.py:578-706
 * PointTransformer, tools/runner_finetune.py:81-270).  Every reduction runs in a
 * fixed order (no float atomics).
 *   prepend_token       out (B, 1+G, C) = per cloud [token (C) | x (B, G, C)];
 *                       _grad: dx (B, G, C) = dout[:, 1:], dtoken (C) = sum over b
 *                       (ascending) of dout[b, 0].  C % 4 == 0, buffers 16-byte
 *                       aligned.
 *   cls_max_concat      out (B, 2C) = [x[:, 0] | max_{t>=1} x[:, t]] of x (B, T, C),
 *                       arg (B, C) uint8 = the first maximal t (2 <= T <= 256);
 *                       _grad: dx (B, T, C) dense.  For finite x: a NaN is passed
 *                       over, where torch.max would return NaN.
 *   bn_relu_dropout     out = Dropout(p)(ReLU(BatchNorm1d(y))) of y (B, N).
 *                       training != 0: batch mean / biased variance (fp64) normalise,
 *                       running_mean / running_var (unbiased, momentum; nullable)
 *                       and num_batches_tracked (nullable) are updated, mean and
 *                       invstd (N) are written for the backward; an element is kept
 *                       when u (B, N uniforms; NULL = no dropout) >= p and scaled by
 *                       1/(1-p).  training == 0: the running estimates, no dropout.
 *                       training == 2 (a frozen BatchNorm inside a model in training
 *                       mode, set_bn_eval): the running estimates AND the draw u;
 *                       nothing of the BatchNorm's state is written.  With training
 *                       0 or 2, mean / invstd (nullable then) receive running_mean and
 *                       1/sqrt(running_var + eps) for _eval_grad.
 *                       _grad (training mode): dy, dgamma, dbeta in one launch.
 *                       _eval_grad (training 0 or 2): dy = g gamma invstd with g =
 *                       dout * keep/(1-p) * act', dbeta = sum g, dgamma = sum g xhat
 *                       (fp64, rows in order); B >= 1.
 *   softmax_xent        nn.CrossEntropyLoss() (mean, no smoothing) of logits (B, K)
 *                       against int64 labels in [0, K): *loss, *correct = the count of
 *                       rows whose first maximal logit is the label (float).  K <= 64,
 *                       B <= 4096.  A label outside [0, K) makes the loss NaN.
 *                       _grad: dlogits = (softmax - onehot) * (*dloss) / B.
 *   bn_lrelu_dropout    out = Dropout(p)(LeakyReLU(negative_slope)(BatchNorm1d(y))),
 *                       bn_relu_dropout's contract otherwise (training / eval, the
 *                       running estimates, u NULL = no dropout, _grad in one launch;
 *                       training mode with B < 2 is refused).  0 <= negative_slope
 *                       < 1; slope 0 gives bn_relu_dropout's bits.  The _grad's
 *                       LeakyReLU test recomputes the forward's pre-activation.
 *   softmax_xent_smooth the label-smoothed cross-entropy of DGCNN's smoothloss
 *                       (models/PointCAE_DGCNN.py:592-600): target t = onehot (1-eps)
 *                       + (1-onehot) eps/(K-1), loss_r = lse_r - sum_k t_k x_k, mean
 *                       over the rows added in row order; *correct as softmax_xent.
 *                       2 <= K <= 64, B <= 4096, 0 <= eps <= 1; eps 0 gives
 *                       softmax_xent's bits.  A label outside [0, K) makes the loss
 *                       NaN.  _grad: dlogits = (softmax - t) * (*dloss) / B.
 *   grad_norm_clip      the L2 norm of grad (n floats, 16-byte aligned) as
 *                       grad_norm_parts(n) fp64 per-block partials (caller's
 *                       workspace) added in block order: *norm (nullable) and *coef =
 *                       min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_), on the
 *                       device.                                                    */
int pdae_prepend_token(int B, int G, int C, const float* x, const float* token, float* out, pdae_stream_t stream);
int pdae_prepend_token_grad(int B, int G, int C, const float* dout, float* dx, float* dtoken, pdae_stream_t stream);
int pdae_cls_max_concat(int B, int T, int C, const float* x, float* out, unsigned char* arg, pdae_stream_t stream);
int pdae_cls_max_concat_grad(int B, int T, int C, const float* dout, const unsigned char* arg, float* dx,
                             pdae_stream_t stream);
int pdae_bn_relu_dropout(int B, int N, const float* y, const float* gamma, const float* beta, float eps,
                         float momentum, float* running_mean /*nullable*/, float* running_var /*nullable*/,
                         long long* num_batches_tracked /*nullable*/, int training, float p,
                         const float* u /*nullable*/, float* out, float* mean, float* invstd, pdae_stream_t stream);
int pdae_bn_relu_dropout_grad(int B, int N, const float* y, const float* gamma, const float* beta, const float* mean,
                              const float* invstd, float p, const float* u /*nullable*/, const float* dout, float* dy,
                              float* dgamma, float* dbeta, pdae_stream_t stream);
int pdae_bn_relu_dropout_eval_grad(int B, int N, const float* y, const float* gamma, const float* beta,
                                   const float* mean, const float* invstd, float p, const float* u /*nullable*/,
                                   const float* dout, float* dy, float* dgamma, float* dbeta, pdae_stream_t stream);
int pdae_softmax_xent(int B, int K, const float* logits, const int64_t* labels, float* loss, float* correct,
                      pdae_stream_t stream);
int pdae_softmax_xent_grad(int B, int K, const float* logits, const int64_t* labels, const float* dloss,
                           float* dlogits, pdae_stream_t stream);
int pdae_bn_lrelu_dropout(int B, int N, const float* y, const float* gamma, const float* beta, float eps,
                          float momentum, float* running_mean /*nullable*/, float* running_var /*nullable*/,
                          long long* num_batches_tracked /*nullable*/, int training, float negative_slope, float p,
                          const float* u /*nullable*/, float* out, float* mean, float* invstd, pdae_stream_t stream);
int pdae_bn_lrelu_dropout_grad(int B, int N, const float* y, const float* gamma, const float* beta, const float* mean,
                               const float* invstd, float negative_slope, float p, const float* u /*nullable*/,
                               const float* dout, float* dy, float* dgamma, float* dbeta, pdae_stream_t stream);
int pdae_bn_lrelu_dropout_eval_grad(int B, int N, const float* y, const float* gamma, const float* beta,
                                    const float* mean, const float* invstd, float negative_slope, float p,
                                    const float* u /*nullable*/, const float* dout, float* dy, float* dgamma,
                                    float* dbeta, pdae_stream_t stream);
int pdae_softmax_xent_smooth(int B, int K, float eps, const float* logits, const int64_t* labels, float* loss,
                             float* correct, pdae_stream_t stream);
int pdae_softmax_xent_smooth_grad(int B, int K, float eps, const float* logits, const int64_t* labels,
                                  const float* dloss, float* dlogits, pdae_stream_t stream);
int pdae_grad_norm_parts(long long n);
int pdae_grad_norm_clip(long long n, const float* grad, float max_norm, double* partials, float* norm /*nullable*/,
                        float* coef, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Linear-SVM evaluation protocol (csrc/svm.hip; tools/runner_finetune.py:1038-1049 of the reference fits
 * sklearn.svm.SVC(C=c, kernel='linear'), i.e. libsvm's one-vs-one C-SVC, for six values of C).
 * The n training samples are ordered by class: order[s] (device, n ints) is the Gram row of the s-th sample in class
 * order, class_ptr (HOST, K + 1 ints, 0 .. n, every class non-empty) the classes' ranges in it.  Cs: HOST, nC doubles.
 * Pairs (p, q), p < q, are numbered (0,1), (0,2), ..., P = K (K - 1) / 2.
 *   svm_ovo_train    the dual C-SVC of every (pair, C), one workgroup each, from the training Gram matrix G = X X^T
 *                    (n x ld fp32, ld >= n): SMO on the maximal violating pair, alpha and gradient in fp64, stopped
 *                    when the violation is < eps (libsvm's -e; the protocol's is 1e-3) or after max_iter iterations.
 *                    Ties go to the lowest member: two runs give the same bits.
 *                    coef (nC, K - 1, n) fp64 = alpha_s y_s in libsvm's dual_coef_ rows with the columns in class
 *                    order: the s-th sample, of class p, against class q sits in row q - 1 if q > p, else in row q.
 *                    rho (nC, P) by libsvm's calculate_rho; status (nC, P, 2) = iterations, 1 when max_iter was hit;
 *                    gap (nC, P) the final violation.  All outputs are fully written.
 *                    A pair of more than PDAE_SVM_MAX_PAIR members, K > PDAE_SVM_MAX_CLASSES: PDAE_ERR_UNSUPPORTED,
 *                    nothing is launched.  max_iter < 1, nC outside 1 .. PDAE_SVM_MAX_C, C <= 0: PDAE_ERR_BAD_ARG.
 *   svm_ovo_predict  from the test-by-train Gram matrix Gte (m x ld fp32): dec (nC, m, P) fp64 = sum over the pair's
 *                    members of coef * Gte - rho (lane-strided partial sums added in a fixed order), pred (nC, m)
 *                    int32 = libsvm's vote as a class INDEX 0 .. K - 1: dec > 0 votes for the pair's first class,
 *                    else for its second; the first class with the most votes.  n <= PDAE_SVM_PREDICT_MAX_TRAIN.   */
#define PDAE_SVM_MAX_PAIR 2048
#define PDAE_SVM_MAX_CLASSES 64
#define PDAE_SVM_MAX_C 8
#define PDAE_SVM_PREDICT_MAX_TRAIN 12288
int pdae_svm_ovo_train(int n, int ld, int K, int nC, const float* G, const int* order, const int* class_ptr /*host*/,
                       const double* Cs /*host*/, double eps, int max_iter, double* coef, double* rho, int* status,
                       double* gap, pdae_stream_t stream);
/* host-side: the status svm_ovo_train would refuse this layout with (no stream, nothing launched) */
int pdae_svm_ovo_supported(int n, int K, int nC, const int* class_ptr /*host*/, const double* Cs /*host*/, int max_iter);
int pdae_svm_ovo_predict(int m, int n, int ld, int K, int nC, const float* Gte, const int* order,
                         const int* class_ptr /*host*/, const double* coef, const double* rho, double* dec, int* pred,
                         pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Pretraining validation's classifier (csrc/linsvc.hip; tools/runner_pretrain.py:25-48 of the reference fits
 * sklearn.svm.LinearSVC(), i.e. liblinear's one-vs-rest L2-regularised squared-hinge machines with a regularised
 * intercept): a truncated-Newton solver of all columns at once, in the primal.  Column k is the machine of class
 * col0 + k: y_i = +1 where labels[i] == col0 + k, else -1;  f_k(w) = 1/2 |w|^2 + C sum_i max(0, 1 - y_i a_i.w)^2 with
 * a_i = [x_i, 1].  The matrices are row-major fp32 with leading dimension ld (ncol <= ld <= 64): W, G, S, R, P, T over the
 * D1 = D + 1 unknowns (row D the intercept), Z, AP, AS, V over the samples; the products Z = A W, AP = A P, AS = A S and
 * T = A^T V are the caller's (pdae_rows_gemm).  sc: PDAE_LINSVC_SC doubles per column = f, |g|, |g(0)|, eps, r^T r,
 * g^T s, the step taken, the line search's first step (the caller sets eps and the first step 1, zeros elsewhere);
 * fl: PDAE_LINSVC_FL ints per column = done, Newton steps, CG active, capped, stalled, Hessian products, CG steps of this
 * Newton step, failed line-search passes (zeros at the start).  A done column is skipped by every entry.  All sums have a
 * fixed order and there are no atomics: two runs give the same bits.
 *   linsvc_supported     host side, nothing launched: K < 2 classes, K > PDAE_LINSVC_MAX_CLASSES, empty input or a feature
 *                        matrix beyond the row GEMMs' reach: PDAE_ERR_UNSUPPORTED.
 *   linsvc_ones          A[r][col] = 1 for r < n: the intercept's column, set in the padding of the feature matrix.
 *   linsvc_residual      over `rows` >= n rows.  mode 0: V = y o r o act with r = 1 - y o Z, act = r > 0 (the gradient is
 *                        W - 2 C A^T V) and part[b][k] = the sum of r^2 over the active rows of row block b (64 rows; fp64);
 *                        mode 1: V = act o AP for the columns whose CG is active (a Hessian product is P + 2 C A^T V).
 *                        Rows >= n, columns >= ncol and skipped columns of V are written as zeros.
 *   linsvc_newton_begin  per column, from T = A^T V and the nb row blocks' part: f, G = W - 2 C T, |g|; done when
 *                        |g| <= eps |g(0)| (liblinear's rule: W starts at 0, so the first call's |g| is |g(0)|), capped
 *                        and done when max_newton steps were taken; else S = 0, R = P = -G, CG active.
 *   linsvc_cg_update     per column with CG active, from T = A^T (act o A P): alpha = r^T r / p^T H p, S += alpha P,
 *                        R -= alpha H P; CG ends when |r| <= xi |g| or after cg_max steps, else P = R + beta P.
 *   linsvc_linesearch    part[b][k][j] = the sum over row block b of max(0, 1 - y (Z + t AS))^2 at t = t0 2^-j, j = 0 .. 7.
 *   linsvc_step          per column: the first t of that sequence with f(w + t s) - f(w) <= eta t g^T s is taken,
 *                        W += t S; if none passes the next pass starts at t0 2^-8, and after four such passes (or when
 *                        g^T s >= 0) the column is stalled and done.  Counts a Newton step either way.
 *   linsvc_predict       pred[r] (int32) = the first column with the largest Z[r][k]; ncol == 1: Z[r][0] > 0 ? 1 : 0.     */
#define PDAE_LINSVC_MAX_CLASSES 64
#define PDAE_LINSVC_SC 8
#define PDAE_LINSVC_FL 8
int pdae_linsvc_supported(int n, int m, int D, int K);
int pdae_linsvc_ones(int n, int ld, int col, float* A, pdae_stream_t stream);
int pdae_linsvc_residual(int mode, int n, int rows, int ld, int ncol, int col0, const float* Z, const float* AP /*mode 1*/,
                         const int* labels, const int* fl, float* V, double* part /*mode 0*/, pdae_stream_t stream);
int pdae_linsvc_newton_begin(int D1, int ld, int ncol, int nb, double C, int max_newton, const float* W, const float* T,
                             const double* part, float* G, float* S, float* R, float* P, double* sc, int* fl,
                             pdae_stream_t stream);
int pdae_linsvc_cg_update(int D1, int ld, int ncol, double C, double xi, int cg_max, const float* T, float* S, float* R,
                          float* P, double* sc, int* fl, pdae_stream_t stream);
int pdae_linsvc_linesearch(int n, int ld, int ncol, int col0, const float* Z, const float* AS, const int* labels,
                           const double* sc, const int* fl, double* part, pdae_stream_t stream);
int pdae_linsvc_step(int D1, int ld, int ncol, int nb, double C, double eta, float* W, const float* S, const float* G,
                     const double* part, double* sc, int* fl, pdae_stream_t stream);
int pdae_linsvc_predict(int m, int ld, int ncol, const float* Z, int* pred, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Task-affinity protocol (csrc/affinity.hip; tools/runner_finetune.py:1198-1269 of the reference trains
 * nn.Linear(feat_dim, num_class) on the frozen encoder's features and reports the test cross-entropy and accuracy).
 *   linear_probe_train  trains W (K, D) and b (K) fp32 IN PLACE from their initial values on X (n x ld fp32, ld >= D)
 *                       and labels (n, 0 .. K - 1): `epochs` epochs of floor(n / PDAE_PROBE_BATCH) batches; step t
 *                       (global, from 1, running on across the epochs) takes the rows
 *                       perm[e][64 i .. 64 i + 63] (perm: device, epochs x n, every row a permutation of 0 .. n - 1; X is
 *                       gathered through it, never copied), logits = x W^T + b, loss = the mean cross-entropy of
 *                       the 64 rows, then torch.optim.AdamW's update in pdae_adamw_step's order with the decay on W and
 *                       b alike.  lr: HOST, `epochs` doubles, the learning rate of each epoch; the bias corrections
 *                       1 - beta^t are formed in fp64 on the host.  ONE launch per step (plus a prologue and a fill) on
 *                       `stream`, no host synchronisation and no wait between workgroups; every sum has a fixed order
 *                       and there are no atomics: two calls give the same bits.  workspace: linear_probe_workspace(D, K)
 *                       floats (the moments, the double-buffered partial logits and bias).  floor(n / 64) == 0 or
 *                       epochs == 0: nothing is launched, W and b are untouched.
 *                       K < 2, D < 1, ld < D, n < 0: PDAE_ERR_BAD_ARG; K > PDAE_PROBE_MAX_CLASSES: PDAE_ERR_UNSUPPORTED;
 *                       both before anything is launched (linear_probe_supported answers the same on the host).
 *   linear_probe_eval   on X (m x ld), labels (m): row_loss (m) fp32 = the rows' cross-entropies, row_pred (m) int32 =
 *                       argmax of the logits, ties to the lowest class; *loss_sum fp64 = the sum of row_loss and
 *                       *correct int32 = the rows with row_pred == label, both added in a fixed order;
 *                       logits (m, K), nullable.  Any m >= 1.                                                             */
#define PDAE_PROBE_MAX_CLASSES 64
#define PDAE_PROBE_BATCH 64
int pdae_linear_probe_supported(int n, int D, int ld, int K);
long long pdae_linear_probe_workspace(int D, int K);
int pdae_linear_probe_train(int n, int D, int ld, int K, int epochs, const float* X, const int32_t* labels,
                            const int32_t* perm, float* W, float* b, const double* lr /*host*/, double beta1, double beta2,
                            double eps, double weight_decay, float* workspace, pdae_stream_t stream);
int pdae_linear_probe_eval(int m, int D, int ld, int K, const float* X, const int32_t* labels, const float* W,
                           const float* b, float* row_loss, int32_t* row_pred, float* logits /*nullable*/,
                           double* loss_sum, int32_t* correct, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Voted evaluation (csrc/vote.hip; tools/runner_finetune.py:835-899 test_vote / :568-632 validate_vote of the reference:
 * per test batch `times` subsets of the FPS order, each through test_transforms and the model, the mean of the logits,
 * its argmax).
 *   vote_resample  pdae_resample_affine for all v votes of a batch in ONE launch:
 *                    out[k,b,n,j] = sum_i raw[b, fps_idx[b, choice[k,n]], i] * A[k,b,i,j] + t[k,b,j]      i, j in 0..2
 *                  raw (b,p,c) with c >= 3, fps_idx (b,point_all), choice (v,npoints): one subset per vote, shared by the
 *                  batch; A (v,b,3,3) and t (v,b,3) each nullable; out (v,b,npoints,3).  The arithmetic is
 *                  pdae_resample_affine's (the sum i = 0, 1, 2, then + t, every operation rounded; no map: the
 *                  coordinates are moved bit for bit; an index outside its array is not followed, that point is written
 *                  as NaN): the result equals v calls of it bit for bit.  Non-positive sizes, c < 3,
 *                  npoints > point_all, a null required pointer: PDAE_ERR_BAD_ARG; more blocks than one launch takes:
 *                  PDAE_ERR_UNSUPPORTED; both before anything is launched.
 *   vote_reduce    logits (v,b,k) fp32, labels (b) int64: per row the fp32 sum over the votes in the order 0 .. v-1,
 *                  divided by (float)v -> mean_out (b,k), nullable; pred_out (b) int64 = its argmax, ties to the lowest
 *                  class, -1 when a logit of the row is NaN; *correct (ONE int32) += the rows with pred == label (a row
 *                  of -1 and a label outside 0 .. k-1 never count).  One workgroup, a fixed order, no atomics: the count
 *                  is added with a plain load and store, so launches that share a counter must share a stream.  Any
 *                  b >= 1, v >= 1; v, b, k < 1 or a null required pointer: PDAE_ERR_BAD_ARG; k > PDAE_VOTE_MAX_CLASSES:
 *                  PDAE_ERR_UNSUPPORTED.                                                                                 */
#define PDAE_VOTE_MAX_CLASSES 64
int pdae_vote_resample(int v, int b, int p, int c, int point_all, int npoints, const float* raw, const int32_t* fps_idx,
                       const int32_t* choice, const float* A /*nullable*/, const float* t /*nullable*/, float* out,
                       pdae_stream_t stream);
int pdae_vote_reduce(int v, int b, int k, const float* logits, const int64_t* labels, float* mean_out /*nullable*/,
                     int64_t* pred_out, int32_t* correct, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * The training batch of a few-shot episode (csrc/fewshot.hip).
 * Replaces, per batch row, ModelNetFewShot.__getitem__ (datasets/ModelNetDatasetFewShot.py:59-71: the item and a fresh
 *   shuffle of its points) and the resample of tools/runner_finetune.py:158-176 (FPS to point_all points, a host draw of
 *   npoints of them, the gather) in ONE launch from the resident episode to the step's input.
 * set (s,p,c) f32 with c >= 3: the episode's clouds; item (b) i32: the cloud of each batch row; perm (b,p) i32: a
 *   permutation of 0..p-1 per row, nullable = the identity; slot (m) i32: the output row of FPS column j or -1,
 *   nullable = the identity (then npoints must equal m); out (b,npoints,3) f32; idx (b,m) i32, nullable.
 * With sh[b][k] = set[item[b]][perm[b][k]][0:3] and f = pdae_furthest_point_sampling of sh to m points (first index 0,
 *   the skipped-point rule, the tie order by the position k in the SHUFFLED cloud):
 *     idx[b][j] = perm[b][f[b][j]];   out[b][slot[j]] = sh[b][f[b][j]] for every j with 0 <= slot[j] < npoints.
 *   Coordinates are moved, not computed on: the result equals the existing entry on the materialised shuffle bit for
 *   bit, signed zeros included.  Rows of out that no slot names are left as they were.
 * Bad indices fault nothing: a perm entry outside 0..p-1 is not followed -- that position reads as the point (0,0,0),
 *   which the skipped-point rule never selects (idx still copies the entry); a slot outside 0..npoints-1 writes
 *   nothing; a row whose item is outside 0..s-1 gets out = NaN and idx = -1.  Two columns with one slot: either.
 * s, p <= 0, negative b / m / npoints, c < 3, m > p, slot == NULL with npoints != m, a null required pointer:
 *   PDAE_ERR_BAD_ARG; p > 8192: PDAE_ERR_UNSUPPORTED; b == 0 or m == 0: nothing to do.  All before anything is launched. */
int pdae_fewshot_batch(int s, int p, int c, int b, int m, int npoints, const float* set, const int32_t* item,
                       const int32_t* perm /*nullable*/, const int32_t* slot /*nullable*/, float* out,
                       int32_t* idx /*nullable*/, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * The augmented training batch of a resident labelled set (csrc/fewshot.hip; datasets.ModelNet on the reference's
 * processed ModelNet40 files).
 * Replaces, per batch row, ModelNet.__getitem__ (datasets/ModelNetDataset.py:127-158: the item, augment_data's per-access
 *   maps, a fresh shuffle of its points) and the resample of tools/runner_finetune.py:158-176 in ONE launch.
 * pdae_fewshot_batch with per-row affine maps in front of the FPS: nmaps (b) i32, nullable, and maps (b,3,12) f32 in
 *   pdae_pipeline_norm_affine's layout (M 3x3 row-major, then t).  With T_b = maps 0 .. nmaps[b]-1 of row b applied in
 *   order, each as x' = ((x*m00 + y*m10) + z*m20) + t0 (y', z' alike; every operation rounded, no contraction),
 *     sh[b][k] = T_b(set[item[b]][perm[b][k]][0:3]),
 *   and FPS, the skipped-point rule, the tie order, idx, slot and out are pdae_fewshot_batch's on sh: out holds the mapped
 *   coordinates.  nmaps == NULL: pdae_fewshot_batch bit for bit.  With maps: bit for bit the chain item select,
 *   permutation gather, pdae_pipeline_norm_affine(normalise = 0), pdae_fewshot_batch -- signed zeros included.
 * Bad indices fault nothing: as pdae_fewshot_batch (the (0,0,0) a bad perm entry reads as is NOT mapped and is never
 *   selected); a row whose nmaps is outside 0..3 gets out = NaN and idx = -1, like a row whose item is out of range.
 * Argument errors are pdae_fewshot_batch's; nmaps without maps: PDAE_ERR_BAD_ARG.  All before anything is launched. */
int pdae_resident_batch(int s, int p, int c, int b, int m, int npoints, const float* set, const int32_t* item,
                        const int32_t* perm /*nullable*/, const int32_t* nmaps /*nullable*/, const float* maps /*(b,3,12)*/,
                        const int32_t* slot /*nullable*/, float* out, int32_t* idx /*nullable*/, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Input-point gradients (csrc/input_grad.hip; tools/runner_finetune.py:751-833 vis_saliency_map of the reference, which
 * takes them from framework autograd one cloud at a time).  The two data-only backward steps that end at coordinates.
 *   group_points_backward  Group.forward's backward: neighbourhood[b,g,j] = xyz[b, knn_idx[b,g,j]] - center[b,g] and
 *                  center[b,g] = xyz[b, fps_idx[b,g]], so
 *                    d_xyz[b,n] = sum_{(g,j): knn_idx[b,g,j] == n} d_nbr[b,g,j]
 *                               + sum_{g: fps_idx[b,g] == n} (d_center[b,g] - sum_j d_nbr[b,g,j]).
 *                  d_nbr (b,g,k,3), d_center (b,g,3) nullable (= zeros), knn_idx (b,g,k) int64, fps_idx (b,g) int32 ->
 *                  d_xyz (b,n,3), every element written.  An ORDERED sum, no atomics: one thread owns a point and adds
 *                  its terms in ascending (g, j), then the centre terms in ascending g, each of them formed as
 *                  d_center - (the group's d_nbr added in ascending j); a point no index names gets exactly 0.0.  The
 *                  indices are only compared, never followed: one outside 0..n-1 contributes nothing.  The inverse map
 *                  is found by scanning the cloud's g*k indices, staged through LDS: n * g * k compares per cloud.
 *   rows_contract3 dx[row(m)][j] = sum_c d[m][c] * w[c][j], j = 0..2: the data gradient of a Linear / 1x1 conv with
 *                  three inputs (the embedder's first conv, the position embedding's first layer).  d (m,c) with
 *                  c % 4 == 0, c <= 1024; w (c,3) as stored (out, in); dx (n_out,3); row_ids (m) int64 nullable:
 *                  row(m) = row_ids[m] (distinct ids; an id outside 0..n_out-1 writes nothing; rows of dx no id names
 *                  are left as they were), else m (then n_out must equal m).  32 lanes share a row: lane
 *                  l adds channels 4l .. 4l+3 (+128, ...) in ascending order, then the lanes meet in a fixed butterfly.
 * Negative sizes, k or c out of range, a null required pointer: PDAE_ERR_BAD_ARG; more blocks than one launch takes:
 * PDAE_ERR_UNSUPPORTED; both before anything is launched.  Zero b, n or m: nothing to do.                          */
int pdae_group_points_backward(int b, int n, int g, int k, const float* d_nbr, const float* d_center /*nullable*/,
                               const int64_t* knn_idx, const int32_t* fps_idx, float* d_xyz, pdae_stream_t stream);
int pdae_rows_contract3(int m, int c, const float* d, const float* w, const int64_t* row_ids /*nullable*/, int n_out,
                        float* dx, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * The part-segmentation head in evaluation mode, forward only (csrc/partseg.hip; segmentation/models/pt.py:301-333 on
 * PointNetFeaturePropagation, segmentation/models/pointnet2_utils.py:262-312, and the metric of segmentation/main.py:246-295
 * of the reference; every BatchNorm as its running-estimate affine scale, shift).
 *   partseg_supported        1 when 3 <= G <= 256 centres per cloud, the propagated width C is a positive multiple of 4, the
 *                            tail's input width K is 256 and P is 50 part labels -- else 0; partseg_propagate / partseg_tail
 *                            return PDAE_ERR_UNSUPPORTED for every other layout before anything is read or launched.
 *   partseg_token_pool       F (B, G, C) -> out (B, 2C) = [max over G | mean over G] (the sum in token order, / G).
 *   partseg_propagate        pts (B, N, 3), centres (B, G, 3), T (B*G, C) = the first layer's feature columns applied once per
 *                            token (bias included), W0x (C, 3) its coordinate columns -> a0 (B*N, C) =
 *                            relu(scale0 (sum_k w_k T[b, idx_k] + W0x p) + shift0): idx_k the three nearest centres by
 *                            ((dx dx + dy dy) + dz dz), ties to the lower index; w_k = r_k / ((r_0 + r_1) + r_2),
 *                            r_k = 1 / (d_k + 1e-8).  idx3 (B, N, 3) int32 receives the indices, nearest first (nullable).
 *                            T, scale0, shift0, a0 16-byte aligned.
 *   partseg_cloud_bias_relu  y (B*N, C) <- relu(y + gbias[b]) in place, gbias (B, C); C a multiple of 4.
 *   partseg_tail             y (S*N, 256) -> logp (S*N, 50) fp32 = log_softmax(relu(y scale + shift) W3^T + b3) as
 *                            (x - max) - log sum exp(x - max); pred (S*N) int32 = the argmax of the stored logp over
 *                            [lo[s], hi[s]] (clamped to 0 .. 49; null lo / hi: the full range), first index on ties.  With
 *                            seg (S*N) int32 the counts are ADDED (int32, integer atomics: exact in any order) into
 *                            shape_iu (S, 2, 50) = per shape and label l of its range |pred = l and seg = l|, |pred = l or seg = l|;
 *                            shape_correct (S) = |pred = seg|; part_seen (50) = |seg = l|, part_correct (50) = |pred = seg = l|.
 *                            Null seg: no counts.  y, scale, shift, W3 16-byte aligned.                                         */
int pdae_partseg_supported(int G, int C, int K, int P);
int pdae_partseg_token_pool(int B, int G, int C, const float* F, float* out, pdae_stream_t stream);
int pdae_partseg_propagate(int B, int N, int G, int C, const float* pts, const float* centres, const float* T,
                           const float* W0x, const float* scale0, const float* shift0, float* a0,
                           int32_t* idx3 /*nullable*/, pdae_stream_t stream);
int pdae_partseg_cloud_bias_relu(int B, int N, int C, float* y, const float* gbias, pdae_stream_t stream);
int pdae_partseg_tail(int S, int N, int K, int P, const float* y, const float* scale, const float* shift, const float* W3,
                      const float* b3, const int32_t* seg /*nullable*/, const int32_t* lo /*nullable*/,
                      const int32_t* hi /*nullable*/, float* logp, int32_t* pred, int32_t* shape_iu /*with seg*/,
                      int32_t* shape_correct, int32_t* part_seen, int32_t* part_correct, pdae_stream_t stream);

/* The DGCNN part-segmentation head (segmentation/models/dgcnn_partseg.py:124-140), the same file:
 *   partseg_cloud_bias_lrelu y (B*N, C) <- lrelu(y + gbias[b]) in place (z > 0 ? z : slope z), gbias (B, C); C a multiple of 4.
 *   partseg_logits_tail      y (S*N, 128) -> logits (S*N, 50) fp32 = lrelu(y scale + shift) W^T (+ bias, nullable), RAW (no
 *                            log-softmax); pred = the argmax of the stored logits over [lo[s], hi[s]] as partseg_tail, first
 *                            index on ties; the counts are partseg_tail's.  K = 128 and P = 50, else PDAE_ERR_UNSUPPORTED
 *                            before anything is read or launched.  y, scale, shift, W 16-byte aligned. */
int pdae_partseg_cloud_bias_lrelu(int B, int N, int C, float* y, const float* gbias, float slope, pdae_stream_t stream);
int pdae_partseg_logits_tail(int S, int N, int K, int P, const float* y, const float* scale, const float* shift, float slope,
                             const float* W, const float* bias /*nullable*/, const int32_t* seg /*nullable*/,
                             const int32_t* lo /*nullable*/, const int32_t* hi /*nullable*/, float* logits, int32_t* pred,
                             int32_t* shape_iu /*with seg*/, int32_t* shape_correct, int32_t* part_seen,
                             int32_t* part_correct, pdae_stream_t stream);

/* A TWO-layer EdgeConv in EVALUATION mode, forward only, as one kernel (csrc/edge2_eval.hip; the first two EdgeConvs of
 * segmentation/models/dgcnn_util.py:140-193 dgcnn_encoder_partseg, every BatchNorm2d as its running-estimate affine):
 *   out[r][c] = max over j of lrelu(scale2[c] (W2[c,:] . h[r][j][:]) + shift2[c])
 *   h[r][j][:] = lrelu(scale1 (p[b n + idx[r][j]] + q[r]) + shift1),   slope 0.2
 * pq (b n, 2 C1) = [p | q] = x [W1; W2 - W1]^T, the first layer applied once per point by the caller (edge_weight_stack +
 * the row GEMM); idx (b, n, k) int32 ids within the cloud (one outside it is clamped, not followed); W2 (C2, C1).  The per-edge
 * activation h exists only in LDS; the product runs on fp32-input MFMA tiles (one fp32 fma chain per output in the fixed order
 * k = 0, 4, 1, 5, 2, 6, 3, 7 within every eight); the max starts
 * from the first edge, j ascending, no atomics.  out (b n, C2); out2 (nullable, row stride ld2 >= C2): a second copy into a
 * wider row-major tensor, as bn_lrelu_rows.  edge2_eval_supported: 1 for 1 <= k <= 32 and C1 = C2 = 64, else 0;
 * edge2_eval_forward returns PDAE_ERR_UNSUPPORTED for every other layout before anything is read or launched.
 * pq, scale1, shift1, W2 16-byte aligned. */
int pdae_edge2_eval_supported(int k, int C1, int C2);
int pdae_edge2_eval_forward(int b, int n, int k, int C1, int C2, const float* pq, const int32_t* idx, const float* scale1,
                            const float* shift1, const float* W2, const float* scale2, const float* shift2, float* out,
                            float* out2 /*nullable*/, int ld2, pdae_stream_t stream);

/* ------------------------------------------------------------------------
 * Measurement aids: box calibration for bench.py (csrc/calib.hip). They replace nothing of the reference; the training
 * step never calls them.  MI355X boxes differ by +-4 % on the step and by up to 12 % on matrix loops (the clock a device
 * holds under load), so a bench line carries the rates of two kernels of known work next to its headline.
 *   calib_mfma_bf16  `blocks` work-groups of 4 waves (one per SIMD) each issue iters x 32 v_mfma_f32_32x32x16_bf16 on
 *                    pseudo-random register operands: *flops (host, nullable) = the FLOPs of the launch; clk[b][0..1] =
 *                    shader-clock cycles and 100 MHz ticks wave 0 of block b lived (clock = 100 MHz x cycles / ticks).
 *   calib_copy       dst[0..bytes) = src[0..bytes), 16 B per lane, grid-stride: 2 x bytes of HBM traffic.            */
int pdae_calib_mfma_bf16(int blocks, int iters, float* sink, long long* clk, double* flops, pdae_stream_t stream);
int pdae_calib_copy(long long bytes, const void* src, void* dst, pdae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDAE_H */
