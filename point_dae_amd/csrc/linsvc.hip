// linsvc.hip -- the pretraining validation's classifier (tools/runner_pretrain.py:25-48 of the reference fits
// sklearn.svm.LinearSVC(): liblinear's L2-regularised squared-hinge one-vs-rest machines with a regularised intercept) on
// gfx950: a truncated-Newton solver of ALL one-vs-rest problems at once, in the primal.
//
// Problem of column k (class col0 + k; y_i = +1 when label_i is that class, else -1; a_i = [x_i, 1]):
//     f_k(w) = 1/2 |w|^2 + C sum_i max(0, 1 - y_i a_i.w)^2
//     g = w - 2 C A^T (y o r o act),   r = 1 - y o (A w),  act = r > 0
//     H = I + 2 C A^T diag(act) A
// The unknowns are the columns of W (rows x ld fp32, row D = the intercept).  The products A W, A P, A S and A^T V are the
// row GEMMs' (point_dae_amd/linsvc_ops.py); the kernels here are everything between them, each ONE launch for all columns:
//   residual    (rows x columns)  V = y o r o act and the loss partials (mode 0), V = act o (A P) (mode 1)
//   newton_begin (a block per column)  f, g, |g|, the stopping test, the start of conjugate gradients
//   cg_update   (a block per column)  one conjugate-gradient step on H s = -g
//   linesearch  (rows x columns)  the loss partials of f(w + t s) at t = t0 2^-j, j = 0 .. 7, from Z and A S
//   step        (a block per column)  the first t of that halving sequence that passes Armijo's test; W += t S
//   predict     argmax over the columns of a decision row, ties to the lowest column
// The per-column scalars (f, |g|, r^T r, g^T s, t0) live in `sc` (fp64) and the flags (done, Newton steps, CG active,
// capped, stalled) in `fl`: the host reads `fl` once per round of launches, never per step.  A column that is done is
// skipped by every kernel, so it stops moving while the others go on.
//
// Every sum has a fixed order: a thread adds its rows (its vector entries) in ascending order, the four row groups of a
// block (the lanes of a wave, then the four waves) are added in a fixed tree, the row blocks' partials go through memory
// and are added the same way by the column's block.  No atomics: two runs give the same bits.
#include "common.h"

namespace pdae {
namespace {

constexpr int LS_ROWS = 64;                // rows of a row block (residual, linesearch)
constexpr int LS_RY = 4;                   // row groups of a row block: blockDim = (64 columns, 4)
constexpr int LS_T = 8;                    // step sizes one line-search pass tries
constexpr int LS_MAX_FAILS = 4;            // passes without an acceptable step before the column is stalled (t < 2^-32)
constexpr int VEC_THREADS = 256;
constexpr int VEC_WAVES = VEC_THREADS / kWave;

// sc (fp64, PDAE_LINSVC_SC per column) and fl (int, PDAE_LINSVC_FL per column): include/pdae.h
enum { SC_F = 0, SC_GNORM, SC_GNORM0, SC_EPS, SC_RR, SC_GS, SC_T, SC_T0 };
enum { FL_DONE = 0, FL_NEWTON, FL_CG_ACTIVE, FL_CAPPED, FL_STALLED, FL_HV, FL_CG_ITERS, FL_LS_FAILS };

// sums of N values over a block of 256 threads, the same result in every thread: lanes by butterfly, then the waves in order
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double (*s_red)[N]) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int c = 0; c < N; ++c) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[c] += __shfl_xor(v[c], o, kWave);
  }
  __syncthreads();                                     // (s_red may still be read from the previous sum)
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < N; ++c) s_red[wave][c] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; ++c) {
    double t = s_red[0][c];
#pragma unroll
    for (int w = 1; w < VEC_WAVES; ++w) t += s_red[w][c];
    v[c] = t;
  }
}

__global__ __launch_bounds__(VEC_THREADS) void linsvc_ones_kernel(int n, int ld, int col, float* __restrict__ A) {
  const int r = blockIdx.x * VEC_THREADS + threadIdx.x;
  if (r < n) A[(size_t)r * ld + col] = 1.0f;
}

// blockDim (64, 4): x = column, y = row group; a block owns LS_ROWS rows of the (rows, ld) matrices
__global__ __launch_bounds__(kWave * LS_RY) void linsvc_residual_kernel(
    int mode, int n, int rows, int ld, int ncol, int col0, const float* __restrict__ Z, const float* __restrict__ AP,
    const int* __restrict__ labels, const int* __restrict__ fl, float* __restrict__ V, double* __restrict__ part) {
  __shared__ double s_loss[LS_RY][kWave];
  const int c = threadIdx.x, ry = threadIdx.y;
  const int r0 = blockIdx.x * LS_ROWS;
  const bool col_ok = c < ncol;
  bool live = false;
  if (col_ok) live = mode == 0 ? fl[c * PDAE_LINSVC_FL + FL_DONE] == 0 : fl[c * PDAE_LINSVC_FL + FL_CG_ACTIVE] != 0;
  double loss = 0.0;
  for (int i = ry; i < LS_ROWS; i += LS_RY) {
    const int r = r0 + i;
    if (r >= rows) break;
    if (c >= ld) continue;
    const size_t o = (size_t)r * ld + c;
    float v = 0.0f;
    if (live && r < n) {
      const float y = labels[r] == c + col0 ? 1.0f : -1.0f;
      const float res = 1.0f - y * Z[o];
      if (res > 0.0f) {
        if (mode == 0) {
          v = y * res;
          loss += (double)res * (double)res;
        } else {
          v = AP[o];
        }
      }
    }
    V[o] = v;                                          // the padding rows and columns are written too: zeros
  }
  if (mode != 0) return;
  s_loss[ry][c] = loss;
  __syncthreads();
  if (ry == 0 && col_ok) {
    double t = s_loss[0][c];
#pragma unroll
    for (int g = 1; g < LS_RY; ++g) t += s_loss[g][c];
    part[(size_t)blockIdx.x * ld + c] = t;
  }
}

__global__ __launch_bounds__(kWave * LS_RY) void linsvc_linesearch_kernel(
    int n, int ld, int ncol, int col0, const float* __restrict__ Z, const float* __restrict__ AS,
    const int* __restrict__ labels, const double* __restrict__ sc, const int* __restrict__ fl, double* __restrict__ part) {
  __shared__ double s_loss[LS_RY][kWave][LS_T];
  const int c = threadIdx.x, ry = threadIdx.y;
  const int r0 = blockIdx.x * LS_ROWS;
  const bool live = c < ncol && fl[(c < ncol ? c : 0) * PDAE_LINSVC_FL + FL_DONE] == 0;
  double acc[LS_T];
#pragma unroll
  for (int j = 0; j < LS_T; ++j) acc[j] = 0.0;
  if (live) {
    const double t0 = sc[c * PDAE_LINSVC_SC + SC_T0];
    for (int i = ry; i < LS_ROWS; i += LS_RY) {
      const int r = r0 + i;
      if (r >= n) break;
      const size_t o = (size_t)r * ld + c;
      const double y = labels[r] == c + col0 ? 1.0 : -1.0;
      const double z = (double)Z[o], d = (double)AS[o];
      double t = t0;
#pragma unroll
      for (int j = 0; j < LS_T; ++j) {
        const double res = 1.0 - y * (z + t * d);
        if (res > 0.0) acc[j] += res * res;
        t *= 0.5;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < LS_T; ++j) s_loss[ry][c][j] = acc[j];
  __syncthreads();
  if (ry == 0 && c < ncol) {
#pragma unroll
    for (int j = 0; j < LS_T; ++j) {
      double t = s_loss[0][c][j];
#pragma unroll
      for (int g = 1; g < LS_RY; ++g) t += s_loss[g][c][j];
      part[((size_t)blockIdx.x * ld + c) * LS_T + j] = t;
    }
  }
}

// one block per column
__global__ __launch_bounds__(VEC_THREADS) void linsvc_newton_begin_kernel(
    int D1, int ld, int nb, double C, int max_newton, const float* __restrict__ W, const float* __restrict__ T,
    const double* __restrict__ part, float* __restrict__ G, float* __restrict__ S, float* __restrict__ R,
    float* __restrict__ P, double* __restrict__ sc, int* __restrict__ fl) {
  __shared__ double s_red[VEC_WAVES][3];
  const int k = blockIdx.x, tid = threadIdx.x;
  double* __restrict__ sck = sc + (size_t)k * PDAE_LINSVC_SC;
  int* __restrict__ flk = fl + (size_t)k * PDAE_LINSVC_FL;
  if (flk[FL_DONE] != 0) return;                       // (block-uniform: written only by this column's blocks, in earlier launches)
  double v[3] = {0.0, 0.0, 0.0};                       // loss, w^T w, g^T g
  for (int b = tid; b < nb; b += VEC_THREADS) v[0] += part[(size_t)b * ld + k];
  const double twoC = 2.0 * C;
  for (int j = tid; j < D1; j += VEC_THREADS) {
    const size_t o = (size_t)j * ld + k;
    const double w = (double)W[o];
    const float g = (float)(w - twoC * (double)T[o]);
    G[o] = g;
    v[1] += w * w;
    v[2] += (double)g * (double)g;
  }
  block_sum<3>(v, s_red);
  const double f = 0.5 * v[1] + C * v[0], gnorm = sqrt(v[2]);
  const int newton = flk[FL_NEWTON];
  const double gnorm0 = newton == 0 ? gnorm : sck[SC_GNORM0];
  const bool converged = gnorm <= sck[SC_EPS] * gnorm0;       // liblinear: |g| <= eps |g(0)|, W starts at 0
  const bool capped = !converged && newton >= max_newton;
  __syncthreads();                                     // (every thread has read the flags and scalars it decides on)
  if (tid == 0) {
    sck[SC_F] = f;
    sck[SC_GNORM] = gnorm;
    sck[SC_GNORM0] = gnorm0;
    sck[SC_RR] = v[2];
    flk[FL_CG_ITERS] = 0;
    flk[FL_CG_ACTIVE] = converged || capped ? 0 : 1;
    if (capped) flk[FL_CAPPED] = 1;
    if (converged || capped) flk[FL_DONE] = 1;
  }
  if (converged || capped) return;
  for (int j = tid; j < D1; j += VEC_THREADS) {
    const size_t o = (size_t)j * ld + k;
    const float g = G[o];                              // (this thread's own store)
    S[o] = 0.0f;
    R[o] = -g;
    P[o] = -g;
  }
}

__global__ __launch_bounds__(VEC_THREADS) void linsvc_cg_update_kernel(
    int D1, int ld, double C, double xi, int cg_max, const float* __restrict__ T, float* __restrict__ S,
    float* __restrict__ R, float* __restrict__ P, double* __restrict__ sc, int* __restrict__ fl) {
  __shared__ double s_red[VEC_WAVES][1];
  const int k = blockIdx.x, tid = threadIdx.x;
  double* __restrict__ sck = sc + (size_t)k * PDAE_LINSVC_SC;
  int* __restrict__ flk = fl + (size_t)k * PDAE_LINSVC_FL;
  if (flk[FL_CG_ACTIVE] == 0) return;
  const double twoC = 2.0 * C, rr = sck[SC_RR], gnorm = sck[SC_GNORM];
  const int iters = flk[FL_CG_ITERS] + 1;
  double v[1] = {0.0};                                 // p^T H p,  H p = p + 2 C A^T (act o A p)
  for (int j = tid; j < D1; j += VEC_THREADS) {
    const size_t o = (size_t)j * ld + k;
    const double p = (double)P[o];
    v[0] += p * (p + twoC * (double)T[o]);
  }
  block_sum<1>(v, s_red);
  const double php = v[0];
  if (!(php > 0.0)) {                                  // p = 0, or not a number: the step so far stands
    __syncthreads();
    if (tid == 0) flk[FL_CG_ACTIVE] = 0;
    return;
  }
  const double alpha = rr / php;
  v[0] = 0.0;
  for (int j = tid; j < D1; j += VEC_THREADS) {
    const size_t o = (size_t)j * ld + k;
    const double p = (double)P[o];
    const float r = (float)((double)R[o] - alpha * (p + twoC * (double)T[o]));
    S[o] = (float)((double)S[o] + alpha * p);
    R[o] = r;
    v[0] += (double)r * (double)r;
  }
  block_sum<1>(v, s_red);
  const double rr_new = v[0];
  const bool stop = sqrt(rr_new) <= xi * gnorm || iters >= cg_max;
  if (!stop) {
    const double beta = rr_new / rr;
    for (int j = tid; j < D1; j += VEC_THREADS) {
      const size_t o = (size_t)j * ld + k;
      P[o] = (float)((double)R[o] + beta * (double)P[o]);
    }
  }
  __syncthreads();
  if (tid == 0) {
    sck[SC_RR] = rr_new;
    flk[FL_CG_ITERS] = iters;
    flk[FL_HV] += 1;
    if (stop) flk[FL_CG_ACTIVE] = 0;
  }
}

__global__ __launch_bounds__(VEC_THREADS) void linsvc_step_kernel(
    int D1, int ld, int nb, double C, double eta, float* __restrict__ W, const float* __restrict__ S,
    const float* __restrict__ G, const double* __restrict__ part, double* __restrict__ sc, int* __restrict__ fl) {
  __shared__ double s_red[VEC_WAVES][4 + LS_T];
  const int k = blockIdx.x, tid = threadIdx.x;
  double* __restrict__ sck = sc + (size_t)k * PDAE_LINSVC_SC;
  int* __restrict__ flk = fl + (size_t)k * PDAE_LINSVC_FL;
  if (flk[FL_DONE] != 0) return;
  double v[4 + LS_T];                                  // g^T s, w^T s, s^T s, w^T w, the LS_T losses
#pragma unroll
  for (int c = 0; c < 4 + LS_T; ++c) v[c] = 0.0;
  for (int j = tid; j < D1; j += VEC_THREADS) {
    const size_t o = (size_t)j * ld + k;
    const double w = (double)W[o], s = (double)S[o], g = (double)G[o];
    v[0] += g * s;
    v[1] += w * s;
    v[2] += s * s;
    v[3] += w * w;
  }
  for (int b = tid; b < nb; b += VEC_THREADS) {
    const double* __restrict__ pb = part + ((size_t)b * ld + k) * LS_T;
#pragma unroll
    for (int j = 0; j < LS_T; ++j) v[4 + j] += pb[j];
  }
  block_sum<4 + LS_T>(v, s_red);
  const double gs = v[0], f0 = sck[SC_F], t0 = sck[SC_T0];
  const int fails = flk[FL_LS_FAILS];
  double t = t0, taken = 0.0;
  if (gs < 0.0) {                                      // (conjugate gradients from s = 0 on a positive definite H descend)
#pragma unroll
    for (int j = 0; j < LS_T; ++j) {
      const double f = 0.5 * (v[3] + 2.0 * t * v[1] + t * t * v[2]) + C * v[4 + j];
      if (taken == 0.0 && f - f0 <= eta * t * gs) taken = t;
      t *= 0.5;
    }
  }
  if (taken != 0.0) {
    for (int j = tid; j < D1; j += VEC_THREADS) {
      const size_t o = (size_t)j * ld + k;
      W[o] = (float)((double)W[o] + taken * (double)S[o]);
    }
  }
  __syncthreads();
  if (tid == 0) {
    sck[SC_GS] = gs;
    sck[SC_T] = taken;
    flk[FL_NEWTON] += 1;
    if (taken != 0.0) {
      sck[SC_T0] = 1.0;
      flk[FL_LS_FAILS] = 0;
    } else if (!(gs < 0.0) || fails + 1 >= LS_MAX_FAILS) {
      flk[FL_STALLED] = 1;                             // no step of the sequence lowers f: the products' rounding floor
      flk[FL_DONE] = 1;
    } else {
      sck[SC_T0] = t;                                  // = t0 2^-LS_T: the next pass goes on halving
      flk[FL_LS_FAILS] = fails + 1;
    }
  }
}

__global__ __launch_bounds__(VEC_THREADS) void linsvc_predict_kernel(int m, int ld, int ncol, const float* __restrict__ Z,
                                                                      int* __restrict__ pred) {
  const int r = blockIdx.x * VEC_THREADS + threadIdx.x;
  if (r >= m) return;
  const float* __restrict__ z = Z + (size_t)r * ld;
  int best = 0;
  if (ncol == 1) {
    best = z[0] > 0.0f ? 1 : 0;                        // the binary machine: its one column is the SECOND class
  } else {
    float zb = z[0];
    for (int k = 1; k < ncol; ++k) {
      const float v = z[k];
      if (v > zb) zb = v, best = k;                    // strict: ties stay with the lowest column (numpy.argmax)
    }
  }
  pred[r] = best;
}

int check_cols(const char* what, int ld, int ncol) {
  if (ncol < 1 || ncol > PDAE_LINSVC_MAX_CLASSES || ld < ncol || ld > kWave) {
    set_error(what);
    return PDAE_ERR_UNSUPPORTED;
  }
  return PDAE_OK;
}

}  // namespace
}  // namespace pdae

using namespace pdae;

extern "C" int pdae_linsvc_supported(int n, int m, int D, int K) {
  if (n < 1 || m < 1 || D < 1) return unsupported("linsvc: empty input (n, m and D must be at least 1)");
  if (K < 2) return unsupported("linsvc: the number of classes has to be greater than one");
  if (K > PDAE_LINSVC_MAX_CLASSES) return unsupported("linsvc: more than PDAE_LINSVC_MAX_CLASSES (64) classes");
  if ((long long)(n + 31) * (D + 32) >= (1LL << 30) || (long long)(m + 31) * (D + 32) >= (1LL << 30))
    return unsupported("linsvc: a feature matrix of 4 GB or more (the row GEMMs' 32-bit byte offsets)");
  return PDAE_OK;
}

extern "C" int pdae_linsvc_ones(int n, int ld, int col, float* A, pdae_stream_t stream) {
  if (n < 1 || col < 0 || col >= ld || !A) return bad_arg("linsvc_ones: n >= 1, 0 <= col < ld and A required");
  hipLaunchKernelGGL(linsvc_ones_kernel, dim3((n + VEC_THREADS - 1) / VEC_THREADS), dim3(VEC_THREADS), 0, as_stream(stream), n,
                     ld, col, A);
  return check_launch("linsvc_ones");
}

extern "C" int pdae_linsvc_residual(int mode, int n, int rows, int ld, int ncol, int col0, const float* Z, const float* AP,
                                    const int* labels, const int* fl, float* V, double* part, pdae_stream_t stream) {
  if (mode < 0 || mode > 1 || n < 1 || rows < n || col0 < 0) return bad_arg("linsvc_residual: mode 0 | 1, 1 <= n <= rows required");
  const int rc = check_cols("linsvc_residual: 1 <= ncol <= ld <= PDAE_LINSVC_MAX_CLASSES (64) columns", ld, ncol);
  if (rc != PDAE_OK) return rc;
  if (!Z || !labels || !fl || !V || (mode == 0 ? !part : !AP)) return bad_arg("linsvc_residual: null pointer");
  hipLaunchKernelGGL(linsvc_residual_kernel, dim3((rows + LS_ROWS - 1) / LS_ROWS), dim3(kWave, LS_RY), 0, as_stream(stream), mode,
                     n, rows, ld, ncol, col0, Z, AP, labels, fl, V, part);
  return check_launch("linsvc_residual");
}

extern "C" int pdae_linsvc_newton_begin(int D1, int ld, int ncol, int nb, double C, int max_newton, const float* W,
                                        const float* T, const double* part, float* G, float* S, float* R, float* P,
                                        double* sc, int* fl, pdae_stream_t stream) {
  if (D1 < 2 || nb < 1 || !(C > 0.0) || max_newton < 1)
    return bad_arg("linsvc_newton_begin: D1 >= 2, nb >= 1, C > 0 and max_newton >= 1 required");
  const int rc = check_cols("linsvc_newton_begin: 1 <= ncol <= ld <= PDAE_LINSVC_MAX_CLASSES (64) columns", ld, ncol);
  if (rc != PDAE_OK) return rc;
  if (!W || !T || !part || !G || !S || !R || !P || !sc || !fl) return bad_arg("linsvc_newton_begin: null pointer");
  hipLaunchKernelGGL(linsvc_newton_begin_kernel, dim3(ncol), dim3(VEC_THREADS), 0, as_stream(stream), D1, ld, nb, C, max_newton,
                     W, T, part, G, S, R, P, sc, fl);
  return check_launch("linsvc_newton_begin");
}

extern "C" int pdae_linsvc_cg_update(int D1, int ld, int ncol, double C, double xi, int cg_max, const float* T, float* S,
                                     float* R, float* P, double* sc, int* fl, pdae_stream_t stream) {
  if (D1 < 2 || !(C > 0.0) || !(xi > 0.0) || cg_max < 1)
    return bad_arg("linsvc_cg_update: D1 >= 2, C > 0, xi > 0 and cg_max >= 1 required");
  const int rc = check_cols("linsvc_cg_update: 1 <= ncol <= ld <= PDAE_LINSVC_MAX_CLASSES (64) columns", ld, ncol);
  if (rc != PDAE_OK) return rc;
  if (!T || !S || !R || !P || !sc || !fl) return bad_arg("linsvc_cg_update: null pointer");
  hipLaunchKernelGGL(linsvc_cg_update_kernel, dim3(ncol), dim3(VEC_THREADS), 0, as_stream(stream), D1, ld, C, xi, cg_max, T, S,
                     R, P, sc, fl);
  return check_launch("linsvc_cg_update");
}

extern "C" int pdae_linsvc_linesearch(int n, int ld, int ncol, int col0, const float* Z, const float* AS, const int* labels,
                                      const double* sc, const int* fl, double* part, pdae_stream_t stream) {
  if (n < 1 || col0 < 0) return bad_arg("linsvc_linesearch: n >= 1 required");
  const int rc = check_cols("linsvc_linesearch: 1 <= ncol <= ld <= PDAE_LINSVC_MAX_CLASSES (64) columns", ld, ncol);
  if (rc != PDAE_OK) return rc;
  if (!Z || !AS || !labels || !sc || !fl || !part) return bad_arg("linsvc_linesearch: null pointer");
  hipLaunchKernelGGL(linsvc_linesearch_kernel, dim3((n + LS_ROWS - 1) / LS_ROWS), dim3(kWave, LS_RY), 0, as_stream(stream), n, ld,
                     ncol, col0, Z, AS, labels, sc, fl, part);
  return check_launch("linsvc_linesearch");
}

extern "C" int pdae_linsvc_step(int D1, int ld, int ncol, int nb, double C, double eta, float* W, const float* S, const float* G,
                                const double* part, double* sc, int* fl, pdae_stream_t stream) {
  if (D1 < 2 || nb < 1 || !(C > 0.0) || !(eta > 0.0 && eta < 1.0))
    return bad_arg("linsvc_step: D1 >= 2, nb >= 1, C > 0 and 0 < eta < 1 required");
  const int rc = check_cols("linsvc_step: 1 <= ncol <= ld <= PDAE_LINSVC_MAX_CLASSES (64) columns", ld, ncol);
  if (rc != PDAE_OK) return rc;
  if (!W || !S || !G || !part || !sc || !fl) return bad_arg("linsvc_step: null pointer");
  hipLaunchKernelGGL(linsvc_step_kernel, dim3(ncol), dim3(VEC_THREADS), 0, as_stream(stream), D1, ld, nb, C, eta, W, S, G, part,
                     sc, fl);
  return check_launch("linsvc_step");
}

extern "C" int pdae_linsvc_predict(int m, int ld, int ncol, const float* Z, int* pred, pdae_stream_t stream) {
  if (m < 1) return bad_arg("linsvc_predict: m >= 1 required");
  const int rc = check_cols("linsvc_predict: 1 <= ncol <= ld <= PDAE_LINSVC_MAX_CLASSES (64) columns", ld, ncol);
  if (rc != PDAE_OK) return rc;
  if (!Z || !pred) return bad_arg("linsvc_predict: null pointer");
  hipLaunchKernelGGL(linsvc_predict_kernel, dim3((m + VEC_THREADS - 1) / VEC_THREADS), dim3(VEC_THREADS), 0, as_stream(stream), m,
                     ld, ncol, Z, pred);
  return check_launch("linsvc_predict");
}
