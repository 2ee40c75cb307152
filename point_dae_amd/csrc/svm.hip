// svm.hip -- the linear-SVM evaluation protocol's classifier (tools/runner_finetune.py:1038-1049 of the reference:
// sklearn.svm.SVC(C=c, kernel='linear') for six values of C) on gfx950: every one-vs-one dual problem of every C in ONE
// launch, decisions and votes in another.
//
// Training.  libsvm's C-SVC dual of a class pair (p, q), p < q, members t = the samples of p (y = +1) then of q (y = -1):
//     min 1/2 a^T Q a - e^T a,   0 <= a <= C,   y^T a = 0,   Q_st = y_s y_t K_st,   K = the Gram matrix X X^T.
// One workgroup per (pair, C).  alpha and the gradient g = Q a - e live in LDS as fp64, one slot per member, beside the
// member's row of the Gram matrix (its global sample index) and K_tt.  An iteration is SMO on the maximal violating pair
// (Keerthi et al.; libsvm's working-set rule before its second-order one):
//     up  = {y > 0, a < C} u {y < 0, a > 0},  low = {y > 0, a > 0} u {y < 0, a < C}
//     i = argmax_up(-y g),  j = argmin_low(-y g),  stop when (-y g)_i - (-y g)_j < eps
//     step s = ((-y g)_i - (-y g)_j) / (K_ii + K_jj - 2 K_ij) along a_i += y_i s, a_j -= y_j s, clipped to the box (a
//     clipped end is SET to its bound), g_t += y_t s (K_ti - K_tj).
// Every thread owns the members t = tid, tid + 256, ...: it alone reads and writes their alpha and gradient, so the one
// barrier of an iteration is the selection's (wave butterfly, then the four waves' candidates through a double-buffered
// LDS record that also carries alpha_i / alpha_j to everybody).  Ties go to the lowest member index: the comparison is a
// total order, so the butterfly's result does not depend on its shape and two runs give the same bits.  The Gram entries
// of an iteration are rows i and j of G at the members' columns: two gathers of an L2-resident line.
// rho is libsvm's calculate_rho: the mean of y g over the free members, else the midpoint of the bounds the members
// at 0 / C leave.  The loop is bounded by max_iter; a problem that hits it says so in its status.
//
// Prediction.  One workgroup per (test row, C): the row of the test-by-train Gram is staged in LDS in class order, a wave
// per pair adds coef * K over the pair's members (lane-strided fp64 partial sums, butterfly: a fixed order), the votes are
// libsvm's (dec > 0: the pair's first class; the first class with the most votes).
#include "common.h"

namespace pdae {
namespace {

constexpr int SVM_THREADS = 256;
constexpr int SVM_WAVES = SVM_THREADS / kWave;
constexpr int SVM_MAX_MEMBERS = PDAE_SVM_MAX_PAIR;
constexpr int SVM_MAX_CLASSES = PDAE_SVM_MAX_CLASSES;
constexpr int SVM_MAX_C = PDAE_SVM_MAX_C;
constexpr int SVM_PRED_MAX_N = PDAE_SVM_PREDICT_MAX_TRAIN;
constexpr double SVM_TAU = 1e-12;           // libsvm's TAU: the curvature a non-positive K_ii + K_jj - 2 K_ij is replaced by

struct SvmLayout {
  int class_ptr[SVM_MAX_CLASSES + 1];
  double C[SVM_MAX_C];
};

struct Cand {          // a selection candidate: the key -y g, the member and its alpha
  double key, alpha;
  int t;
};

// the total orders of the two selections: larger (smaller) key first, then the lower member index; t < 0: no candidate
__device__ __forceinline__ bool better_up(const Cand& a, const Cand& b) {
  if (a.t < 0 || b.t < 0) return b.t < 0 && a.t >= 0;
  return a.key > b.key || (a.key == b.key && a.t < b.t);
}
__device__ __forceinline__ bool better_low(const Cand& a, const Cand& b) {
  if (a.t < 0 || b.t < 0) return b.t < 0 && a.t >= 0;
  return a.key < b.key || (a.key == b.key && a.t < b.t);
}

__device__ __forceinline__ Cand shfl_xor_cand(const Cand& c, int o) {
  Cand r;
  r.key = __shfl_xor(c.key, o, kWave);
  r.alpha = __shfl_xor(c.alpha, o, kWave);
  r.t = __shfl_xor(c.t, o, kWave);
  return r;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmin(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, kWave));
  return v;
}

__device__ __forceinline__ void pair_of(int pair, int K, int& p, int& q) {
  p = 0;
  int left = pair;
  while (left >= K - 1 - p) {
    left -= K - 1 - p;
    ++p;
  }
  q = p + 1 + left;
}

__global__ __launch_bounds__(SVM_THREADS) void svm_ovo_train_kernel(
    int n, int ld, int K, int P, const float* __restrict__ G, const int* __restrict__ order, SvmLayout lay, double eps,
    int max_iter, double* __restrict__ coef, double* __restrict__ rho, int* __restrict__ status, double* __restrict__ gap_out) {
  __shared__ double s_alpha[SVM_MAX_MEMBERS];
  __shared__ double s_grad[SVM_MAX_MEMBERS];
  __shared__ int s_row[SVM_MAX_MEMBERS];
  __shared__ float s_diag[SVM_MAX_MEMBERS];
  __shared__ Cand s_up[2][SVM_WAVES], s_low[2][SVM_WAVES];
  __shared__ double s_red[3][SVM_WAVES];
  __shared__ int s_free[SVM_WAVES];

  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int pair = blockIdx.x, ci = blockIdx.y;
  int p, q;
  pair_of(pair, K, p, q);
  const int p0 = lay.class_ptr[p], np = lay.class_ptr[p + 1] - p0;
  const int q0 = lay.class_ptr[q], nq = lay.class_ptr[q + 1] - q0;
  const int nm = np + nq;                         // <= SVM_MAX_MEMBERS (checked by the host entry)
  const double C = lay.C[ci];

  for (int t = tid; t < nm; t += SVM_THREADS) {
    const int row = order[t < np ? p0 + t : q0 + (t - np)];
    s_row[t] = row;
    s_diag[t] = G[(size_t)row * ld + row];
    s_alpha[t] = 0.0;
    s_grad[t] = -1.0;
  }
  // (a thread reads only the slots it wrote; s_row / s_diag of OTHER members are first read behind the loop's barrier)

  int iter = 0, capped = 0;
  double gap = 0.0;
  for (;;) {
    Cand up, low;
    up.t = low.t = -1;
    up.key = low.key = up.alpha = low.alpha = 0.0;
    for (int t = tid; t < nm; t += SVM_THREADS) {
      const double a = s_alpha[t], g = s_grad[t];
      const bool pos = t < np;
      Cand c;
      c.key = pos ? -g : g;
      c.alpha = a;
      c.t = t;
      if ((pos ? a < C : a > 0.0) && better_up(c, up)) up = c;
      if ((pos ? a > 0.0 : a < C) && better_low(c, low)) low = c;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const Cand ou = shfl_xor_cand(up, o), ol = shfl_xor_cand(low, o);
      if (better_up(ou, up)) up = ou;
      if (better_low(ol, low)) low = ol;
    }
    const int buf = iter & 1;
    if (lane == 0) {
      s_up[buf][wave] = up;
      s_low[buf][wave] = low;
    }
    __syncthreads();
    up = s_up[buf][0];
    low = s_low[buf][0];
#pragma unroll
    for (int w = 1; w < SVM_WAVES; ++w) {
      const Cand ou = s_up[buf][w], ol = s_low[buf][w];
      if (better_up(ou, up)) up = ou;
      if (better_low(ol, low)) low = ol;
    }
    if (up.t < 0 || low.t < 0) {                  // one of the sets is empty: nothing can move (libsvm: the gap is -inf)
      gap = 0.0;
      break;
    }
    gap = up.key - low.key;
    if (gap < eps) break;
    if (iter >= max_iter) {
      capped = 1;
      break;
    }
    ++iter;
    const int i = up.t, j = low.t;
    const int ri = s_row[i], rj = s_row[j];
    const float* __restrict__ Gi = G + (size_t)ri * ld;
    const float* __restrict__ Gj = G + (size_t)rj * ld;
    double eta = (double)s_diag[i] + (double)s_diag[j] - 2.0 * (double)Gi[rj];
    if (eta <= 0.0) eta = SVM_TAU;
    const bool ipos = i < np, jpos = j < np;
    const double room_i = ipos ? C - up.alpha : up.alpha;          // a_i moves by y_i s, a_j by -y_j s, s > 0
    const double room_j = jpos ? low.alpha : C - low.alpha;
    const double s = fmin(gap / eta, fmin(room_i, room_j));        // (both rooms are positive: i is in up, j in low)
    if (i % SVM_THREADS == tid)
      s_alpha[i] = s == room_i ? (ipos ? C : 0.0) : (ipos ? fmin(up.alpha + s, C) : fmax(up.alpha - s, 0.0));
    if (j % SVM_THREADS == tid)
      s_alpha[j] = s == room_j ? (jpos ? 0.0 : C) : (jpos ? fmax(low.alpha - s, 0.0) : fmin(low.alpha + s, C));
    for (int t = tid; t < nm; t += SVM_THREADS) {
      const int rt = s_row[t];
      const double d = s * ((double)Gi[rt] - (double)Gj[rt]);
      s_grad[t] += t < np ? d : -d;
    }
  }

  // ---- rho (libsvm calculate_rho) and the dual coefficients --------------------------------------------------------------
  double ub = __builtin_huge_val(), lb = -__builtin_huge_val(), sum = 0.0;
  int nfree = 0;
  double* __restrict__ coef_c = coef + (size_t)ci * (K - 1) * n;
  for (int t = tid; t < nm; t += SVM_THREADS) {
    const double a = s_alpha[t];
    const bool pos = t < np;
    const double yg = pos ? s_grad[t] : -s_grad[t];
    if (a >= C) {
      if (pos) lb = fmax(lb, yg);
      else ub = fmin(ub, yg);
    } else if (a <= 0.0) {
      if (pos) ub = fmin(ub, yg);
      else lb = fmax(lb, yg);
    } else {
      ++nfree;
      sum += yg;
    }
    // dual_coef_: a sample of class p against class q sits in row q - 1, one of class q against p < q in row p
    if (pos) coef_c[(size_t)(q - 1) * n + p0 + t] = a;
    else coef_c[(size_t)p * n + q0 + (t - np)] = -a;
  }
  ub = wave_min_f64(ub);
  lb = wave_max_f64(lb);
  sum = wave_sum_f64(sum);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) nfree += __shfl_xor(nfree, o, kWave);
  if (lane == 0) {
    s_red[0][wave] = ub;
    s_red[1][wave] = lb;
    s_red[2][wave] = sum;
    s_free[wave] = nfree;
  }
  __syncthreads();
  if (tid == 0) {
    ub = s_red[0][0], lb = s_red[1][0], sum = s_red[2][0], nfree = s_free[0];
    for (int w = 1; w < SVM_WAVES; ++w) {
      ub = fmin(ub, s_red[0][w]);
      lb = fmax(lb, s_red[1][w]);
      sum += s_red[2][w];
      nfree += s_free[w];
    }
    const size_t o = (size_t)ci * P + pair;
    rho[o] = nfree > 0 ? sum / nfree : (ub + lb) / 2.0;
    status[2 * o] = iter;
    status[2 * o + 1] = capped;
    gap_out[o] = gap;
  }
}

// (Every coef slot is written by exactly one workgroup: a sample of class k meets each of the K - 1 other classes once,
// in the rows 0 .. k - 1 for the classes below it and k .. K - 2 for those above.)

__global__ __launch_bounds__(SVM_THREADS) void svm_ovo_predict_kernel(
    int m, int n, int ld, int K, int P, const float* __restrict__ Gte, const int* __restrict__ order, SvmLayout lay,
    const double* __restrict__ coef, const double* __restrict__ rho, double* __restrict__ dec, int* __restrict__ pred) {
  __shared__ float s_k[SVM_PRED_MAX_N];           // the test row's Gram entries in class order
  __shared__ unsigned char s_first[SVM_MAX_CLASSES * (SVM_MAX_CLASSES - 1) / 2];   // dec > 0 per pair
  __shared__ int s_votes[SVM_MAX_CLASSES];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int r = blockIdx.x, ci = blockIdx.y;
  const float* __restrict__ row = Gte + (size_t)r * ld;
  for (int t = tid; t < n; t += SVM_THREADS) s_k[t] = row[order[t]];
  __syncthreads();
  const double* __restrict__ coef_c = coef + (size_t)ci * (K - 1) * n;
  for (int pair = wave; pair < P; pair += SVM_WAVES) {
    int p, q;
    pair_of(pair, K, p, q);
    const int p0 = lay.class_ptr[p], p1 = lay.class_ptr[p + 1], q0 = lay.class_ptr[q], q1 = lay.class_ptr[q + 1];
    const double* __restrict__ cp = coef_c + (size_t)(q - 1) * n;
    const double* __restrict__ cq = coef_c + (size_t)p * n;
    double acc = 0.0;
    for (int t = p0 + lane; t < p1; t += kWave) acc += cp[t] * (double)s_k[t];
    for (int t = q0 + lane; t < q1; t += kWave) acc += cq[t] * (double)s_k[t];
    acc = wave_sum_f64(acc);
    const double d = acc - rho[(size_t)ci * P + pair];
    if (lane == 0) {
      dec[((size_t)ci * m + r) * P + pair] = d;
      s_first[pair] = d > 0.0 ? 1 : 0;
    }
  }
  __syncthreads();
  if (tid < K) {
    int votes = 0;
    for (int o = 0; o < K; ++o) {
      if (o == tid) continue;
      const int a = o < tid ? o : tid, b = o < tid ? tid : o;
      const int pair = a * (2 * K - a - 1) / 2 + (b - a - 1);
      votes += (s_first[pair] != 0) == (tid == a) ? 1 : 0;
    }
    s_votes[tid] = votes;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    for (int k = 1; k < K; ++k)
      if (s_votes[k] > s_votes[best]) best = k;
    pred[(size_t)ci * m + r] = best;
  }
}

int fill_layout(int n, int K, int nC, const int* class_ptr, const double* Cs, SvmLayout& lay) {
  if (!class_ptr || !Cs) return bad_arg("svm: null class_ptr / Cs");
  if (K < 2 || K > SVM_MAX_CLASSES) return unsupported("svm: 2 <= K <= PDAE_SVM_MAX_CLASSES classes");
  if (nC < 1 || nC > SVM_MAX_C) return bad_arg("svm: 1 <= nC <= PDAE_SVM_MAX_C values of C");
  if (class_ptr[0] != 0 || class_ptr[K] != n) return bad_arg("svm: class_ptr must run from 0 to n");
  for (int k = 0; k < K; ++k)
    if (class_ptr[k + 1] <= class_ptr[k]) return bad_arg("svm: every class needs at least one sample");
  for (int k = 0; k <= K; ++k) lay.class_ptr[k] = class_ptr[k];
  for (int k = K + 1; k <= SVM_MAX_CLASSES; ++k) lay.class_ptr[k] = n;
  for (int c = 0; c < SVM_MAX_C; ++c) lay.C[c] = c < nC ? Cs[c] : 0.0;
  for (int c = 0; c < nC; ++c)
    if (!(Cs[c] > 0.0)) return bad_arg("svm: C must be positive");
  return PDAE_OK;
}

}  // namespace
}  // namespace pdae

using namespace pdae;

extern "C" int pdae_svm_ovo_supported(int n, int K, int nC, const int* class_ptr, const double* Cs, int max_iter) {
  SvmLayout lay;
  const int rc = fill_layout(n, K, nC, class_ptr, Cs, lay);
  if (rc != PDAE_OK) return rc;
  if (max_iter <= 0) return bad_arg("svm_ovo_train: max_iter >= 1 required (the solver loop is bounded by it)");
  int a = 0, b = 0;                                // the two largest classes make the largest pair
  for (int k = 0; k < K; ++k) {
    const int c = class_ptr[k + 1] - class_ptr[k];
    if (c > a) b = a, a = c;
    else if (c > b) b = c;
  }
  if (a + b > SVM_MAX_MEMBERS)
    return unsupported("svm_ovo_train: a class pair has more than PDAE_SVM_MAX_PAIR (2048) members");
  return PDAE_OK;
}

extern "C" int pdae_svm_ovo_train(int n, int ld, int K, int nC, const float* G, const int* order, const int* class_ptr,
                                  const double* Cs, double eps, int max_iter, double* coef, double* rho, int* status,
                                  double* gap, pdae_stream_t stream) {
  if (n < 2 || ld < n) return bad_arg("svm_ovo_train: n >= 2 and ld >= n required");
  if (!G || !order || !coef || !rho || !status || !gap) return bad_arg("svm_ovo_train: null pointer");
  if (!(eps > 0.0)) return bad_arg("svm_ovo_train: eps > 0 required");
  const int ok = pdae_svm_ovo_supported(n, K, nC, class_ptr, Cs, max_iter);
  if (ok != PDAE_OK) return ok;
  SvmLayout lay;
  fill_layout(n, K, nC, class_ptr, Cs, lay);
  const int P = K * (K - 1) / 2;
  hipLaunchKernelGGL(svm_ovo_train_kernel, dim3(P, nC), dim3(SVM_THREADS), 0, as_stream(stream), n, ld, K, P, G, order, lay,
                     eps, max_iter, coef, rho, status, gap);
  return check_launch("svm_ovo_train");
}

extern "C" int pdae_svm_ovo_predict(int m, int n, int ld, int K, int nC, const float* Gte, const int* order,
                                    const int* class_ptr, const double* coef, const double* rho, double* dec, int* pred,
                                    pdae_stream_t stream) {
  if (m < 1 || n < 2 || ld < n) return bad_arg("svm_ovo_predict: m >= 1, n >= 2 and ld >= n required");
  if (!Gte || !order || !coef || !rho || !dec || !pred) return bad_arg("svm_ovo_predict: null pointer");
  if (n > SVM_PRED_MAX_N)
    return unsupported("svm_ovo_predict: more than PDAE_SVM_PREDICT_MAX_TRAIN (12288) training samples");
  SvmLayout lay;
  const double ones[SVM_MAX_C] = {1, 1, 1, 1, 1, 1, 1, 1};
  const int rc = fill_layout(n, K, nC, class_ptr, ones, lay);
  if (rc != PDAE_OK) return rc;
  const int P = K * (K - 1) / 2;
  hipLaunchKernelGGL(svm_ovo_predict_kernel, dim3(m, nC), dim3(SVM_THREADS), 0, as_stream(stream), m, n, ld, K, P, Gte, order,
                     lay, coef, rho, dec, pred);
  return check_launch("svm_ovo_predict");
}
