// loss_ce.hip — fused weighted cross-entropy (label smoothing, ignore_index) and Dice + CE for 2 to 16 classes.
//
// Replaces torch.nn.CrossEntropyLoss on (N, K, H, W) logits (the factory's 'ce' branch, reference loss.py:253-256:
// log_softmax, nll_loss and their two backward kernels, each a pass over the fp32 logits) and adds the pairing of
// the reference's multi-class DiceLoss (loss.py:18-85) with a cross-entropy that weights every class.
//
// With logp = log_softmax(z) over the classes, class weights w[K] (ones when none) and label smoothing eps:
//   nll_i = -w[t_i] logp_i[t_i],   sm_i = -sum_k w[k] logp_i[k],   Wsum = sum_valid w[t_i]
//   CE = ((1-eps) sum nll_i + (eps/K) sum sm_i) / Wsum   ('mean'; 'sum' without the division; 'none' per pixel)
//   Dice = 1 - mean_{n, c >= c_lo} (2 I_nc + s) / (P_nc + T_nc + s),  I, P, T summed over VALID pixels only
//   total = sum_s set_w[s] (ce_w CE_s + dice_w Dice_s)
// A pixel is valid iff 0 <= t < K and t != ignore_index; any other label contributes nothing to any sum and gets a
// zero gradient (no device assert, unlike torch's kernels).
//
// Pass 1 (reduce): a lane owns 4 consecutive pixels: K 16-byte loads (one per class plane) issued before any is
//   used, then max, exp-sum, lse, nll, sm and p_k from registers: every logit is read from memory once.  A block
//   covers one partial row (unet_loss_rows(HW) rows of `per` pixels, per a multiple of 4; past the 1024-row cap a
//   block strides).  Fields per row: F = 4 (sum w_t, sum nll, sum sm, #valid), + 3K (I_c, P_c, T_c) only in the DICE
//   instantiation.  Block reduction: a wave reduction per field, the waves' F values to LDS, ONE barrier, threads
//   f < F add the waves in wave order.  part[set][n][row][F].
// Finalize (one block, fp64): the rows in a fixed order, the scalar, and the grad pass's table
//   coef[set][4 + 2NK]: c_nll = set_w ce_w (1-eps) / Wsum, c_sm = set_w ce_w (eps/K) / Wsum (no division unless
//   'mean'), sum_k w_k, Wsum, then per (n, c) Dice gA[N][K], gB[N][K] scaled by set_w dice_w (DICE only).
// Pass 2 (grad): the same loads and register softmax, 16-byte stores per class plane:
//   dz_k = g ( c_nll w_t (p_k - [k=t]) + c_sm (p_k sum_j w_j - w_k) + G_k p_k - p_k sum_c G_c p_c ),
//   G_c = gA_nc [t=c] + gB_nc for c >= c_lo; invalid pixels get zeros in all K planes.
// HW % 4 != 0 (plane bases not 16-byte aligned), a misaligned pointer and a row's last partial quad take scalar
// loads / stores of the same arithmetic.  All three are HBM-bound (one read of the logits per pass; the only matrix
// product, the soft confusion sums onehot^T p, is under 5 % of the load time): no MFMA.  Sums are fixed-order, there
// are no atomics: results are bit-identical from run to run.  This file is built with -ffp-contract=on so that the
// DICE and plain instantiations round the shared cross-entropy arithmetic identically.
#include <stdio.h>

#include "common.h"

namespace unet {

constexpr int CE_MAXK = 16;
constexpr int CE_MAXS = 4;
constexpr int CE_THREADS = 256;
constexpr int CE_WAVES = CE_THREADS / WAVE;
constexpr int CE_HDR = 4;   // coef header: c_nll, c_sm, sum_k w_k, Wsum

struct CeSets {
  const float* z[CE_MAXS];
  float* dz[CE_MAXS];
  float w[CE_MAXS];
};

// the logits of up to 4 consecutive pixels of every class plane: v[k][j] = zp[k HW + j] (0 where k >= K or j >= cnt)
template <int KP>
__device__ __forceinline__ void ce_load_quad(const float* __restrict__ zp, long long HW, int K, int cnt, bool vec,
                                             float (&v)[KP][4]) {
  if (vec && cnt == 4) {
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < K) q = *reinterpret_cast<const float4*>(zp + k * HW);
      v[k][0] = q.x; v[k][1] = q.y; v[k][2] = q.z; v[k][3] = q.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < KP; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[k][j] = (k < K && j < cnt) ? zp[k * HW + j] : 0.f;
  }
}

// labels of the quad: the class, or -1 for an invalid pixel (out of range, ignore_index, or past the quad's end)
__device__ __forceinline__ void ce_load_targets(const int64_t* __restrict__ tp, int K, int cnt, bool vec,
                                                int ignore_index, int (&tv)[4]) {
  long long tl[4] = {-1, -1, -1, -1};
  if (vec && cnt == 4) {
    const longlong2 a = *reinterpret_cast<const longlong2*>(tp), b = *reinterpret_cast<const longlong2*>(tp + 2);
    tl[0] = a.x; tl[1] = a.y; tl[2] = b.x; tl[3] = b.y;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (j < cnt) tl[j] = tp[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) tv[j] = (tl[j] >= 0 && tl[j] < K && tl[j] != ignore_index) ? (int)tl[j] : -1;
}

// pixel j of a quad: e[k] = exp(z_k - max) (0 for k >= K), their sum, and the max
template <int KP>
__device__ __forceinline__ float ce_exps(const float (&v)[KP][4], int j, int K, float (&e)[KP], float& se) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < KP; ++k) if (k < K) m = fmaxf(m, v[k][j]);
  se = 0.f;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    e[k] = k < K ? expf(v[k][j] - m) : 0.f;
    se += e[k];
  }
  return m;
}

template <int KP>
__device__ __forceinline__ void ce_load_weights(const float* __restrict__ wgt, int K, float (&wk)[KP]) {
#pragma unroll
  for (int k = 0; k < KP; ++k) wk[k] = k < K ? (wgt ? wgt[k] : 1.f) : 0.f;
}

// ------------------------------------------------------------------------------------------------
// pass 1
// ------------------------------------------------------------------------------------------------
template <int KP, int DICE>
__global__ __launch_bounds__(CE_THREADS) void ce_reduce_kernel(long long N, int K, long long HW, const CeSets sets,
                                                               const int64_t* __restrict__ t,
                                                               const float* __restrict__ wgt, int ignore_index,
                                                               float c_nll, float c_sm, float* __restrict__ part,
                                                               float* __restrict__ map, int rows, long long per,
                                                               int vec) {
  constexpr int FM = 4 + (DICE ? 3 * KP : 0);
  __shared__ float sh[CE_WAVES][FM];
  const int F = 4 + (DICE ? 3 * K : 0);
  const long long n = blockIdx.y;
  const float* z = sets.z[blockIdx.z] + n * K * HW;
  const int64_t* tt = t + n * HW;
  float wk[KP];
  ce_load_weights<KP>(wgt, K, wk);
  float acc[FM];
#pragma unroll
  for (int f = 0; f < FM; ++f) acc[f] = 0.f;
  const long long q0 = blockIdx.x * per, q1 = min(HW, q0 + per);
  for (long long q = q0 + 4 * threadIdx.x; q < q1; q += 4 * CE_THREADS) {
    const int cnt = (int)min(4LL, q1 - q);
    float v[KP][4];
    int tv[4];
    ce_load_quad<KP>(z + q, HW, K, cnt, vec, v);
    ce_load_targets(tt + q, K, cnt, vec, ignore_index, tv);
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float e[KP], se;
      const float m = ce_exps<KP>(v, j, K, e, se);
      const float lse = m + logf(se);
      const bool ok = tv[j] >= 0;
      float wt = 0.f, nll = 0.f, sm = 0.f;
#pragma unroll
      for (int k = 0; k < KP; ++k) {   // a padded class k >= K has w_k = 0, z_k = 0, e_k = 0 and matches no label
        const float nl = wk[k] * (lse - v[k][j]);   // -w_k logp_k >= 0
        sm += nl;
        if (tv[j] == k) { wt = wk[k]; nll = nl; }
      }
      acc[0] += wt;
      acc[1] += nll;
      acc[2] += ok ? sm : 0.f;
      acc[3] += ok ? 1.f : 0.f;
      out[j] = ok ? c_nll * nll + c_sm * sm : 0.f;
      if (DICE) {
        const float inv = 1.f / se;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          const float pk = e[k] * inv;
          acc[4 + 3 * k] += tv[j] == k ? pk : 0.f;
          acc[4 + 3 * k + 1] += ok ? pk : 0.f;
          acc[4 + 3 * k + 2] += tv[j] == k ? 1.f : 0.f;
        }
      }
    }
    if (map) {   // reduction 'none' (one set): the per-pixel loss
      float* mp = map + n * HW + q;
      if (vec && cnt == 4) {
        *reinterpret_cast<float4*>(mp) = make_float4(out[0], out[1], out[2], out[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < cnt) mp[j] = out[j];
      }
    }
  }
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int f = 0; f < FM; ++f) {   // the fields of padded classes are zeros
    const float s = wave_sum(acc[f]);
    if (lane == 0) sh[wave][f] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < F) {
    float s = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < CE_WAVES; ++w) s += sh[w][threadIdx.x];
    part[(((size_t)blockIdx.z * N + n) * rows + blockIdx.x) * F + threadIdx.x] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// finalize: one block, fp64.  Per set: (1) one wave per (image, field) pair sums the rows (fixed order per lane,
// then a fixed shuffle tree); (2) one thread per image forms its Dice terms; (3) thread 0 combines in image order.
// ------------------------------------------------------------------------------------------------
__global__ void ce_finalize_kernel(const float* __restrict__ part, int rows, int S, const CeSets sets, long long N,
                                   int K, const float* __restrict__ wgt, float ce_w, float dice_w, double eps,
                                   float dice_smooth, int ignore_bg, int dice, int reduction,
                                   float* __restrict__ loss, float* __restrict__ coef) {
  extern __shared__ double dsh[];   // [N*F] field sums, [N*K] Dice coefficients D_nc
  const int F = 4 + (dice ? 3 * K : 0);
  const size_t cstride = CE_HDR + (dice ? 2 * (size_t)N * K : 0);
  const int c_lo = ignore_bg ? 1 : 0;
  const int nd = K - c_lo;
  double* fs = dsh;
  double* dD = dsh + N * F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  double total = 0;
  for (int si = 0; si < S; ++si) {
    const float* ps = part + (size_t)si * N * rows * F;
    float* cf = coef + si * cstride;
    const double ws = sets.w[si];
    for (long long pf = wave; pf < N * F; pf += nw) {
      const long long n = pf / F;
      const int f = (int)(pf % F);
      double a = 0;
      for (int r = lane; r < rows; r += 64) a += ps[((size_t)n * rows + r) * F + f];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      if (lane == 0) fs[pf] = a;
    }
    __syncthreads();
    if (dice) {
      const double wred = ws * dice_w / ((double)N * nd);
      for (long long n = threadIdx.x; n < N; n += blockDim.x) {
        const double* s = fs + n * F + 4;
        float* g = cf + CE_HDR + n * 2 * K;
        for (int c = 0; c < K; ++c) {
          const double I = s[3 * c], U = s[3 * c + 1] + s[3 * c + 2] + dice_smooth;
          dD[n * K + c] = (2.0 * I + dice_smooth) / U;
          g[c] = c >= c_lo ? (float)(-2.0 * wred / U) : 0.f;
          g[K + c] = c >= c_lo ? (float)(wred * (2.0 * I + dice_smooth) / (U * U)) : 0.f;
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      double wsum = 0, nll = 0, sm = 0, sw = 0;
      for (long long n = 0; n < N; ++n) {
        wsum += fs[n * F];
        nll += fs[n * F + 1];
        sm += fs[n * F + 2];
      }
      for (int k = 0; k < K; ++k) sw += wgt ? (double)wgt[k] : 1.0;
      const double den = reduction == 0 ? wsum : 1.0;   // 'mean' with every pixel ignored: 0 / 0 = NaN, as torch
      const double ce = ((1.0 - eps) * nll + (eps / K) * sm) / den;
      cf[0] = (float)(ws * ce_w * (1.0 - eps) / den);
      cf[1] = (float)(ws * ce_w * (eps / K) / den);
      cf[2] = (float)sw;
      cf[3] = (float)wsum;
      double term = ce_w * ce;
      if (dice) {
        double dsum = 0;
        for (long long n = 0; n < N; ++n)
          for (int c = c_lo; c < K; ++c) dsum += dD[n * K + c];
        term += dice_w * (1.0 - dsum / ((double)N * nd));
      }
      total += ws * term;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && reduction != 2) loss[0] = (float)total;
}

// ------------------------------------------------------------------------------------------------
// pass 2
// ------------------------------------------------------------------------------------------------
template <int KP, int DICE>
__global__ __launch_bounds__(CE_THREADS) void ce_grad_kernel(int S, long long N, int K, long long HW,
                                                             const CeSets sets, const int64_t* __restrict__ t,
                                                             const float* __restrict__ wgt, int ignore_index,
                                                             const float* __restrict__ coef,
                                                             const float* __restrict__ gout, int gout_map, int c_lo,
                                                             int vec) {
  const long long Q = (HW + 3) / 4, total = N * Q;
  const size_t cstride = CE_HDR + (DICE ? 2 * (size_t)N * K : 0);
  float wk[KP];
  ce_load_weights<KP>(wgt, K, wk);
  for (long long i = blockIdx.x * (long long)CE_THREADS + threadIdx.x; i < total * S;
       i += (long long)gridDim.x * CE_THREADS) {
    const int si = (int)(i / total);
    const long long r = i - si * total;
    const long long n = r / Q, q = (r - n * Q) * 4;
    const int cnt = (int)min(4LL, HW - q);
    const float* cf = coef + si * cstride;
    const float c_nll = cf[0], c_sm = cf[1], sw = cf[2];
    float v[KP][4];
    int tv[4];
    ce_load_quad<KP>(sets.z[si] + n * K * HW + q, HW, K, cnt, vec, v);
    ce_load_targets(t + n * HW + q, K, cnt, vec, ignore_index, tv);
    float gA[DICE ? KP : 1], gB[DICE ? KP : 1];
    if (DICE) {
      const float* g = cf + CE_HDR + n * 2 * K;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        gA[k] = k < K ? g[k] : 0.f;
        gB[k] = k < K ? g[K + k] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float e[KP], se;
      ce_exps<KP>(v, j, K, e, se);
      const float inv = 1.f / se;
      const bool ok = tv[j] >= 0;
      const float go = gout_map ? (j < cnt ? gout[n * HW + q + j] : 0.f) : gout[0];
      float wt = 0.f, sgp = 0.f;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        e[k] *= inv;   // p_k
        if (tv[j] == k) wt = wk[k];
        if (DICE && k >= c_lo) sgp += ((tv[j] == k ? gA[k] : 0.f) + gB[k]) * e[k];
      }
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        float d = c_nll * (wt * (e[k] - (tv[j] == k ? 1.f : 0.f))) + c_sm * (e[k] * sw - wk[k]);
        if (DICE) d += (k >= c_lo ? ((tv[j] == k ? gA[k] : 0.f) + gB[k]) * e[k] : 0.f) - e[k] * sgp;
        v[k][j] = ok ? go * d : 0.f;
      }
    }
    float* dz = sets.dz[si] + n * K * HW + q;
    if (vec && cnt == 4) {
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k < K) *reinterpret_cast<float4*>(dz + k * HW) = make_float4(v[k][0], v[k][1], v[k][2], v[k][3]);
    } else {
#pragma unroll
      for (int k = 0; k < KP; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) if (k < K && j < cnt) dz[k * HW + j] = v[k][j];
    }
  }
}

static int ce_load_sets(const char* who, int S, int K, const float* const* z, float* const* dz, const float* w,
                        CeSets& cs) {
  static thread_local char msg[96];
  if (K < 2 || K > CE_MAXK || S > CE_MAXS) {
    snprintf(msg, sizeof(msg), "%s: n_classes must be in [2, 16] and at most 4 logit sets", who);
    set_error(msg);
    return UNET_ERR_UNSUPPORTED;
  }
  if (S < 1) {
    snprintf(msg, sizeof(msg), "%s: at least one logit set", who);
    set_error(msg);
    return UNET_ERR_ARG;
  }
  for (int i = 0; i < CE_MAXS; ++i) {
    cs.z[i] = (i < S && z) ? z[i] : nullptr;
    cs.dz[i] = (i < S && dz) ? dz[i] : nullptr;
    cs.w[i] = i < S ? (w ? w[i] : 1.f) : 0.f;
  }
  return 0;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the instantiation of KERNEL for K classes (padded to 4, 8 or 16) with or without the Dice sums
#define CE_DISPATCH(KERNEL, K, dice, grid, stream, ...)                                                          \
  do {                                                                                                           \
    if ((K) <= 4) {                                                                                              \
      if (dice) hipLaunchKernelGGL((KERNEL<4, 1>), grid, dim3(CE_THREADS), 0, stream, __VA_ARGS__);              \
      else hipLaunchKernelGGL((KERNEL<4, 0>), grid, dim3(CE_THREADS), 0, stream, __VA_ARGS__);                   \
    } else if ((K) <= 8) {                                                                                       \
      if (dice) hipLaunchKernelGGL((KERNEL<8, 1>), grid, dim3(CE_THREADS), 0, stream, __VA_ARGS__);              \
      else hipLaunchKernelGGL((KERNEL<8, 0>), grid, dim3(CE_THREADS), 0, stream, __VA_ARGS__);                   \
    } else {                                                                                                     \
      if (dice) hipLaunchKernelGGL((KERNEL<16, 1>), grid, dim3(CE_THREADS), 0, stream, __VA_ARGS__);             \
      else hipLaunchKernelGGL((KERNEL<16, 0>), grid, dim3(CE_THREADS), 0, stream, __VA_ARGS__);                  \
    }                                                                                                            \
  } while (0)

}  // namespace unet

using namespace unet;

extern "C" {

int unet_ce_reduce_multi(int S, long long N, int K, long long HW, const float* const* z, const int64_t* t,
                         const float* weight, int ignore_index, double label_smoothing, int dice, float* partial,
                         float* map, void* stream) {
  CeSets cs;
  if (int rc = ce_load_sets("unet_ce_reduce", S, K, z, nullptr, nullptr, cs)) return rc;
  if (!z || !t || !partial || N < 1 || N > 65535 || HW < 1 || (map && S != 1)) {
    set_error("unet_ce_reduce: needs logits, targets and partial, 1 <= N <= 65535, and one set for the 'none' map");
    return UNET_ERR_ARG;
  }
  const int rows = unet_loss_rows(HW);
  const long long per = ((HW + rows - 1) / rows + 3) & ~3LL;   // whole quads: a row starts 16-byte aligned
  int vec = (HW % 4 == 0) && aligned16(t) && aligned16(map);
  for (int i = 0; i < S; ++i) vec = vec && aligned16(z[i]);
  const float c_nll = (float)(1.0 - label_smoothing), c_sm = (float)(label_smoothing / K);
  CE_DISPATCH(ce_reduce_kernel, K, dice, dim3(rows, (unsigned)N, S), (hipStream_t)stream, N, K, HW, cs, t, weight,
              ignore_index, c_nll, c_sm, partial, map, rows, per, vec);
  return check_launch("ce_reduce");
}

int unet_ce_reduce(long long N, int K, long long HW, const float* z, const int64_t* t, const float* weight,
                   int ignore_index, double label_smoothing, int dice, float* partial, float* map, void* stream) {
  return unet_ce_reduce_multi(1, N, K, HW, &z, t, weight, ignore_index, label_smoothing, dice, partial, map, stream);
}

int unet_ce_finalize_multi(const float* partial, int rows, int S, const float* set_weights, long long N, int K,
                           const float* weight, float ce_w, float dice_w, double label_smoothing, float dice_smooth,
                           int ignore_bg, int dice, int reduction, float* loss, float* coef, void* stream) {
  CeSets cs;
  if (int rc = ce_load_sets("unet_ce_finalize", S, K, nullptr, nullptr, set_weights, cs)) return rc;
  if (!partial || !coef || N < 1 || rows < 1 || reduction < 0 || reduction > 2 || (reduction != 2 && !loss) ||
      (reduction == 2 && (S != 1 || dice))) {
    set_error("unet_ce_finalize: needs partial and coef (and loss unless 'none'); 'none' takes one set and no Dice term");
    return UNET_ERR_ARG;
  }
  const size_t shm = (size_t)N * (4 + (dice ? 3 * K : 0) + K) * sizeof(double);
  if (shm > 60000) { set_error("unet_ce_finalize: batch too large"); return UNET_ERR_UNSUPPORTED; }
  hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(1024), shm, (hipStream_t)stream, partial, rows, S, cs, N, K,
                     weight, ce_w, dice_w, label_smoothing, dice_smooth, ignore_bg, dice, reduction, loss, coef);
  return check_launch("ce_finalize");
}

int unet_ce_finalize(const float* partial, int rows, long long N, int K, const float* weight, float ce_w,
                     float dice_w, double label_smoothing, float dice_smooth, int ignore_bg, int dice, int reduction,
                     float* loss, float* coef, void* stream) {
  return unet_ce_finalize_multi(partial, rows, 1, nullptr, N, K, weight, ce_w, dice_w, label_smoothing, dice_smooth,
                                ignore_bg, dice, reduction, loss, coef, stream);
}

int unet_ce_grad_multi(int S, long long N, int K, long long HW, const float* const* z, const int64_t* t,
                       const float* weight, int ignore_index, const float* coef, const float* gout,
                       int gout_per_pixel, int dice, int ignore_bg, float* const* dz, void* stream) {
  CeSets cs;
  if (int rc = ce_load_sets("unet_ce_grad", S, K, z, dz, nullptr, cs)) return rc;
  if (!z || !dz || !t || !coef || !gout || N < 1 || HW < 1 || (gout_per_pixel && S != 1)) {
    set_error("unet_ce_grad: needs logits, targets, coef, gout and outputs; a per-pixel gout takes one set");
    return UNET_ERR_ARG;
  }
  int vec = (HW % 4 == 0) && aligned16(t);
  for (int i = 0; i < S; ++i) vec = vec && aligned16(z[i]) && aligned16(dz[i]);
  long long b = (S * N * ((HW + 3) / 4) + CE_THREADS - 1) / CE_THREADS;
  if (b > 8192) b = 8192;
  CE_DISPATCH(ce_grad_kernel, K, dice, dim3((unsigned)b), (hipStream_t)stream, S, N, K, HW, cs, t, weight,
              ignore_index, coef, gout, gout_per_pixel, ignore_bg ? 1 : 0, vec);
  return check_launch("ce_grad");
}

int unet_ce_grad(long long N, int K, long long HW, const float* z, const int64_t* t, const float* weight,
                 int ignore_index, const float* coef, const float* gout, int gout_per_pixel, int dice, int ignore_bg,
                 float* dz, void* stream) {
  return unet_ce_grad_multi(1, N, K, HW, &z, t, weight, ignore_index, coef, gout, gout_per_pixel, dice, ignore_bg,
                            &dz, stream);
}

}  // extern "C"
