// outconv.hip — OutConv for up to 8 classes: forward, backward, and the backward fused with the BatchNorm backward of
// its input activation.  The class axis lives in per-class registers and shuffles here, which is what stops at 8;
// outconv_mc.hip serves 9..16 classes with the class axis on an MFMA row tile (stages.py picks by n_classes).
#include "common.h"

namespace unet {

// ---- OutConv: logits[n,k,h,w] = b[k] + Σ_c w[k][c] · act(y)[n,h,w,c]   (layers.py:120) ----------------
constexpr int OC_MAXK = 8;

template <typename T>
__global__ void outconv_fwd_kernel(long long P, int HW, int C, int K, const T* y, const float* sc, const float* sf,
                                   int relu, const float* w, const float* b, float* out) {
  extern __shared__ float ws[];  // [K][C] then scale/shift
  for (int i = threadIdx.x; i < K * C; i += blockDim.x) ws[i] = w[i];
  float* s_sc = ws + K * C;
  float* s_sf = s_sc + C;
  for (int i = threadIdx.x; i < C; i += blockDim.x) {
    s_sc[i] = sc ? sc[i] : 1.f;
    s_sf[i] = sf ? sf[i] : 0.f;
  }
  __syncthreads();
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < P; q += (long long)gridDim.x * blockDim.x) {
    float acc[OC_MAXK];
#pragma unroll
    for (int k = 0; k < OC_MAXK; ++k) acc[k] = (k < K) ? b[k] : 0.f;
    const T* yp = y + q * C;
    for (int c = 0; c < C; ++c) {
      float a = __builtin_fmaf(to_f(yp[c]), s_sc[c], s_sf[c]);
      if (relu) a = fmaxf(a, 0.f);
#pragma unroll
      for (int k = 0; k < OC_MAXK; ++k)
        if (k < K) acc[k] += ws[k * C + c] * a;
    }
    const long long n = q / HW, hw = q % HW;
#pragma unroll
    for (int k = 0; k < OC_MAXK; ++k)
      if (k < K) out[(n * K + k) * HW + hw] = acc[k];
  }
}

// coalesced variant: G = C/8 lanes per pixel, 8 channels per lane, class sums by xor-shuffles
template <typename T, int KT>
__global__ void outconv_fwd_vec_kernel(long long P, int HW, int C, int G, const T* y, const float* sc, const float* sf,
                                       int relu, const float* w, const float* b, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int sub = lane % G, ppw = 64 / G;
  const int c0 = sub * 8;
  float s[8], f[8], wk[KT][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    s[j] = sc ? sc[c0 + j] : 1.f;
    f[j] = sf ? sf[c0 + j] : 0.f;
#pragma unroll
    for (int k = 0; k < KT; ++k) wk[k][j] = w[k * C + c0 + j];
  }
  const long long stride = (long long)gridDim.x * nw * ppw;
  // OC_U pixels per trip, all their loads issued first (round 6: one memory round trip per trip instead of per
  // pixel; 2.5 TB/s before); each pixel's sum is unchanged
  constexpr int OC_U = 4;
  for (long long q = ((long long)blockIdx.x * nw + wave) * ppw + lane / G; q < P; q += OC_U * stride) {
    float a[OC_U][8];
#pragma unroll
    for (int u = 0; u < OC_U; ++u) {
      const long long qq = q + u * stride < P ? q + u * stride : q;
      if constexpr (sizeof(T) == 2) {
        load_vec<T>(y + qq * C + c0, a[u]);
      } else {
        load_vec<float>((const float*)y + qq * C + c0, a[u]);
        load_vec<float>((const float*)y + qq * C + c0 + 4, a[u] + 4);
      }
    }
#pragma unroll
    for (int u = 0; u < OC_U; ++u) {
      const long long qu = q + u * stride;
      float acc[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) acc[k] = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = __builtin_fmaf(a[u][j], s[j], f[j]);
        if (relu) v = fmaxf(v, 0.f);
#pragma unroll
        for (int k = 0; k < KT; ++k) acc[k] += wk[k][j] * v;
      }
#pragma unroll
      for (int k = 0; k < KT; ++k)
        for (int o = G >> 1; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
      if (sub == 0 && qu < P) {
        const long long n = qu / HW, hw = qu % HW;
#pragma unroll
        for (int k = 0; k < KT; ++k) out[(n * KT + k) * HW + hw] = acc[k] + b[k];
      }
    }
  }
}

// channel lanes x pixel rows: da[p][c] (+)= Σ_k w[k][c] dl[k][p]; partial dW[k][c], db[k]
template <typename T>
__global__ void outconv_bwd_kernel(long long P, int HW, int C, int CL, int K, const T* y, const float* sc,
                                   const float* sf, int relu, const float* w, const float* dl, float* da, int accum,
                                   float* part, int rows) {
  __shared__ float sh[256];
  const int tid = threadIdx.x;
  const int cx = tid % CL, py = tid / CL, R = blockDim.x / CL;
  const int c = blockIdx.x * CL + cx;
  const long long per = (P + rows - 1) / rows;
  const long long p0 = blockIdx.y * per, p1 = min(P, p0 + per);
  float dw[OC_MAXK], db[OC_MAXK], wk[OC_MAXK];
#pragma unroll
  for (int k = 0; k < OC_MAXK; ++k) { dw[k] = 0.f; db[k] = 0.f; wk[k] = (k < K && c < C) ? w[k * C + c] : 0.f; }
  const float s = (c < C && sc) ? sc[c] : 1.f, f = (c < C && sf) ? sf[c] : 0.f;
  for (long long q = p0 + py; q < p1; q += R) {
    const long long n = q / HW, hw = q % HW;
    float g = 0.f;
    float dlk[OC_MAXK];
#pragma unroll
    for (int k = 0; k < OC_MAXK; ++k) {
      dlk[k] = (k < K) ? dl[(n * K + k) * HW + hw] : 0.f;
      g += wk[k] * dlk[k];
      db[k] += dlk[k];
    }
    if (c < C) {
      float a = __builtin_fmaf(to_f(y[q * C + c]), s, f);
      if (relu) a = fmaxf(a, 0.f);
#pragma unroll
      for (int k = 0; k < OC_MAXK; ++k) dw[k] += dlk[k] * a;
      float* o = da + q * C + c;
      *o = accum ? *o + g : g;
    }
  }
  // reduce over the R pixel rows sharing a channel lane
  const int F = K + 1;
  for (int k = 0; k < F; ++k) {
    float v = 0.f;
#pragma unroll
    for (int kk = 0; kk < OC_MAXK; ++kk) if (kk == k) v = dw[kk];
    if (k == K) v = 0.f;
    sh[tid] = v;
    __syncthreads();
    if (py == 0 && c < C && k < K) {
      float a = 0.f;
      for (int r = 0; r < R; ++r) a += sh[r * CL + cx];
      part[((size_t)blockIdx.y * (K + 1) + k) * C + c] = a;
    }
    __syncthreads();
  }
  // db: only channel-block 0 writes it (every lane saw all pixels of its rows)
  if (blockIdx.x == 0) {
    for (int k = 0; k < K; ++k) {
      float v = 0.f;
#pragma unroll
      for (int kk = 0; kk < OC_MAXK; ++kk) if (kk == k) v = db[kk];
      sh[tid] = (cx == 0) ? v : 0.f;
      __syncthreads();
      if (tid == 0) {
        float a = 0.f;
        for (int r = 0; r < R; ++r) a += sh[r * CL];
        part[((size_t)blockIdx.y * (K + 1) + K) * C + k] = a;  // db stored in row K, column k
      }
      __syncthreads();
    }
  }
}

// vectorised form (bf16, C % 8 == 0, G = C/8 a power of two <= 256): a thread owns 8 channels of one
// pixel per iteration — one 16-byte y load, two 16-byte da stores (or read-modify-writes); the K class
// gradients of the pixel are loaded once per thread.  Same partial-sum table as outconv_bwd_kernel:
// part[block][k][c] = Σ dl·a, part[block][K][k] = Σ dl (db).
template <typename T, int KK>
__global__ __launch_bounds__(256) void outconv_bwd_vec_kernel(long long P, int HW, int C, int G, const T* y,
                                                              const float* sc, const float* sf, int relu,
                                                              const float* w, const float* dl, float* da, int accum,
                                                              float* part) {
  constexpr int F = KK * 8 + KK;  // per-thread partials: dw[k][8], db[k]
  __shared__ float sh[256 * F];
  const int tid = threadIdx.x, v = tid % G, py = tid / G, R = 256 / G;
  const int c0 = v * 8;
  float s8[8], f8[8], wk[KK][8], dw[KK][8], db[KK];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    s8[j] = sc ? sc[c0 + j] : 1.f;
    f8[j] = sf ? sf[c0 + j] : 0.f;
#pragma unroll
    for (int k = 0; k < KK; ++k) { wk[k][j] = w[k * C + c0 + j]; dw[k][j] = 0.f; }
  }
#pragma unroll
  for (int k = 0; k < KK; ++k) db[k] = 0.f;
  const float lo = relu ? 0.f : -INFINITY;
  const long long per = (P + gridDim.x - 1) / gridDim.x;
  const long long p0 = blockIdx.x * per, p1 = min(P, p0 + per);
  for (long long q = p0 + py; q < p1; q += R) {
    const long long n = q / HW, hw = q % HW;
    float dlk[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) { dlk[k] = dl[(n * KK + k) * HW + hw]; db[k] += dlk[k]; }
    float a[8];
    load_vec<T>(y + q * C + c0, a);
    float g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = fmaxf(__builtin_fmaf(a[j], s8[j], f8[j]), lo);
      g[j] = 0.f;
#pragma unroll
      for (int k = 0; k < KK; ++k) { g[j] += wk[k][j] * dlk[k]; dw[k][j] += dlk[k] * a[j]; }
    }
    float4* o = reinterpret_cast<float4*>(da + q * C + c0);
    float4 g0 = make_float4(g[0], g[1], g[2], g[3]), g1 = make_float4(g[4], g[5], g[6], g[7]);
    if (accum) {
      const float4 a0 = o[0], a1 = o[1];
      g0.x += a0.x; g0.y += a0.y; g0.z += a0.z; g0.w += a0.w;
      g1.x += a1.x; g1.y += a1.y; g1.z += a1.z; g1.w += a1.w;
    }
    o[0] = g0;
    o[1] = g1;
  }
#pragma unroll
  for (int k = 0; k < KK; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[tid * F + k * 8 + j] = dw[k][j];
    sh[tid * F + KK * 8 + k] = db[k];
  }
  __syncthreads();
  // fixed-order sums over the R pixel rows: thread e < C*KK owns dw[k][c]; e < KK (extra) owns db[k]
  for (int e = tid; e < C * KK + KK; e += 256) {
    float acc = 0.f;
    if (e < C * KK) {
      const int k = e / C, c = e % C, vv = c / 8, j = c % 8;
      for (int r = 0; r < R; ++r) acc += sh[(r * G + vv) * F + k * 8 + j];
      part[((size_t)blockIdx.x * (KK + 1) + k) * C + c] = acc;
    } else {
      const int k = e - C * KK;
      for (int r = 0; r < R; ++r) acc += sh[(r * G) * F + KK * 8 + k];  // channel-vector 0 of each row
      part[((size_t)blockIdx.x * (KK + 1) + KK) * C + k] = acc;
    }
  }
}

// OutConv backward fused with the BatchNorm backward of its input activation (the last DoubleConv's output,
// whose only consumer is OutConv: unet.py:92 / :203).  The activation gradient g[px][c] = Σ_k W[k][c]·dl[k][px]
// is never stored: this pass accumulates OutConv's dW / db partials (as outconv_bwd_vec_kernel) and the
// BatchNorm-backward sums Σ g_m, Σ g_m·x̂ (g_m: g where the ReLU passed, as bn_bwd_reduce_vec_kernel) from
// one read of y and the 2-class logit gradient; bn_bwd_apply_oc_kernel recomputes g the same way.  Removes the
// fp32 [N,H,W,C] gradient write and its two reads (3 x 268 MB at 4 x 512^2 x 64).
template <typename T, int KK>
__global__ __launch_bounds__(256) void outconv_bwd_bn_kernel(long long P, int HW, int C, int G, const T* y,
                                                             const float* sc, const float* sf, int relu,
                                                             const float* w, const float* dl, const float* mean,
                                                             const float* invstd, float* part, float* bpart, int rows) {
  constexpr int F = KK * 8 + KK;  // per-thread partials: dw[k][8], db[k]
  __shared__ float sh[256 * F];
  const int tid = threadIdx.x, v = tid % G, py = tid / G, R = 256 / G;
  const int c0 = v * 8;
  float s8[8], f8[8], mu[8], is[8], wk[KK][8], dw[KK][8], db[KK], sg[8], sgx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    s8[j] = sc[c0 + j];
    f8[j] = sf[c0 + j];
    mu[j] = mean[c0 + j];
    is[j] = invstd[c0 + j];
    sg[j] = 0.f;
    sgx[j] = 0.f;
#pragma unroll
    for (int k = 0; k < KK; ++k) { wk[k][j] = w[k * C + c0 + j]; dw[k][j] = 0.f; }
  }
#pragma unroll
  for (int k = 0; k < KK; ++k) db[k] = 0.f;
  const float lo = relu ? 0.f : -INFINITY;
  const long long per = (P + gridDim.x - 1) / gridDim.x;
  const long long p0 = blockIdx.x * per, p1 = min(P, p0 + per);
  // OB_U pixels per trip, loads first (round 6); the sums still run over q, q + R, ... in order (bit-identical)
  constexpr int OB_U = 4;
  for (long long q = p0 + py; q < p1; q += OB_U * R) {
    float dlu[OB_U][KK], yu[OB_U][8];
#pragma unroll
    for (int u = 0; u < OB_U; ++u) {
      const long long qq = q + u * R < p1 ? q + u * R : q;
      const long long n = qq / HW, hw = qq % HW;
#pragma unroll
      for (int k = 0; k < KK; ++k) dlu[u][k] = dl[(n * KK + k) * HW + hw];
      load_vec<T>(y + qq * C + c0, yu[u]);
      if constexpr (sizeof(T) == 4) load_vec<T>(y + qq * C + c0 + 4, yu[u] + 4);
    }
#pragma unroll
    for (int u = 0; u < OB_U; ++u) {
      if (q + u * R >= p1) break;
      const float* dlk = dlu[u];
      const float* yv = yu[u];
#pragma unroll
      for (int k = 0; k < KK; ++k) db[k] += dlk[k];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pre = __builtin_fmaf(yv[j], s8[j], f8[j]);
        const float a = fmaxf(pre, lo);
        float g = 0.f;
#pragma unroll
        for (int k = 0; k < KK; ++k) { g += wk[k][j] * dlk[k]; dw[k][j] += dlk[k] * a; }
        const float gm = (relu && !(pre > 0.f)) ? 0.f : g;
        sg[j] += gm;
        sgx[j] += gm * (yv[j] - mu[j]) * is[j];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < KK; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[tid * F + k * 8 + j] = dw[k][j];
    sh[tid * F + KK * 8 + k] = db[k];
  }
  __syncthreads();
  for (int e = tid; e < C * KK + KK; e += 256) {
    float acc = 0.f;
    if (e < C * KK) {
      const int k = e / C, c = e % C, vv = c / 8, j = c % 8;
      for (int r = 0; r < R; ++r) acc += sh[(r * G + vv) * F + k * 8 + j];
      part[((size_t)blockIdx.x * (KK + 1) + k) * C + c] = acc;
    } else {
      const int k = e - C * KK;
      for (int r = 0; r < R; ++r) acc += sh[(r * G) * F + KK * 8 + k];
      part[((size_t)blockIdx.x * (KK + 1) + KK) * C + k] = acc;
    }
  }
  __syncthreads();
  // BatchNorm-backward partial sums of the block: [2][rows][C] (unet_bn_bwd_finalize's layout)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sh[tid] = sg[j];
    sh[256 + tid] = sgx[j];
    __syncthreads();
    if (tid < G) {
      float a = 0.f, b = 0.f;
      for (int r = 0; r < R; ++r) { a += sh[r * G + tid]; b += sh[256 + r * G + tid]; }
      bpart[(size_t)blockIdx.x * C + tid * 8 + j] = a;
      bpart[((size_t)rows + blockIdx.x) * C + tid * 8 + j] = b;
    }
    __syncthreads();
  }
}

// dy = A·g_m + B·y + C with g recomputed from the logit gradient (bn_bwd_apply_vec_kernel's formula)
template <typename T, int KK>
__global__ __launch_bounds__(256) void bn_bwd_apply_oc_kernel(long long P, int HW, int C, const T* y, const float* scale,
                                                              const float* shift, int relu, const float* w,
                                                              const float* dl, const float* coef, T* dy) {
  const int CV = C / 8;
  const long long total = P * CV;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const int cv = (int)(e % CV);  // fixed: the stride is a multiple of CV (power of two <= 256)
  float sc[8], sf[8], A[8], B[8], Cc[8], wk[KK][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cv * 8 + j;
    sc[j] = scale[c]; sf[j] = shift[c]; A[j] = coef[c]; B[j] = coef[C + c]; Cc[j] = coef[2 * C + c];
#pragma unroll
    for (int k = 0; k < KK; ++k) wk[k][j] = w[k * C + c];
  }
  const int cvs = __builtin_ctz(CV);
  // AO_U elements per trip, every load before the stores (dy may alias the loads as far as the compiler knows,
  // which serialised one memory round trip per pixel; round 6); elementwise.  The unroll moved the compiler's
  // fma contraction of o = A g + B y + C (last bits of dy); the order is now explicit, as in bn.hip
  constexpr int AO_U = 4;
  for (; e < total; e += AO_U * stride) {
    float dlu[AO_U][KK], yu[AO_U][8];
    long long pu[AO_U];
#pragma unroll
    for (int u = 0; u < AO_U; ++u) {
      const long long p = (e + u * stride < total ? e + u * stride : e) >> cvs;
      pu[u] = p;
      const unsigned n = (unsigned)p / (unsigned)HW, hw = (unsigned)p - n * (unsigned)HW;
#pragma unroll
      for (int k = 0; k < KK; ++k) dlu[u][k] = dl[((size_t)n * KK + k) * HW + hw];
      load_vec<T>(y + p * C + cv * 8, yu[u]);
      if constexpr (sizeof(T) == 4) load_vec<T>(y + p * C + cv * 8 + 4, yu[u] + 4);
    }
#pragma unroll
    for (int u = 0; u < AO_U; ++u) {
      if (e + u * stride >= total) break;
      const long long p = pu[u];
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float g = 0.f;
#pragma unroll
        for (int k = 0; k < KK; ++k) g += wk[k][j] * dlu[u][k];
        const float gj = (relu && !(__builtin_fmaf(yu[u][j], sc[j], sf[j]) > 0.f)) ? 0.f : g;
        o[j] = f32_rounded(__builtin_fmaf(A[j], gj, __builtin_fmaf(B[j], yu[u][j], Cc[j])));   // bn.hip's rounding
      }
      store_vec<T>(dy + p * C + cv * 8, o);
      if constexpr (sizeof(T) == 4) store_vec<T>(dy + p * C + cv * 8 + 4, o + 4);
    }
  }
}

// one block per output element; fixed-order fp64 block reduction over the partial rows
__global__ void outconv_bwd_finalize_kernel(const float* part, int rows, int C, int K, float* dw, float* db, int accum) {
  __shared__ double sh[4];
  const int e = blockIdx.x;
  const bool is_w = e < K * C;
  const int k = is_w ? e / C : K;
  const int c = is_w ? e % C : e - K * C;
  double s = 0;
  for (int r = threadIdx.x; r < rows; r += blockDim.x) s += part[((size_t)r * (K + 1) + k) * C + c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = (float)(sh[0] + sh[1] + sh[2] + sh[3]);
    float* o = is_w ? dw + e : db + c;
    *o = accum ? *o + v : v;
  }
}

static inline int oc_rows(long long P) {
  long long r = (P + 1023) / 1024;
  if (r > 1024) r = 1024;
  if (r < 1) r = 1;
  return (int)r;
}

// one launch per kernel, T from the entry point's dtype code (UNET_DISPATCH_T / _T16); KK = 2 classes throughout
template <typename T>
static int launch_oc_fwd_vec(int blocks, hipStream_t st, long long P, int HW, int C, int G, const void* y,
                             const float* sc, const float* sf, int relu, const float* w, const float* b, float* out) {
  hipLaunchKernelGGL((outconv_fwd_vec_kernel<T, 2>), dim3(blocks), dim3(256), 0, st, P, HW, C, G, (const T*)y, sc, sf,
                     relu, w, b, out);
  return check_launch("outconv_fwd");
}
template <typename T>
static int launch_oc_fwd(hipStream_t st, long long P, int HW, int C, int K, const void* y, const float* sc,
                         const float* sf, int relu, const float* w, const float* b, float* out) {
  const size_t shm = (size_t)(K * C + 2 * C) * sizeof(float);
  hipLaunchKernelGGL(outconv_fwd_kernel<T>, dim3(grid_for(P, 8192)), dim3(256), shm, st, P, HW, C, K, (const T*)y, sc, sf,
                     relu, w, b, out);
  return check_launch("outconv_fwd");
}
template <typename T>
static int launch_oc_bwd_vec(int rows, hipStream_t st, long long P, int HW, int C, int G, const void* y, const float* sc,
                             const float* sf, int relu, const float* w, const float* dl, float* da, int accum,
                             float* part) {
  hipLaunchKernelGGL((outconv_bwd_vec_kernel<T, 2>), dim3(rows), dim3(256), 0, st, P, HW, C, G, (const T*)y, sc, sf, relu,
                     w, dl, da, accum, part);
  return check_launch("outconv_bwd");
}
template <typename T>
static int launch_oc_bwd(int rows, hipStream_t st, long long P, int HW, int C, int K, const void* y, const float* sc,
                         const float* sf, int relu, const float* w, const float* dl, float* da, int accum, float* part) {
  const int cl = chan_lanes(C);
  hipLaunchKernelGGL(outconv_bwd_kernel<T>, dim3(cdiv(C, cl), rows), dim3(256), 0, st, P, HW, C, cl, K, (const T*)y, sc,
                     sf, relu, w, dl, da, accum, part, rows);
  return check_launch("outconv_bwd");
}
template <typename T>
static int launch_oc_bwd_bn(int rows, hipStream_t st, long long P, int HW, int C, const void* y, const float* sc,
                            const float* sf, int relu, const float* w, const float* dl, const float* mean,
                            const float* invstd, float* part, float* bpart) {
  hipLaunchKernelGGL((outconv_bwd_bn_kernel<T, 2>), dim3(rows), dim3(256), 0, st, P, HW, C, C / 8, (const T*)y, sc, sf,
                     relu, w, dl, mean, invstd, part, bpart, rows);
  return check_launch("outconv_bwd_bn");
}
template <typename T>
static int launch_bn_bwd_apply_oc(int blocks, hipStream_t st, long long P, int HW, int C, const void* y, const float* sc,
                                  const float* sf, int relu, const float* w, const float* dl, const float* coef,
                                  void* dy) {
  hipLaunchKernelGGL((bn_bwd_apply_oc_kernel<T, 2>), dim3(blocks), dim3(256), 0, st, P, HW, C, (const T*)y, sc, sf, relu,
                     w, dl, coef, (T*)dy);
  return check_launch("bn_bwd_apply_oc");
}

}  // namespace unet

using namespace unet;

extern "C" {

int unet_outconv_rows(long long P) { return oc_rows(P); }

int unet_outconv_fwd(int dtype, long long N, int H, int W, int C, int K, const void* y, const float* scale,
                     const float* shift, int relu, const float* w, const float* b, float* logits, void* stream) {
  if (K > OC_MAXK || K < 1) { set_error("unet_outconv_fwd: n_classes > 8 unsupported"); return UNET_ERR_UNSUPPORTED; }
  const long long P = N * H * (long long)W;
  hipStream_t st = (hipStream_t)stream;
  const int G = (C % 8 == 0 && C / 8 <= 64 && ((C / 8) & (C / 8 - 1)) == 0) ? C / 8 : 0;
  if (G && K == 2) {
    long long blocks = (P * G + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    return UNET_DISPATCH_T(dtype, launch_oc_fwd_vec<T>((int)blocks, st, P, H * W, C, G, y, scale, shift, relu, w, b, logits));
  }
  return UNET_DISPATCH_T(dtype, launch_oc_fwd<T>(st, P, H * W, C, K, y, scale, shift, relu, w, b, logits));
}

int unet_outconv_bwd(int dtype, long long N, int H, int W, int C, int K, const void* y, const float* scale,
                     const float* shift, int relu, const float* w, const float* dl, float* da, int accum, float* partial,
                     void* stream) {
  if (K > OC_MAXK || K < 1 || C < K) { set_error("unet_outconv_bwd: need 1 <= n_classes <= min(8, C)"); return UNET_ERR_UNSUPPORTED; }
  const long long P = N * H * (long long)W;
  const int rows = oc_rows(P);
  hipStream_t st = (hipStream_t)stream;
  const int G = (C % 8 == 0 && C / 8 <= 256 && ((C / 8) & (C / 8 - 1)) == 0) ? C / 8 : 0;
  if (dtype != UNET_F32 && G && K == 2)
    return UNET_DISPATCH_T16(dtype, launch_oc_bwd_vec<T>(rows, st, P, H * W, C, G, y, scale, shift, relu, w, dl, da, accum,
                                                         partial));
  return UNET_DISPATCH_T(dtype, launch_oc_bwd<T>(rows, st, P, H * W, C, K, y, scale, shift, relu, w, dl, da, accum, partial));
}

int unet_outconv_bwd_bn(int dtype, long long N, int H, int W, int C, int K, const void* y, const float* scale,
                        const float* shift, int relu, const float* w, const float* dl, const float* mean,
                        const float* invstd, float* partial, float* bn_partial, void* stream) {
  const long long P = N * H * (long long)W;
  const int G = C / 8;
  if (K != 2 || C % 8 || G > 256 || (G & (G - 1)) || !scale || !shift || !mean || !invstd || P >= (1LL << 31)) {
    set_error("unet_outconv_bwd_bn: needs n_classes == 2, C % 8 == 0, C/8 a power of two <= 256, a BN activation");
    return UNET_ERR_UNSUPPORTED;
  }
  return UNET_DISPATCH_T(dtype, launch_oc_bwd_bn<T>(oc_rows(P), (hipStream_t)stream, P, H * W, C, y, scale, shift, relu, w,
                                                    dl, mean, invstd, partial, bn_partial));
}

int unet_bn_bwd_apply_oc(int dtype, long long N, int H, int W, int C, int K, const void* y, const float* scale,
                         const float* shift, int relu, const float* w, const float* dl, const float* coef, void* dy,
                         void* stream) {
  const long long P = N * H * (long long)W;
  const int CV = C / 8;
  if (K != 2 || C % 8 || CV > 256 || (CV & (CV - 1)) || P >= (1LL << 31)) {
    set_error("unet_bn_bwd_apply_oc: needs n_classes == 2, C % 8 == 0, C/8 a power of two <= 256");
    return UNET_ERR_UNSUPPORTED;
  }
  long long b = (P * CV + 255) / 256;
  if (b > 8192) b = 8192;
  return UNET_DISPATCH_T(dtype, launch_bn_bwd_apply_oc<T>((int)b, (hipStream_t)stream, P, H * W, C, y, scale, shift, relu,
                                                          w, dl, coef, dy));
}

int unet_outconv_bwd_finalize(const float* partial, int rows, int C, int K, float* dw, float* db, int accum,
                              void* stream) {
  const int total = K * C + K;
  hipLaunchKernelGGL(outconv_bwd_finalize_kernel, dim3(total), dim3(256), 0, (hipStream_t)stream, partial, rows, C, K,
                     dw, db, accum);
  return check_launch("outconv_bwd_finalize");
}

}  // extern "C"
