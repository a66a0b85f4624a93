// bn_gate.hip — the pooled BatchNorm backward of an attention Up block's skip activation, with the gate's
// gradient of that activation formed on the fly instead of read from a stored fp32 map.
//
// Reference: AttentionGate's x * psi and W_x(x) (layers.py:187-192) feed the encoder activation x, whose
// BatchNorm2d(+ReLU) backward (layers.py:36-37) also takes the MaxPool2d(2) backward of the Down block below
// (layers.py:56).  The three-launch form stores
//   dx = W_x^T dxw + sigmoid(a p + b) * d(x s)          (pw_conv_kernel<..., 2, ...>, UNET_OUT_F32_GATED)
// and unet_bn_bwd_reduce_pool / unet_bn_bwd_apply_pool read it back as `da`.  The two kernels here are those two
// passes with `da` replaced by the operands of that dgrad; the result is defined as the bits of the three
// launches:
//  * g = (the MFMA chain over the Ci/32 chunks in order, from a zero accumulator) + (dxs * s): the product rounded
//    on its own, one fp32 add — the GATED epilogue of pw.hip with accum == 0; an MFMA output element is the dot
//    product of its own row and column, so the 16-pixel tiling here changes nothing;
//  * the routed pooled gradient is added to g, then the ReLU mask, then the sums / the apply (bn.hip);
//  * the reduce pass keeps bn_bwd_reduce_vec_kernel<.., POOL>'s summation order: partial row b owns the pixels
//    [b per, (b+1) per); per channel R = 256 / (C/8) running sums over p0 + py, p0 + py + R, ..., each from +0 in
//    that order, then summed from 0.f in order py = 0 .. R-1.
// Layout: a wave owns 16-pixel tiles x 32 channels (two 16-channel MFMA tiles); after a v_permlane16_swap of the
// two accumulators lane (i16, g) holds the 8 contiguous channels cb + 16 (g & 1) + 8 (g >> 1) .. + 7 of pixel
// i16.  In the reduce pass a lane's running sum over the tiles t, t + R/16, ... of its block is exactly the chain
// (py = 16 (t mod R/16) + i16, c), so the block's four waves are (R/16 tile classes) x (C/32 channel groups):
// C 64 -> 2 x 2, C 128 -> 1 x 4.  Those are the shapes served (the 512^2 and 256^2 levels of the bs-4
// AttentionUNet); the W_x fragments (2 x Ci/32 per wave) stay in registers.
#include "conv_common.h"

namespace unet {

struct GateBnArgs {
  const float* dxs;      // d(x s), fp32 [P][C]
  const void* dxw;       // W_x's output gradient, 16-bit [P][Ci]
  const void* wt;        // packed transposed W_x (the dgrad's weight operand)
  const float* gate_p;   // psi's pre-activation [P]
  const float* gate_ab;  // psi-BN scale / shift
  const float* g2;       // pooled gradient fp32 [N][ph][pw][C]
  const uint8_t* code;   // argmax codes, same shape
  int H, W, ph, pw;
};

// one lane's operands of a (16 pixels x 32 channels) tile, all loaded before any is used
template <int NCH>
struct GateBnTile {
  uint4 xw[NCH];
  float4 dxs[2], g2[2];
  uint4 y;
  uint2 code;
  float gp;
  bool pool;
};

// (n, h, w) of pixel p: 32-bit math, the host admits N*H*W < 2^31
struct GbPix {
  unsigned n, h, w;
};
__device__ __forceinline__ GbPix gb_pix(const GateBnArgs& a, unsigned p) {
  const unsigned W = (unsigned)a.W, H = (unsigned)a.H;
  const unsigned t = p / W, w = p - t * W;
  const unsigned n = t / H;
  return GbPix{n, t - n * H, w};
}
// advanced in place by a fixed pixel step sq * W + sr (sr < W)
__device__ __forceinline__ void gb_adv(GbPix& c, const GateBnArgs& a, unsigned sq, unsigned sr) {
  c.w += sr;
  unsigned h = c.h + sq;
  if (c.w >= (unsigned)a.W) { c.w -= (unsigned)a.W; ++h; }
  while (h >= (unsigned)a.H) { h -= (unsigned)a.H; ++c.n; }
  c.h = h;
}

// the 8 contiguous channels lane row g owns once the two MFMA tiles' accumulators are swapped (gb_form)
__device__ __forceinline__ int gb_c8(int cb, int g) { return cb + 16 * (g & 1) + 8 * (g >> 1); }

// p: the pixel whose operands are loaded (always inside the map); ok: it is this lane's own pixel px (a lane past
// the end of its range loads some valid pixel for the MFMA and takes no pooled gradient: px may lie past the map)
template <typename T, int NCH>
__device__ __forceinline__ void gb_load(GateBnTile<NCH>& t, const GateBnArgs& a, const T* y, int C, long long p,
                                        bool ok, const GbPix& px, int c8, int g) {
  const T* xw = (const T*)a.dxw + p * (32 * NCH) + 8 * g;
#pragma unroll
  for (int c = 0; c < NCH; ++c) t.xw[c] = *reinterpret_cast<const uint4*>(xw + 32 * c);
  t.gp = a.gate_p[p];
  t.dxs[0] = *reinterpret_cast<const float4*>(a.dxs + p * C + c8);
  t.dxs[1] = *reinterpret_cast<const float4*>(a.dxs + p * C + c8 + 4);
  t.y = *reinterpret_cast<const uint4*>(y + p * C + c8);
  const unsigned hh = px.h >> 1, ww = px.w >> 1;
  t.pool = ok && hh < (unsigned)a.ph && ww < (unsigned)a.pw;
  if (t.pool) {
    const size_t o = (size_t)((px.n * (unsigned)a.ph + hh) * (unsigned)a.pw + ww) * C + c8;
    t.g2[0] = *reinterpret_cast<const float4*>(a.g2 + o);
    t.g2[1] = *reinterpret_cast<const float4*>(a.g2 + o + 4);
    t.code = *reinterpret_cast<const uint2*>(a.code + o);
  } else {
    t.g2[0] = t.g2[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    t.code = make_uint2(0xffffffffu, 0xffffffffu);   // matches no window position
  }
}

// gv[j]: the gradient of channel c8 + j before the ReLU mask; yv[j]: the stored conv output
template <typename T, int NCH>
__device__ __forceinline__ void gb_form(const GateBnTile<NCH>& t, const uint4 (&wq)[2][NCH], float ga, float gb,
                                        const GbPix& px, float (&gv)[8], float (&yv)[8]) {
  typedef typename Mma<T>::frag F;
  // psi's sigmoid as the dgrad's epilogue forms it (the pre-activation is one fma there)
  const float s = sigmoidf_(__builtin_fmaf(t.gp, ga, gb));
  const unsigned q = (px.h & 1) * 2 + (px.w & 1);
  f32x4 acc[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      acc[k] = Mma<T>::mma(__builtin_bit_cast(F, wq[k][c]), __builtin_bit_cast(F, t.xw[c]), acc[k]);
  }
  // accumulator lane (i16, g) holds channels 16 k + 4 g + r of pixel i16: v_permlane16_swap of the (tile 0,
  // tile 1) pairs leaves row g with the 8 contiguous channels 16 (g & 1) + 8 (g >> 1) .. + 7 (pw.hip's y epilogue),
  // which is how every other operand is loaded: 32-byte fp32 and 16-byte 16-bit vectors, as bn.hip's passes
  float m[8];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[0][r]), __float_as_uint(acc[1][r]), false,
                                                     false);
    m[r] = __uint_as_float(sw[0]);
    m[4 + r] = __uint_as_float(sw[1]);
  }
  const float x[8] = {t.dxs[0].x, t.dxs[0].y, t.dxs[0].z, t.dxs[0].w, t.dxs[1].x, t.dxs[1].y, t.dxs[1].z, t.dxs[1].w};
  const float v[8] = {t.g2[0].x, t.g2[0].y, t.g2[0].z, t.g2[0].w, t.g2[1].x, t.g2[1].y, t.g2[1].z, t.g2[1].w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // the product is rounded before the add (f32_rounded keeps the compiler from contracting the two)
    float gg = m[j] + f32_rounded(x[j] * s);
    const unsigned cj = ((j < 4 ? t.code.x : t.code.y) >> (8 * (j & 3))) & 0xffu;
    if (cj == q) gg += v[j];
    gv[j] = gg;
  }
  unpack8_16<T>(t.y, yv);
}

template <int NCH>
__device__ __forceinline__ void gb_weights(const GateBnArgs& a, int cb, int lane, uint4 (&wq)[2][NCH]) {
  // packed [16-channel tile][chunk][64 lanes][16 B]
  const uint4* w = reinterpret_cast<const uint4*>(a.wt);
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int c = 0; c < NCH; ++c) wq[k][c] = w[(size_t)((cb / 16 + k) * NCH + c) * 64 + lane];
}

// grid = rows (unet_bn_bwd_reduce_rows), block = 256
template <typename T, int NCH>
__global__ __launch_bounds__(256) void bn_bwd_reduce_pool_gate_kernel(long long P, int C, const GateBnArgs a,
                                                                      const T* __restrict__ y, const float* scale,
                                                                      const float* shift, int relu, const float* mean,
                                                                      const float* invstd, float* part, int rows) {
  __shared__ float sh[2][2048];   // [R][C]: 32 x 64 or 16 x 128
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int np = 128 / C;          // tile classes = R / 16 (C 64: 2, C 128: 1)
  const int cls = wave % np, cb = 32 * (wave / np);
  const int R = 16 * np, py = 16 * cls + i16;
  const long long per = (P + rows - 1) / rows;
  const long long p0 = blockIdx.x * per, p1 = min(P, p0 + per);

  uint4 wq[2][NCH];
  gb_weights<NCH>(a, cb, lane, wq);
  const float ga = a.gate_ab[0], gb = a.gate_ab[1];
  const int c8 = gb_c8(cb, g);
  float sc[8], sf[8], mu[8], is[8], sg[8], sgx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = scale[c8 + j]; sf[j] = shift[c8 + j]; mu[j] = mean[c8 + j]; is[j] = invstd[c8 + j];
    sg[j] = 0.f; sgx[j] = 0.f;
  }
  // this lane's pixel sequence p0 + py, + R, ...: its (n, h, w) advance by the fixed step R (no division per pixel)
  const unsigned sq = (unsigned)R / (unsigned)a.W, sr = (unsigned)R - sq * (unsigned)a.W;
  GbPix px{0, 0, 0};
  if (p0 + py < p1) px = gb_pix(a, (unsigned)(p0 + py));
  // the trip count is wave-uniform (the MFMAs need the whole wave); a lane past p1 loads its tile's first pixel
  // and adds nothing
  for (long long pt = p0 + 16 * cls; pt < p1; pt += R) {
    const bool ok = pt + i16 < p1;
    GateBnTile<NCH> t;
    gb_load<T, NCH>(t, a, y, C, ok ? pt + i16 : pt, ok, px, c8, g);
    float gv[8], yv[8];
    gb_form<T, NCH>(t, wq, ga, gb, px, gv, yv);
    gb_adv(px, a, sq, sr);
    if (ok) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gj = (relu && !(__builtin_fmaf(yv[j], sc[j], sf[j]) > 0.f)) ? 0.f : gv[j];
        sg[j] += gj;
        // (the contraction bn_bwd_reduce_vec_kernel compiles to, written out)
        sgx[j] = __builtin_fmaf(gj * (yv[j] - mu[j]), is[j], sgx[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sh[0][py * C + c8 + j] = sg[j];
    sh[1][py * C + c8 + j] = sgx[j];
  }
  __syncthreads();
  if (tid < C) {
    float u = 0.f, v = 0.f;
    for (int r = 0; r < R; ++r) { u += sh[0][r * C + tid]; v += sh[1][r * C + tid]; }
    part[(size_t)blockIdx.x * C + tid] = u;
    part[((size_t)rows + blockIdx.x) * C + tid] = v;
  }
}

// grid-strided over (16-pixel tile, 32-channel group) items, one per wave and trip
template <typename T, int NCH>
__global__ __launch_bounds__(256) void bn_bwd_apply_pool_gate_kernel(long long P, int C, const GateBnArgs a,
                                                                     const T* y, const float* scale,
                                                                     const float* shift, int relu, const float* coef,
                                                                     T* dy) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int ncg = C / 32;                                   // 2 or 4: divides the 4 waves of a block
  const long long wg = (long long)blockIdx.x * 4 + wave;
  const int cb = 32 * (int)(wg % ncg);                      // fixed: the wave stride is a multiple of ncg
  const long long ntiles = (P + 15) / 16, tstride = (long long)gridDim.x * 4 / ncg;
  uint4 wq[2][NCH];
  gb_weights<NCH>(a, cb, lane, wq);
  const float ga = a.gate_ab[0], gb = a.gate_ab[1];
  const int c8 = gb_c8(cb, g);
  float sc[8], sf[8], A[8], B[8], Cc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c8 + j;
    sc[j] = scale[c]; sf[j] = shift[c]; A[j] = coef[c]; B[j] = coef[C + c]; Cc[j] = coef[2 * C + c];
  }
  // one tile per trip: two (every load of both ahead of the stores, as bn_bwd_apply_vec_kernel) took 139-151
  // registers, 3 waves per SIMD, and measured 132.1 against 128.3 us at 512^2, 76.3 against 75.9 at 256^2
  constexpr int U = 1;
  for (long long t0 = wg / ncg; t0 < ntiles; t0 += U * tstride) {
    GateBnTile<NCH> t[U];
    GbPix px[U];
    long long pu[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long tt = t0 + u * tstride;
      const long long p = tt * 16 + i16;
      ok[u] = tt < ntiles && p < P;
      pu[u] = ok[u] ? p : t0 * 16;           // (a lane past the end reloads a valid pixel and stores nothing)
      px[u] = gb_pix(a, (unsigned)pu[u]);
      gb_load<T, NCH>(t[u], a, y, C, pu[u], ok[u], px[u], c8, g);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float gv[8], yv[8];
      gb_form<T, NCH>(t[u], wq, ga, gb, px[u], gv, yv);
      if (!ok[u]) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gj = (relu && !(__builtin_fmaf(yv[j], sc[j], sf[j]) > 0.f)) ? 0.f : gv[j];
        o[j] = f32_rounded(__builtin_fmaf(A[j], gj, __builtin_fmaf(B[j], yv[j], Cc[j])));
      }
      store_vec<T>(dy + pu[u] * C + c8, o);
    }
  }
}

static bool gate_bn_shape_ok(int dtype, long long N, int H, int W, int C, int Ci, int ph, int pw) {
  if (dtype != UNET_BF16 && dtype != UNET_F16) return false;
  if (N <= 0 || H <= 0 || W <= 0) return false;
  const long long P = N * H * W;
  if (P >= (1LL << 31) || ph < 0 || pw < 0 || ph > (H >> 1) || pw > (W >> 1)) return false;
  return (C == 64 || C == 128) && (Ci == 32 || Ci == 64);
}

}  // namespace unet

using namespace unet;

extern "C" {

int unet_bn_bwd_pool_gate_ok(int dtype, long long N, int H, int W, int C, int Ci) {
  return gate_bn_shape_ok(dtype, N, H, W, C, Ci, H >> 1, W >> 1) ? 1 : 0;
}

int unet_bn_bwd_reduce_pool_gate(int dtype, long long N, int H, int W, int C, int Ci, const float* dxs,
                                 const void* dxw, const void* wt_packed, const float* gate_p, const float* gate_ab,
                                 const float* g2, const uint8_t* code, int ph, int pw, const void* y,
                                 const float* scale, const float* shift, int relu, const float* mean,
                                 const float* invstd, float* partial, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!gate_bn_shape_ok(dtype, N, H, W, C, Ci, ph, pw) || !dxs || !dxw || !wt_packed || !gate_p || !gate_ab || !g2 ||
      !code || !y || !partial) {
    set_error("unet_bn_bwd_reduce_pool_gate: bad arguments (16-bit, C 64 / 128, Ci 32 / 64)");
    return UNET_ERR_ARG;
  }
  const long long P = N * H * W;
  const GateBnArgs a{dxs, dxw, wt_packed, gate_p, gate_ab, g2, code, H, W, ph, pw};
  const int rows = unet_bn_bwd_reduce_rows(P, C);
  if (dtype == UNET_F16) {
    if (Ci == 32)
      hipLaunchKernelGGL((bn_bwd_reduce_pool_gate_kernel<f16, 1>), dim3(rows), dim3(256), 0, st, P, C, a, (const f16*)y,
                         scale, shift, relu, mean, invstd, partial, rows);
    else
      hipLaunchKernelGGL((bn_bwd_reduce_pool_gate_kernel<f16, 2>), dim3(rows), dim3(256), 0, st, P, C, a, (const f16*)y,
                         scale, shift, relu, mean, invstd, partial, rows);
  } else {
    if (Ci == 32)
      hipLaunchKernelGGL((bn_bwd_reduce_pool_gate_kernel<bf16, 1>), dim3(rows), dim3(256), 0, st, P, C, a,
                         (const bf16*)y, scale, shift, relu, mean, invstd, partial, rows);
    else
      hipLaunchKernelGGL((bn_bwd_reduce_pool_gate_kernel<bf16, 2>), dim3(rows), dim3(256), 0, st, P, C, a,
                         (const bf16*)y, scale, shift, relu, mean, invstd, partial, rows);
  }
  return check_launch("bn_bwd_reduce_pool_gate");
}

int unet_bn_bwd_apply_pool_gate(int dtype, long long N, int H, int W, int C, int Ci, const float* dxs,
                                const void* dxw, const void* wt_packed, const float* gate_p, const float* gate_ab,
                                const float* g2, const uint8_t* code, int ph, int pw, const void* y,
                                const float* scale, const float* shift, int relu, const float* coef, void* dy,
                                void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!gate_bn_shape_ok(dtype, N, H, W, C, Ci, ph, pw) || !dxs || !dxw || !wt_packed || !gate_p || !gate_ab || !g2 ||
      !code || !y || !coef || !dy) {
    set_error("unet_bn_bwd_apply_pool_gate: bad arguments (16-bit, C 64 / 128, Ci 32 / 64)");
    return UNET_ERR_ARG;
  }
  const long long P = N * H * W;
  const GateBnArgs a{dxs, dxw, wt_packed, gate_p, gate_ab, g2, code, H, W, ph, pw};
  // one (tile, channel group) item per wave: 512 elements, as a thread of bn_bwd_apply_vec_kernel owns 8
  long long b = ((P + 15) / 16 * (C / 32) + 3) / 4;
  if (b > 8192) b = 8192;
  if (dtype == UNET_F16) {
    if (Ci == 32)
      hipLaunchKernelGGL((bn_bwd_apply_pool_gate_kernel<f16, 1>), dim3((int)b), dim3(256), 0, st, P, C, a, (const f16*)y,
                         scale, shift, relu, coef, (f16*)dy);
    else
      hipLaunchKernelGGL((bn_bwd_apply_pool_gate_kernel<f16, 2>), dim3((int)b), dim3(256), 0, st, P, C, a, (const f16*)y,
                         scale, shift, relu, coef, (f16*)dy);
  } else {
    if (Ci == 32)
      hipLaunchKernelGGL((bn_bwd_apply_pool_gate_kernel<bf16, 1>), dim3((int)b), dim3(256), 0, st, P, C, a,
                         (const bf16*)y, scale, shift, relu, coef, (bf16*)dy);
    else
      hipLaunchKernelGGL((bn_bwd_apply_pool_gate_kernel<bf16, 2>), dim3((int)b), dim3(256), 0, st, P, C, a,
                         (const bf16*)y, scale, shift, relu, coef, (bf16*)dy);
  }
  return check_launch("bn_bwd_apply_pool_gate");
}

}  // extern "C"
